"""CPU: the sampling controls of lstm_hip_generate_ex (include/lstm_hip.h) without a device -- the
reference filter's own invariants on oracle distributions, the control of the GPU oracle comparison (how often its
distributions are ambiguous, and whether the filter cuts anything on them), the header and the program's --help."""
import os
import re
import subprocess

import numpy as np

import sampling_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 256


def _trajectories(orc):
    """per stream of the shared case: the temperature-1 distributions [count, 256] along an oracle32.sample trajectory"""
    N = sr.ORACLE_N
    P, prompts, u = sr.oracle_case()
    dists = []
    for s in range(sr.ORACLE_STREAMS):
        xi = np.full((2, 1), -1, np.int32)
        xi[1, 0] = prompts[s][0]
        fw = orc.forward(N, M, 2, 1, P, xi, np.full((2, 1), -1, np.int32), np.zeros((1, N), np.float32),
                         np.zeros((1, N), np.float32))
        drawn, _, _ = orc.sample(N, M, P, fw["h"][1][0], fw["c"][1][0], u[:, s])
        dists.append(sr.replay(orc, N, P, prompts[s], drawn))
    return dists, u


def test_reference_filter_invariants_on_oracle_distributions(oracle32):
    N = 64
    P, xi, ti, h0, c0 = sr.gu.random_case(N, 6, 3, seed=5, scale=0.2)
    P = sr.peaked_params(N, seed=5)
    fw = oracle32.forward(N, M, 6, 3, P, xi, ti, h0, c0)
    rs = np.random.RandomState(6)
    for p1 in np.asarray(fw["probs"][1:], np.float64).reshape(-1, M):
        for top_k, top_p, tau in ((0, 1.0, 1.0), (1, 1.0, 1.0), (1, 1.0, 0.7), (40, 1.0, 1.0), (0, 0.9, 1.0), (40, 0.9, 0.8),
                                  (5, 0.5, 1.5), (255, 0.999, 1.0), (0, 1e-30, 1.0)):
            p = sr.tempered(p1, tau)
            r = sr.ranks(p1)
            assert sorted(r) == list(range(M))  # a total order
            keep, mask, q = sr.filter64(p1, p, top_k, top_p)
            cum = np.cumsum(p[np.argsort(r)])
            nucleus = int(np.nonzero(cum >= top_p)[0][0]) + 1 if top_p < 1.0 and (cum >= top_p).any() else 256
            assert keep == min(top_k if 1 <= top_k <= 255 else 256, nucleus) and keep >= 1
            assert mask.sum() == keep and np.array_equal(mask, r < keep)
            assert abs(q.sum() - 1.0) <= 1e-12 and not q[~mask].any()
            if top_k == 1 or top_p == 1e-30:
                assert keep == 1 and mask[int(np.argmax(p1))]
            u = rs.random_sample()
            x, keep32, q32 = sr.draw32(p1, p.astype(np.float32), top_k, top_p, u)
            assert mask[x] or sr.ambiguous(p, top_k, top_p)
            assert abs(float(q32.astype(np.float64).sum()) - 1.0) <= 1e-5
            # u past every edge: the largest kept index
            x, keep32, _ = sr.draw32(p1, p.astype(np.float32), top_k, top_p, 2.0)
            kept32 = sr.ranks(p1) < keep32
            assert x == int(np.nonzero(kept32)[0].max())


def test_top_k_one_takes_the_lowest_index_on_ties():
    z = np.zeros(M, np.float32)
    z[[200, 17, 90]] = 3.0  # three equal maxima
    p = np.exp(z - z.max())
    p = (p / p.sum()).astype(np.float32)
    assert sr.ranks(z)[17] == 0 and sr.ranks(z)[90] == 1 and sr.ranks(z)[200] == 2
    for u in (0.0, 0.3, 0.999999, 1.0):
        x, keep, q = sr.draw32(z, p, 1, 1.0, u)
        assert (x, keep) == (17, 1) and q[17] == 1.0 and q.sum() == 1.0
    keep, mask, _ = sr.filter64(z, p, 2, 1.0)
    assert keep == 2 and list(np.nonzero(mask)[0]) == [17, 90]
    # all logits equal: ranks are the indices
    assert np.array_equal(sr.ranks(np.zeros(M)), np.arange(M))


def test_control_of_the_gpu_oracle_comparison(oracle32):
    """The GPU test skips draws whose distribution is ambiguous and asserts that they are at most 5 %: here the same
    parameters, seeds and settings on oracle32.sample trajectories, without a device.  And the filter must do something
    on them: the mean kept count under the top-p settings lies between 5 and 100 of 256."""
    dists, _ = _trajectories(oracle32)
    for top_k, top_p, tau in sr.ORACLE_SETTINGS:
        amb, keeps = [], []
        for d in dists:
            for p1 in d:
                p = sr.tempered(p1, tau)
                amb.append(sr.ambiguous(p, top_k, top_p))
                keeps.append(sr.filter64(p1, p, top_k, top_p)[0])
        print(f"top_k {top_k} top_p {top_p} tau {tau}: ambiguous {np.mean(amb):.4f}, mean kept {np.mean(keeps):.2f}")
        assert np.mean(amb) <= 0.05, (top_k, top_p, tau, np.mean(amb))
        if top_p < 1.0:
            assert 5.0 <= np.mean(keeps) <= 100.0, (top_k, top_p, tau, np.mean(keeps))


def test_header_declares_the_call_and_its_options():
    header = open(os.path.join(ROOT, "include", "lstm_hip.h")).read()
    assert re.search(r"int lstm_hip_generate_ex\(lstm_hip_t \*h, int32_t streams,", header)
    m = re.search(r"typedef struct lstm_hip_sampling \{(.*?)\} lstm_hip_sampling;", header, re.S)
    assert m
    fields = re.findall(r"^\s*(\w+)\s+(\w+);", m.group(1), re.M)
    assert fields == [("uint32_t", "size"), ("double", "temperature"), ("int32_t", "top_k"), ("double", "top_p"),
                      ("int32_t", "stop_byte")], fields
    import ctypes as C
    import lstm_hip
    assert "lstm_hip_generate_ex" in lstm_hip.SYMBOLS
    assert C.sizeof(lstm_hip._Sampling) == 40 and lstm_hip._Sampling.top_p.offset == 24  # the C layout on this ABI


def test_program_help_names_the_three_flags():
    exe = os.path.join(ROOT, "eigen-lstm_amd", "lstm_generate")
    out = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    for flag in ("--top-k", "--top-p", "--stop-byte"):
        assert flag in out.stdout, flag
    for bad in (["--top-k", "257"], ["--top-p", "0"], ["--top-p", "1.5"], ["--stop-byte", "256"], ["--stop-byte", "x"]):
        r = subprocess.run([exe, "--load", "nowhere", "--count", "1"] + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (bad, r.returncode, r.stderr)
