"""-m gpu: lstm_hip_beam_search (include/lstm_hip.h).

With one beam the search is greedy decoding, byte for byte; a hypothesis's cost is the sum the LSTM_HIP_STABLE_SOFTMAX prompt
scorer makes of the same text, bit for bit (the same double sequence of the same float terms); against the float64 rule
through the oracle (tests/beam_ref.py, whose margins tests/test_beam_search_cpu.py controls) hypotheses and lengths are
equal and costs agree within 1e-4 bits."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import beam_ref as br
import gpu_util as gu
from test_pad_hidden import pad_cols, pad_params, padded_width

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(N, seed, scale=0.3):
    return gu.random_case(N, 2, 1, seed=seed, scale=scale)[0]


def _state(streams, N, seed):
    rs = np.random.RandomState(seed)
    return (rs.randn(streams, N) * 0.1).astype(np.float32), (rs.randn(streams, N) * 0.1).astype(np.float32)


def _prompts(lengths, seed):
    rs = np.random.RandomState(seed)
    return [rs.randint(32, 127, size=n).astype(np.uint8) for n in lengths]


def _handle(N, P, flags=0, B=1):
    import lstm_hip
    L = lstm_hip.Lstm(N, 2, B, flags=flags)
    L.set_params(P)
    return L


def _control_prompts():
    return [np.array([b], np.uint8) for b in br.CONTROL_PROMPTS]


def _check_shape_of_a_result(res, W, count, stop):
    """what holds for every search: distinct hypotheses in cost order; a finished one ends in its only stop byte"""
    for hyps in res:
        texts = [t for t, _ in hyps]
        assert len(hyps) == W and len(set(texts)) == W, texts
        bits = [b for _, b in hyps]
        assert all(bits[r] <= bits[r + 1] for r in range(W - 1)), bits
        for t in texts:
            if stop >= 0 and stop in t:
                assert t.index(bytes([stop])) == len(t) - 1, t
            else:
                assert len(t) == count, t


@pytest.mark.parametrize("N", [64, 192, 512])   # (192: a width the plan puts on the per-step engine)
def test_one_beam_is_greedy_decoding(N):
    count = 40
    P = _params(N, seed=3, scale=0.3 if N == 64 else 0.1)
    prompts = _prompts([0, 3, 1, 17], seed=4)
    h0, c0 = _state(4, N, seed=5)
    L = _handle(N, P)
    want = L.generate(prompts, count=count, temperature=0.0, h0=h0, c0=c0)[0]
    got = L.beam_search(prompts, count=count, beams=1, h0=h0, c0=c0)
    zero = L.beam_search(prompts, count=count, beams=1)
    want0 = L.generate(prompts, count=count, temperature=0.0)[0]
    L.close()
    for s in range(4):
        assert got[s][0][0] == want[:, s].tobytes(), s
        assert zero[s][0][0] == want0[:, s].tobytes(), s
        assert np.isfinite(got[s][0][1]) and got[s][0][1] > 0.0


@pytest.mark.parametrize("stable", [True, False])
def test_costs_are_the_prompt_scorers_sums(stable):
    import lstm_hip
    N, W, count = br.CONTROL_N, 4, 16
    prompts = _control_prompts()
    L = _handle(N, br.control_params(), flags=lstm_hip.STABLE_SOFTMAX if stable else 0)
    free = L.beam_search(prompts, count=count, beams=W)
    stop = free[0][0][0][5]
    for stop_byte in (-1, stop):
        res = L.beam_search(prompts, count=count, beams=W, stop_byte=stop_byte)
        _check_shape_of_a_result(res, W, count, stop_byte)
        texts = [bytes(prompts[s]) + t for s in range(4) for t, _ in res[s]]
        scored = L.generate(texts, count=0, score=True)[1]
        got = np.array([b for s in range(4) for _, b in res[s]])
        print("largest difference to the scorer: %.3g bits" % np.abs(got - scored).max())
        if stable:
            assert got.tobytes() == scored.tobytes(), (got, scored)
        else:
            assert np.abs(got - scored).max() <= 1e-4, np.abs(got - scored).max()
    L.close()


@pytest.mark.parametrize("W", br.CONTROL_BEAMS)
def test_hypotheses_against_the_float64_rule(W, oracle64):
    N, count = br.CONTROL_N, br.CONTROL_COUNT
    P = br.control_params()
    prompts = _control_prompts()
    L = _handle(N, P)
    worst = 0.0
    for stopped in (False, True):
        stops = [-1] * 4
        if stopped:
            stops = [br.beam64(oracle64, N, P, p, W, count)["hyps"][0][br.CONTROL_STOP_AT] for p in prompts]
        for s, p in enumerate(prompts):  # (the stop byte is the stream's own: one call per stream)
            want = br.beam64(oracle64, N, P, p, W, count, stops[s])
            got, raw = L.beam_search([p], count=count, beams=W, stop_byte=stops[s], trace=True)
            assert [t for t, _ in got[0]] == want["hyps"], (s, stopped)
            assert list(raw["out_len"][0]) == want["length"], (s, stopped)
            diff = np.abs(np.array([b for _, b in got[0]]) - np.array(want["bits"])).max()
            worst = max(worst, diff)
            assert diff <= 1e-4, (s, stopped, diff)
            if stopped:
                assert any(want["fin"]), s
    L.close()
    print("largest cost difference to float64: %.3g bits" % worst)


def test_the_tables_walk_back_to_the_hypotheses():
    N, W, count = 64, 8, 20
    prompts = _prompts([2, 0, 9, 1], seed=21)
    L = _handle(N, br.control_params())
    free = L.beam_search(prompts, count=count, beams=W)
    for stop in (-1, free[1][0][0][3]):
        res, raw = L.beam_search(prompts, count=count, beams=W, stop_byte=stop, trace=True)
        _check_shape_of_a_result(res, W, count, stop)
        tp, tb = raw["parent"].reshape(count, 4, W), raw["byte"].reshape(count, 4, W)
        assert tp.max() < W
        assert not tp[0].any()  # the first selection expands slot 0 only
        for s in range(4):
            hyps = br.backtrack(tp[:, s].tolist(), tb[:, s].tolist(), raw["out_len"][s].tolist(), W, count)
            assert hyps == [t for t, _ in res[s]], s
            for r in range(W):
                n = raw["out_len"][s, r]
                assert raw["out"][s, r, :n].tobytes() == hyps[r] and not raw["out"][s, r, n:].any(), (s, r)
    L.close()


def test_a_wide_batch_equals_its_streams_four_at_a_time():
    N, K, W, count = 64, 512, 8, 8
    rs = np.random.RandomState(31)
    lengths = rs.randint(0, 6, size=K)
    prompts = _prompts(lengths, seed=32)
    h0, c0 = _state(K, N, seed=33)
    L = _handle(N, br.control_params())
    _, wide = L.beam_search(prompts, count=count, beams=W, h0=h0, c0=c0, trace=True)
    for k in range(0, K, 4):
        _, small = L.beam_search(prompts[k:k + 4], count=count, beams=W, h0=h0[k:k + 4], c0=c0[k:k + 4], trace=True)
        assert np.array_equal(wide["out"][k:k + 4], small["out"]), k
        assert np.array_equal(wide["out_len"][k:k + 4], small["out_len"]), k
        assert wide["bits"][k:k + 4].tobytes() == small["bits"].tobytes(), k
        for name in ("parent", "byte"):
            assert np.array_equal(wide[name][:, k * W:(k + 4) * W], small[name]), (k, name)
    L.close()


def test_the_widest_beam_at_the_lds_limit():
    """N = 512 with 32 beams: 64 KB of h in LDS.  The costs are still the scorer's sums, bit for bit."""
    import lstm_hip
    import sampling_ref as sr
    N, W, count = 512, 32, 6
    prompts = _prompts([1, 1, 1], seed=41)  # (one byte: the scorer then scores the hypothesis and nothing else)
    L = _handle(N, sr.peaked_params(N, seed=43, scale=0.05, gain=4.0), flags=lstm_hip.STABLE_SOFTMAX)
    res = L.beam_search(prompts, count=count, beams=W)
    _check_shape_of_a_result(res, W, count, -1)
    texts = [bytes(prompts[s]) + t for s in range(3) for t, _ in res[s]]
    scored = L.generate(texts, count=0, score=True)[1]
    got = np.array([b for s in range(3) for _, b in res[s]])
    assert got.tobytes() == scored.tobytes()
    one = L.beam_search(prompts, count=1, beams=W)
    greedy = L.generate(prompts, count=1, temperature=0.0)[0]
    L.close()
    for s in range(3):
        assert len(set(t for t, _ in one[s])) == W and one[s][0][0] == greedy[:, s].tobytes(), s


def test_stop_byte_finishes_hypotheses_and_finished_streams_stay():
    N, W, count = 64, 4, 24
    prompts = _control_prompts()
    L = _handle(N, br.control_params())
    greedy = L.beam_search(prompts, count=count, beams=1)
    # one beam, stopped by its own first byte: every slot of the stream is finished after the first selection
    for s in range(4):
        stop = greedy[s][0][0][0]
        once = L.beam_search([prompts[s]], count=1, beams=1)
        res, raw = L.beam_search([prompts[s]], count=count, beams=1, stop_byte=stop, trace=True)
        assert res[0][0][0] == bytes([stop]) and res[0][0][1] == once[0][0][1], s
        assert raw["out_len"][0, 0] == 1 and not raw["out"][0, 0, 1:].any() and not raw["byte"][1:].any()
    # four beams and a byte from the middle of the best hypothesis
    seen = 0
    for s in range(4):
        stop = greedy[s][0][0][count // 3]
        res, raw = L.beam_search([prompts[s]], count=count, beams=W, stop_byte=stop, trace=True)
        _check_shape_of_a_result(res, W, count, stop)
        for r in range(W):
            n = raw["out_len"][0, r]
            assert not raw["out"][0, r, n:].any()
            seen += n < count
    assert seen >= 1
    L.close()


def test_bf16_padded_and_step_kernel_handles_match_their_twins():
    import lstm_hip
    W, count = 4, 20
    prompts = _prompts([0, 4, 30, 1], seed=51)

    def run(N, P, flags, B, h0, c0):
        L = _handle(N, P, flags=flags, B=B)
        out = L.beam_search(prompts, count=count, beams=W, h0=h0, c0=c0)
        L.close()
        return out
    N = 256
    P = _params(N, seed=53, scale=0.1)
    h0, c0 = _state(4, N, seed=54)
    assert run(N, P, 0, 8, h0, c0) == run(N, P, lstm_hip.BF16_RECURRENCE, 8, h0, c0)
    N = 64
    P = br.control_params()
    h0, c0 = _state(4, N, seed=55)
    assert run(N, P, 0, 1, h0, c0) == run(N, P, lstm_hip.STEP_KERNELS, 1, h0, c0)
    N = 50
    Np = padded_width(N, lstm_hip.PAD_HIDDEN)
    P = _params(N, seed=56, scale=0.3)
    h0, c0 = _state(4, N, seed=57)
    assert run(N, P, lstm_hip.PAD_HIDDEN, 1, h0, c0) == run(Np, pad_params(P, N, Np), 0, 1, pad_cols(h0, N, Np), pad_cols(c0, N, Np))


def _trainer(text, N, S, B):
    import lstm_hip
    L = lstm_hip.Lstm(N, S, B)
    L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(5), N))
    L.set_text(text)
    L.set_cursors(lstm_hip.initial_cursors(text.size, S, B))
    return L


def test_training_state_is_untouched_by_a_search():
    import lstm_hip
    N, S, B = 64, 8, 4
    text = np.random.RandomState(61).randint(97, 123, size=5000).astype(np.uint8)
    A, Bh = _trainer(text, N, S, B), _trainer(text, N, S, B)
    la = [A.train_windows(5, 0.1)]
    A.beam_search(_prompts([3, 40], seed=62), count=30, beams=5, stop_byte=101)
    la.append(A.train_windows(5, 0.1))
    lb = [Bh.train_windows(5, 0.1), Bh.train_windows(5, 0.1)]
    assert np.array_equal(np.concatenate(la), np.concatenate(lb))
    for which in (lstm_hip.P_PARAMS, lstm_hip.P_GRADS, lstm_hip.P_MEM):
        assert np.array_equal(A.get_params(which), Bh.get_params(which)), which
    assert np.array_equal(A.get_cursors(), Bh.get_cursors())
    for a, b in zip(A.get_window(), Bh.get_window()):
        assert np.array_equal(a, b)
    for t in range(S):
        for a, b in zip(A.get_state(t), Bh.get_state(t)):
            assert np.array_equal(a, b), t
    A.close()
    Bh.close()


def test_refused_arguments_leave_a_usable_handle():
    import lstm_hip
    N = 528  # 528 x 31 beams fit the 16384 floats of LDS, 528 x 32 do not
    L = _handle(N, _params(N, seed=71, scale=0.05))
    lib = L.lib
    out = np.zeros(4096 * 4, np.uint8)
    n_out = np.zeros(4096, np.int32)
    bits = np.zeros(4096, np.float64)
    p = np.frombuffer(b"abcdef", np.uint8).copy()
    up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    op, lp, bp = (out.ctypes.data_as(C.POINTER(C.c_uint8)), n_out.ctypes.data_as(C.POINTER(C.c_int32)),
                  bits.ctypes.data_as(C.POINTER(C.c_double)))
    pp = p.ctypes.data_as(C.POINTER(C.c_uint8))
    tail3 = np.array([0, 3], np.uint64)
    bad_start = np.array([1, 3], np.uint64)
    decreasing = np.array([0, 4, 2, 6], np.uint64)
    opt = lambda W, stop=-1, size=None: lstm_hip._Beam(C.sizeof(lstm_hip._Beam) if size is None else size, W, stop)
    cases = [  # (streams, prompts, off, opt, count, out, out_len, bits)
        (1, None, None, None, 4, op, lp, bp),                   # no options
        (1, None, None, opt(4, size=8), 4, op, lp, bp),         # options of the wrong size
        (1, None, None, opt(0), 4, op, lp, bp),                 # beams outside 1..32
        (1, None, None, opt(33), 4, op, lp, bp),
        (0, None, None, opt(4), 4, op, lp, bp),                 # streams < 1
        (1025, None, None, opt(4), 4, op, lp, bp),              # streams * beams > 4096
        (1, None, None, opt(32), 4, op, lp, bp),                # hidden width * beams > 16384
        (1, None, None, opt(4), -1, op, lp, bp),                # count < 0
        (1, None, None, opt(4, -2), 4, op, lp, bp),             # stop_byte outside -1..255
        (1, None, None, opt(4, 256), 4, op, lp, bp),
        (1, pp, up(bad_start), opt(4), 4, op, lp, bp),          # offsets not starting at 0
        (3, pp, up(decreasing), opt(4), 4, op, lp, bp),         # decreasing offsets
        (1, pp, None, opt(4), 4, op, lp, bp),                   # prompts without offsets
        (1, None, up(tail3), opt(4), 4, op, lp, bp),            # offsets without prompts
        (1, None, None, opt(4), 4, None, lp, bp),               # no out, out_len or bits with count > 0
        (1, None, None, opt(4), 4, op, None, bp),
        (1, None, None, opt(4), 4, op, lp, None),
    ]
    for i, (streams, prompts, off, o, count, a, b, c) in enumerate(cases):
        rc = lib.lstm_hip_beam_search(L._h, streams, prompts, off, None, None, C.byref(o) if o is not None else None, count,
                                      a, b, c, None, None)
        assert rc == lstm_hip.EINVAL, (i, rc)
        assert lib.lstm_hip_last_error().decode().startswith("beam_search:"), i
    # null results are fine with count 0, and the handle still searches and generates
    assert lib.lstm_hip_beam_search(L._h, 1, None, None, None, None, C.byref(opt(4)), 0, None, None, None, None, None) == 0
    res = L.beam_search([b"ab"], count=5, beams=31)
    _check_shape_of_a_result(res, 31, 5, -1)
    out2 = L.generate(count=10, temperature=0.0)[0]
    assert out2.shape == (10, 1)
    L.close()


def test_non_finite_parameters_still_give_bytes_inside_the_tables():
    N, W, count = 64, 8, 10
    P = br.control_params().copy()
    P[-256 + 7] = np.nan      # by[7]: every cost is NaN
    P[-256 + 9] = np.inf
    L = _handle(N, P)
    res, raw = L.beam_search(_control_prompts(), count=count, beams=W, stop_byte=10, trace=True)
    L.close()
    assert raw["parent"].max() < W and raw["out_len"].max() <= count and raw["out_len"].min() >= 0
    assert all(len(t) <= count for hyps in res for t, _ in hyps)


LSTM = os.path.join(ROOT, "eigen-lstm_amd", "lstm")
GEN = os.path.join(ROOT, "eigen-lstm_amd", "lstm_generate")


def test_program_with_one_beam_prints_the_greedy_text(tmp_path):
    rs = np.random.RandomState(81)
    corpus = tmp_path / "corpus.txt"
    rs.randint(97, 110, size=3000).astype(np.uint8).tofile(corpus)
    tr = subprocess.run([LSTM, str(corpus), "64", "8", "4", "0.1", "--epochs", "1", "--windows", "30", "--sample", "0",
                         "--save", str(tmp_path / "ck"), "--quiet"], capture_output=True, text=True, errors="replace", timeout=300)
    assert tr.returncode == 0, tr.stderr
    run = lambda *extra: subprocess.run([GEN, "--load", str(tmp_path / "ck"), "--count", "60", "--streams", "2", "--prime", "The ",
                                         *extra], capture_output=True, timeout=300)
    texts = lambda o: re.split(rb"== sample \d+[^\n]*==\n", o.stdout)[1:]
    greedy, beam = run("--temperature", "0"), run("--beams", "1")
    assert greedy.returncode == 0 and beam.returncode == 0, (greedy.stderr, beam.stderr)
    assert len(texts(beam)) == 2 and texts(beam) == texts(greedy)
    assert re.search(rb"== sample 1 hypothesis 0: [\d.]+ bits ==", beam.stdout)
    best = run("--beams", "4", "--nbest", "3", "--length-alpha", "0.7", "--stop-byte", "101")
    assert best.returncode == 0 and len(texts(best)) == 6, best.stderr
    assert run("--beams", "4", "--temperature", "0.5").returncode == 2  # a search draws nothing
