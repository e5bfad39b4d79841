"""CPU: the rule of lstm_hip_generate_guided / lstm_hip_score_guided (include/lstm_hip.h) without a
device -- the control of tests/guided_ref.py: the identities of the mix in numpy float32 on random logits, two mutants the
listed cases must catch (the bias mixed in ahead of the mix, the guides summed in reverse order), the control of the GPU oracle
comparison (how often its mixed distributions are ambiguous on the oracle's own trajectories), the program's help and usage
errors, and the header's two calls and blocks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import guided_ref as gr
import logit_processor_ref as lr
import sampling_ref as sr
import score_ref as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 256
f32 = np.float32


def _logits(seed, scale=3.0):
    return (np.random.RandomState(seed).randn(M) * scale).astype(f32)


def test_the_identities_of_the_mix():
    for seed in range(20):
        z, z1, z2 = _logits(seed), _logits(100 + seed), _logits(200 + seed, 0.5)
        # (0, 1): the guide's logits as values (0 * z is a zero of either sign: equal, not always the same bits)
        assert np.array_equal(gr.mix32(z, [z1], 0.0, [1.0]), z1)
        # (1, 0): the main model's
        assert np.array_equal(gr.mix32(z, [z1], 1.0, [0.0]), z)
        # (2, -1) and (0.5, 0.5) with the guide's logits equal to the main model's: z bit for bit (2z - z and z/2 + z/2 are exact)
        assert gr.mix32(z, [z], 2.0, [-1.0]).tobytes() == z.tobytes()
        assert gr.mix32(z, [z], 0.5, [0.5]).tobytes() == z.tobytes()
        # the general case is the float32 expression, each operation rounded
        a, b1, b2 = 1.5, -0.75, 0.25
        want = np.array([f32(f32(f32(a) * z[m]) + f32(f32(f32(b1) * z1[m]) + f32(f32(b2) * z2[m]))) for m in range(M)], f32)
        assert gr.mix32(z, [z1, z2], a, [b1, b2]).tobytes() == want.tobytes()
        # ... and the probabilities it stands for are p_main^a * prod p_k^b_k
        sm = lambda v: np.exp(v.astype(np.float64) - v.max()) / np.exp(v.astype(np.float64) - v.max()).sum()
        p = sm(gr.mix32(z, [z1, z2], a, [b1, b2]))
        assert np.abs(p - gr.mix64(sm(z), [sm(z1), sm(z2)], a, [b1, b2])).max() < 1e-5


def test_draws_and_scores_run_on_the_mixed_logits():
    V = np.ones(M, bool)
    for seed in range(6):
        z, z1 = _logits(seed), _logits(50 + seed)
        u = 0.1 + 0.13 * seed
        # (0, 1): the guide's own draw; (1, 0): the main model's
        for mode, tau in ((0, 1.0), (1, 0.7), (2, 0.0)):
            kw = dict(V=V, T=b"", mode=mode, tau=tau, top_k=40, top_p=0.9, u=u)
            assert gr.draw32(z, [z1], 0.0, [1.0], **kw) == lr.draw32(z1, V, b"", mode, tau, 40, 0.9, u)
            assert gr.draw32(z, [z1], 1.0, [0.0], **kw) == lr.draw32(z, V, b"", mode, tau, 40, 0.9, u)
        x = int(np.argmax(z1))
        got = gr.statement32(z, [z1], 0.0, [1.0], x, top_n=3)
        want = sc.statement32(z1, x, False, None, 3)
        assert all(np.array_equal(np.asarray(g), np.asarray(w)) for g, w in zip(got, want))
        # a negative weight on the guide moves mass away from the guide's favourite
        zz = gr.mix32(z, [z1], 1.5, [-0.5])
        assert zz[x] - zz.max() < z[x] - z.max() + 1e-6


def test_mixing_behind_the_bias_is_caught():
    """greedy draws: with main weight 2 a bias of +3 on one byte counts 3 mixed in ahead of the bias (the rule) and 6 behind it"""
    caught = 0
    V = np.ones(M, bool)
    for seed in range(8):
        z, z1 = _logits(seed, 1.0), _logits(300 + seed, 1.0)
        zz = gr.mix32(z, [z1], 2.0, [-1.0])
        top, second = np.argsort(zz)[::-1][:2]
        bias = np.zeros(M, f32)
        bias[second] = f32(zz[top] - zz[second]) * f32(0.75)  # not enough under the rule, enough when it is doubled
        kw = dict(V=V, T=b"", mode=2, tau=0.0, top_k=0, top_p=1.0, u=0.5, bias=bias)
        good = gr.draw32(z, [z1], 2.0, [-1.0], **kw)
        assert good[0] == top
        mutant = gr.draw32(z, [z1], 2.0, [-1.0], after_bias=True, **kw)
        caught += mutant[0] != good[0]
    assert caught == 8


def test_summing_the_guides_in_reverse_order_is_caught():
    """three guides of very different scale: (big + -big) + small keeps the small term, small + (-big + big) ... in the other
    order the small term is rounded away"""
    caught = 0
    for seed in range(8):
        rs = np.random.RandomState(400 + seed)
        big = (rs.randn(M) * 3e4).astype(f32)
        small = (rs.randn(M) * 1e-3).astype(f32)
        z = np.zeros(M, f32)
        zs, w = [big, big, small], [1.0, -1.0, 1.0]
        good = gr.mix32(z, zs, 1.0, w)
        assert np.array_equal(good, small)  # (big - big) + small
        mutant = gr.mix32(z, zs, 1.0, w, reverse=True)  # (small - big) + big
        caught += int(np.argmax(mutant)) != int(np.argmax(good)) or mutant.tobytes() != good.tobytes()
        assert mutant.tobytes() != good.tobytes()
    assert caught == 8


def _trajectories(orc):
    """the temperature-1 distributions of the main model along its own oracle32.sample trajectories (as
    tests/test_logit_processors_cpu.py) and of the guide replayed on the same bytes"""
    N = sr.ORACLE_N
    P, prompts, u = sr.oracle_case()
    Pg = gr.oracle_guide()
    main, guide = [], []
    for s in range(sr.ORACLE_STREAMS):
        xi = np.full((2, 1), -1, np.int32)
        xi[1, 0] = prompts[s][0]
        fw = orc.forward(N, M, 2, 1, P, xi, np.full((2, 1), -1, np.int32), np.zeros((1, N), np.float32),
                         np.zeros((1, N), np.float32))
        drawn, _, _ = orc.sample(N, M, P, fw["h"][1][0], fw["c"][1][0], u[:, s])
        main.append(sr.replay(orc, N, P, prompts[s], drawn))
        guide.append(sr.replay(orc, gr.ORACLE_GUIDE_N, Pg, prompts[s], drawn))
    return main, guide


def test_control_of_the_gpu_oracle_comparison(oracle32):
    """The GPU test skips ambiguous draws and asserts that they are at most 5 %: here the same parameters, weights and settings
    on the oracle's own trajectories of the main model, the guide replayed on the same bytes."""
    main, guide = _trajectories(oracle32)
    S = np.ones(M, bool)
    worst = 0.0
    for a, b in gr.ORACLE_WEIGHTS:
        for min_p, biased, top_k, top_p, tau in lr.ORACLE_SETTINGS:
            bias = lr.oracle_bias() if biased else None
            amb, keeps = [], []
            for dm, dg in zip(main, guide):
                for p1, pg in zip(dm, dg):
                    keep, _, _, p = gr.filter64(p1, [pg], a, [b], S, tau, top_k, top_p, min_p, bias)
                    amb.append(lr.ambiguous(p, S, top_k, top_p, min_p))
                    keeps.append(keep)
            print(f"weights ({a}, {b}) min_p {min_p} bias {biased} top_k {top_k} top_p {top_p} tau {tau}: "
                  f"ambiguous {np.mean(amb):.4f}, mean kept {np.mean(keeps):.2f}")
            assert np.mean(amb) <= 0.05, (a, b, min_p, biased, np.mean(amb))
            assert 1.0 < np.mean(keeps) <= 60.0, np.mean(keeps)
            worst = max(worst, float(np.mean(amb)))
    print(f"largest ambiguous share {worst:.4f}")


def test_program_help_names_the_flags_and_bad_values_are_usage_errors():
    exe = os.path.join(ROOT, "eigen-lstm_amd", "lstm_generate")
    out = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    for flag in ("--guide ", "--guide-weight", "--main-weight", "--guidance", "--negative-prime"):
        assert flag in out.stdout, flag
    g = ["--guide", "elsewhere"]
    for bad in (g + ["--guide-weight", "x"], g + ["--guide-weight", "inf"], g + ["--guide-weight", "nan"], g,  # (a guide needs a weight)
                ["--guide-weight", "0.5"], g + ["--guide-weight", "0.5", "--main-weight", "inf"], ["--main-weight", "0.5"],
                (g + ["--guide-weight", "0.2"]) * 5,
                ["--guidance", "x"], ["--guidance", "nan"], ["--negative-prime", "abc"],
                ["--guidance", "0.5"] + g + ["--guide-weight", "0.5"],
                ["--beams", "2"] + g + ["--guide-weight", "0.5"], ["--beams", "2", "--guidance", "0.5"]):
        r = subprocess.run([exe, "--load", "nowhere", "--count", "1"] + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (bad, r.returncode, r.stderr)
    # well-formed values pass the parser: the program then fails on the checkpoint, not on its usage
    for good in (g + ["--guide-weight", "-0.5", "--main-weight", "1.5"], (g + ["--guide-weight", "0.2"]) * 4,
                 ["--guidance", "0.5", "--negative-prime", "abc"], ["--guidance", "1.5"]):
        r = subprocess.run([exe, "--load", "nowhere", "--count", "1"] + good, capture_output=True, text=True, timeout=60)
        assert r.returncode != 2 and r.returncode != 0, (good, r.returncode, r.stderr)


def test_header_declares_the_two_calls_and_blocks():
    header = open(os.path.join(ROOT, "include", "lstm_hip.h")).read()
    assert re.search(r"int lstm_hip_generate_guided\(lstm_hip_t \*h, int32_t streams,", header)
    assert re.search(r"int lstm_hip_score_guided\(lstm_hip_t \*h, int32_t streams,", header)
    assert re.search(r"#define LSTM_HIP_MAX_GUIDES 4\b", header)
    m = re.search(r"typedef struct lstm_hip_guide \{(.*?)\} lstm_hip_guide;", header, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.findall(r"[\w ]+?\*?\s*\*?(\w+)\s*(?:,\s*\*(\w+))?;", body) == [("model", ""), ("weight", ""), ("h0", "c0"), ("h_out", "c_out")]
    m = re.search(r"typedef struct lstm_hip_guidance \{(.*?)\} lstm_hip_guidance;", header, re.S)
    assert m
    fields = re.findall(r"^\s*(?:const )?(\w+)\s+\*?(\w+);", m.group(1), re.M)
    assert fields == [("uint32_t", "size"), ("double", "main_weight"), ("int32_t", "nguides"), ("lstm_hip_guide", "guides")], fields
    import lstm_hip
    assert "lstm_hip_generate_guided" in lstm_hip.SYMBOLS and "lstm_hip_score_guided" in lstm_hip.SYMBOLS
    g, gd = lstm_hip._Guide, lstm_hip._Guidance
    assert C.sizeof(g) == 48 and g.weight.offset == 8 and g.h0.offset == 16 and g.c_out.offset == 40  # this ABI
    assert C.sizeof(gd) == 32 and gd.main_weight.offset == 8 and gd.nguides.offset == 16 and gd.guides.offset == 24
    # the heads take the sum and the main weight, and the guides' kernel is a file of its own that kernels.hip includes
    csrc = os.path.join(ROOT, "eigen-lstm_amd", "csrc")
    args = open(os.path.join(csrc, "heads", "head_args.h")).read()
    assert args.count("const float *gsum;") == 2 and args.count("float wmain;") == 2 and "struct GuideLogitsArgs {" in args
    assert '#include "heads/guide_logits.inc"' in open(os.path.join(csrc, "kernels.hip")).read()
    api = open(os.path.join(csrc, "lstm_hip_api.cpp")).read()
    assert re.search(r'kKernelNamesLast\[K_COUNT - K_COUNT_MORE\] = \{"guide_logits"\};', api)
