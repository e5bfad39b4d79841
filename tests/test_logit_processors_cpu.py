"""CPU: the logit processors of lstm_hip_generate_processed (include/lstm_hip.h) without a device -- the
control of tests/logit_processor_ref.py: the n-gram ban against a brute-force set of n-grams, the float32 min-p keep against
its float64 definition, the drop rule on a one-byte state, a mutant the listed cases must catch, and the control of the GPU
oracle comparison (how often its distributions are ambiguous; that greedy decoding of its parameters cycles)."""
import ctypes as C
import os
import re

import numpy as np

import constraint_ref as cr
import logit_processor_ref as lr
import sampling_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 256
f32 = np.float32


def _brute(T, n):
    """the bytes m for which T ++ [m] would end in an n-gram that T already holds"""
    T = bytes(T)
    if n < 1 or len(T) < n - 1:
        return set()
    grams = {T[j:j + n] for j in range(len(T) - n + 1)}
    suf = T[len(T) - (n - 1):] if n > 1 else b""
    return {m for m in range(M) if suf + bytes([m]) in grams}


def _texts():
    rs = np.random.RandomState(1)
    out = [b"", b"a", b"ab", b"aaaaaaaaaaaa", b"abababababab", b"abcabcabcabcab", b"the the the th", bytes(range(256)) * 2]
    for size, hi in ((5, 3), (40, 2), (40, 4), (200, 3), (200, 256), (700, 5)):
        out.append(bytes(rs.randint(0, hi, size=size).astype(np.uint8)))
    for period in (1, 2, 3, 7, 9):
        unit = bytes(rs.randint(0, 256, size=period).astype(np.uint8))
        out.append((unit * 30)[:50 + period])
    return out


def test_ngram_banned_is_the_brute_force_rule():
    bites = 0
    for T in _texts():
        for n in (1, 2, 3, 8):
            B = lr.ngram_banned(T, n)
            assert set(np.nonzero(B)[0]) == _brute(T, n), (T, n)
            bites += int(B.any())
            if n == 1:
                assert set(np.nonzero(B)[0]) == set(T)
            if len(T) < n - 1:
                assert not B.any()
            # a text extended by a byte that is not banned repeats no n-gram that it did not repeat before
            if not lr.repeats_ngram(T, n):
                for m in range(0, M, 37):
                    assert lr.repeats_ngram(T + bytes([m]), n) == bool(B[m]), (T, n, m)
    assert bites >= 30
    assert not lr.ngram_banned(b"abcdef", 8).any() and not lr.ngram_banned(b"", 2).any()  # len < n - 1
    assert not lr.ngram_banned(b"abab", 0).any()
    assert list(np.nonzero(lr.ngram_banned(b"abcab", 3))[0]) == [ord("c")]
    assert list(np.nonzero(lr.ngram_banned(np.frombuffer(b"xyx", np.uint8), 2))[0]) == [ord("y")]


def test_min_p_keep_in_float32_is_the_float64_definition():
    rs = np.random.RandomState(2)
    checked = cut = 0
    for trial in range(300):
        z = rs.randn(M) * rs.choice([1.0, 3.0, 8.0])  # peaked to very peaked
        p = np.exp(z - z.max())
        p /= p.sum()
        ps = np.sort(p)[::-1]
        for min_p in (0.01, 0.05, 0.3, 0.9, 1.0):
            thr = min_p * ps[0]
            if (np.abs(ps[1:] - thr) < 1e-6 * thr).any():  # (the largest term is kept whatever the threshold)
                continue  # within 1e-6 relative of the threshold: float32 may rightly differ
            want = lr.min_p_keep64(ps, min_p)
            got = lr.min_p_keep32(ps.astype(f32), min_p)
            assert got == want and want >= 1, (trial, min_p, got, want)
            assert want == (int((ps >= thr).sum()) if (ps < thr).any() else M)
            checked += 1
            cut += want < M
    assert checked >= 1400 and cut >= 1000
    assert lr.min_p_keep32(np.full(M, 1 / M, f32), 1.0) == M and lr.min_p_keep32(np.full(M, 1 / M, f32), 0.0) == M


def test_min_p_caps_keep_with_the_other_filters():
    rs = np.random.RandomState(3)
    z = (rs.randn(M) * 3).astype(f32)
    V = np.ones(M, bool)
    base = lr.draw32(z, V, b"", 1, 0.8, 0, 1.0, 0.5)
    assert base[1] == M
    k_m = lr.draw32(z, V, b"", 1, 0.8, 0, 1.0, 0.5, min_p=0.1)[1]
    k_k = lr.draw32(z, V, b"", 1, 0.8, 5, 1.0, 0.5)[1]
    k_p = lr.draw32(z, V, b"", 1, 0.8, 0, 0.9, 0.5)[1]
    assert 1 <= k_m < M and k_k == 5 and 1 <= k_p < M
    assert lr.draw32(z, V, b"", 1, 0.8, 5, 0.9, 0.5, min_p=0.1)[1] == min(k_m, k_k, k_p)
    # the float64 rule agrees on this distribution, and past every edge the byte is the largest kept index
    p1 = np.exp(z.astype(np.float64) - z.max())
    p1 /= p1.sum()
    keep, mask, q, _ = lr.filter64(p1, V, 0.8, 0, 1.0, min_p=0.1)
    assert keep == k_m and mask.sum() == keep and abs(q.sum() - 1) < 1e-12
    x = lr.draw32(z, V, b"", 1, 0.8, 0, 1.0, 2.0, min_p=0.1)[0]
    assert x == int(np.nonzero(mask)[0].max())
    assert lr.draw32(z, V, b"", 2, 0.0, 0, 1.0, 0.5, min_p=0.9)[:2] == (int(np.argmax(z)), 1)  # greedy ignores min-p
    # a bias moves the argmax
    bias = np.zeros(M, f32)
    bias[7] = 100.0
    assert lr.draw32(z, V, b"", 2, 0.0, 0, 1.0, 0.5, bias=bias)[0] == 7


def test_the_ban_is_dropped_where_it_leaves_no_byte():
    table = np.full((2, 256), cr.FORBID, np.uint16)
    table[0, 65] = 1  # state 0 allows 'A' alone
    table[1, 65:91] = 0
    z = np.zeros(M, f32)
    z[66] = 5.0
    V0, V1 = lr.valid(table, 0), lr.valid(table, 1)
    for mode, tau in ((2, 0.0), (1, 0.7), (0, 1.0)):
        x, kept, bit, dropped = lr.draw32(z, V0, b"AA", mode, tau, 0, 1.0, 0.3, n=1)
        assert (x, kept, bit, dropped) == (65, 1, True, True)  # 'A' is banned and it is all the state has: the table wins
        x, kept, bit, dropped = lr.draw32(z, V1, b"AB", mode, tau, 0, 1.0, 0.3, n=1)
        assert not dropped and bit and x not in (65, 66) and 65 <= x <= 90 and kept == (1 if mode == 2 else 24)
    S, B, dropped = lr.survivors(V0, b"xyz", 1)
    assert not dropped and not (B & V0).any() and np.array_equal(S, V0)


def _mutant_cases():
    """(z, T, prompt length, n): greedy draws on which the ban depends on the prompt"""
    rs = np.random.RandomState(4)
    cases = []
    for n in (1, 2, 3):
        z = (rs.randn(M)).astype(f32)
        top = int(np.argmax(z))
        prompt =bytes([9, 8][:n - 1]) + bytes([top]) + b"q" * 3 + bytes([9, 8][:n - 1])  # ... suf top ... suf
        cases.append((z, prompt, len(prompt), n))
    return cases


def test_a_ban_that_forgets_the_prompt_is_caught():
    caught = 0
    V = np.ones(M, bool)
    for z, T, L, n in _mutant_cases():
        good = lr.draw32(z, V, T, 2, 0.0, 0, 1.0, 0.5, n=n)
        assert good[2] and good[0] != int(np.argmax(z))  # the ban bites: the prompt holds the n-gram
        mutant = lr.draw32(z, V, T, 2, 0.0, 0, 1.0, 0.5, n=n, forget_prompt=L)
        caught += mutant[0] != good[0]
    assert caught == 3


def _trajectories(orc):
    """as tests/test_sampling_controls_cpu.py: the temperature-1 distributions along oracle32.sample trajectories"""
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
    return dists


def test_control_of_the_gpu_oracle_comparison(oracle32):
    """The GPU test skips ambiguous draws and asserts that they are at most 5 %: here the same parameters and settings on the
    oracle's own trajectories.  And min-p must cut something on them."""
    dists = _trajectories(oracle32)
    S = np.ones(M, bool)
    for min_p, biased, top_k, top_p, tau in lr.ORACLE_SETTINGS:
        bias = lr.oracle_bias() if biased else None
        amb, keeps = [], []
        for d in dists:
            for p1 in d:
                keep, _, _, p = lr.filter64(p1, S, tau, top_k, top_p, min_p, bias)
                amb.append(lr.ambiguous(p, S, top_k, top_p, min_p))
                keeps.append(keep)
        print(f"min_p {min_p} bias {biased} top_k {top_k} top_p {top_p} tau {tau}: ambiguous {np.mean(amb):.4f}, "
              f"mean kept {np.mean(keeps):.2f}")
        assert np.mean(amb) <= 0.05, (min_p, biased, np.mean(amb))
        assert 1.0 < np.mean(keeps) <= 60.0, np.mean(keeps)
    bias = lr.oracle_bias()
    assert (bias == 2).sum() == 8 and (bias == -2).sum() == 8 and (bias != 0).sum() == 16


def test_greedy_decoding_of_the_peaked_parameters_cycles(oracle32):
    """what tests/test_logit_processors.py relies on: the oracle's greedy run repeats a 4-gram within 60 bytes, on every stream"""
    N = sr.ORACLE_N
    P, prompts, _ = sr.oracle_case()
    for s in range(sr.ORACLE_STREAMS):
        drawn = []
        for i in range(60):
            p = sr.replay(oracle32, N, P, prompts[s], np.array(drawn + [0], np.uint8))[-1]
            drawn.append(int(np.argmax(p)))
        assert lr.repeats_ngram(bytes(prompts[s]) + bytes(drawn), 4), (s, drawn)


def test_program_help_names_the_three_flags_and_bad_values_are_usage_errors():
    import subprocess
    exe = os.path.join(ROOT, "eigen-lstm_amd", "lstm_generate")
    out = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    for flag in ("--logit-bias", "--min-p", "--no-repeat-ngram"):
        assert flag in out.stdout, flag
    for bad in (["--logit-bias", "65"], ["--logit-bias", "65:x"], ["--logit-bias", "65:inf"], ["--logit-bias", "300:1"],
                ["--logit-bias", "0x41-0x5a:-2.5,"], ["--min-p", "1.5"], ["--min-p", "-0.1"], ["--min-p", "x"],
                ["--no-repeat-ngram", "65"], ["--no-repeat-ngram", "-1"],
                ["--beams", "2", "--min-p", "0.1"], ["--beams", "2", "--no-repeat-ngram", "3"],
                ["--beams", "2", "--logit-bias", "0x41-0x5a:-2.5,10:+1"]):
        r = subprocess.run([exe, "--load", "nowhere", "--count", "1"] + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (bad, r.returncode, r.stderr)
    # a well-formed value passes the parser: the program then fails on the checkpoint, not on its usage
    r = subprocess.run([exe, "--load", "nowhere", "--count", "1", "--logit-bias", "0x41-0x5a:-2.5,10:+1", "--min-p", "0.05",
                        "--no-repeat-ngram", "4"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 2 and r.returncode != 0, (r.returncode, r.stderr)


def test_header_declares_the_call_and_its_block():
    header = open(os.path.join(ROOT, "include", "lstm_hip.h")).read()
    assert re.search(r"int lstm_hip_generate_processed\(lstm_hip_t \*h, int32_t streams,", header)
    m = re.search(r"typedef struct lstm_hip_logit_processors \{(.*?)\} lstm_hip_logit_processors;", header, re.S)
    assert m
    fields = re.findall(r"^\s*(?:const )?(\w+)\s+\*?(\w+);", m.group(1), re.M)
    assert fields == [("uint32_t", "size"), ("float", "bias"), ("double", "min_p"), ("int32_t", "no_repeat"),
                      ("uint8_t", "history"), ("uint64_t", "history_off")], fields
    import lstm_hip
    assert "lstm_hip_generate_processed" in lstm_hip.SYMBOLS
    lp = lstm_hip._LogitProcessors
    assert C.sizeof(lp) == 48 and lp.bias.offset == 8 and lp.min_p.offset == 16 and lp.no_repeat.offset == 24  # this ABI
    assert lp.history.offset == 32 and lp.history_off.offset == 40
