"""CPU: what lstm_hip_generate_accepting needs besides a device (include/lstm_hip.h): the header, the
Python names, the program's options, and the control of the GPU oracle comparison."""
import os
import re
import subprocess

import numpy as np
import pytest

import constraint_ref as cr
import deadline_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "eigen-lstm_amd", "lstm_generate")
M = 256


def test_header_and_python_names():
    import inspect
    import lstm_hip
    header = open(os.path.join(ROOT, "include", "lstm_hip.h")).read()
    assert re.search(r"int32_t lstm_hip_dfa_regex\(const uint8_t \*pattern, size_t len, int32_t stop_byte[^,]*, uint16_t \*next, "
                     r"uint8_t \*accept,\s*int32_t cap, int32_t \*error_pos[^)]*\);", header)
    assert re.search(r"int32_t lstm_hip_dfa_intersect\(const uint16_t \*a, int32_t qa, const uint8_t \*acc_a[^,]*, const uint16_t \*b, "
                     r"int32_t qb,\s*const uint8_t \*acc_b[^,]*, uint16_t \*next, uint8_t \*accept, int32_t cap\);", header)
    decl = header[header.index("int lstm_hip_generate_accepting("):]
    decl = decl[:decl.index(";")]
    old = header[header.index("int lstm_hip_generate_constrained("):]
    old = old[:old.index(";")]
    strip = lambda d: re.sub(r"/\*.*?\*/", "", re.sub(r"\s+", " ", d))
    # the arguments of lstm_hip_generate_constrained, with the beam constraint in place of the table
    want = strip(old).replace("lstm_hip_generate_constrained", "lstm_hip_generate_accepting").replace(
        "const lstm_hip_constraint *con", "const lstm_hip_beam_constraint *bc")
    assert re.sub(r"\s+", " ", strip(decl)).replace(" ,", ",") == re.sub(r"\s+", " ", want).replace(" ,", ","), (strip(decl), want)
    for word in ("NOT the one long call", "lowest EXISTING byte", "acc(end_state[s]) holds for every stream", "A QUANTIFIER BINDS THE LAST BYTE"):
        assert word in header, word
    for name in ("lstm_hip_dfa_regex", "lstm_hip_dfa_intersect", "lstm_hip_generate_accepting"):
        assert name in lstm_hip.SYMBOLS and hasattr(lstm_hip.load_library(), name), name
    assert "accept" in inspect.signature(lstm_hip.Lstm.generate).parameters
    assert list(inspect.signature(lstm_hip.dfa_regex).parameters) == ["pattern", "stop_byte"]
    assert list(inspect.signature(lstm_hip.dfa_intersect).parameters) == ["a", "acc_a", "b", "acc_b"]
    t, a = lstm_hip.dfa_regex("é+")  # a str is its UTF-8 bytes: the quantifier binds the last byte
    assert t.shape == (3, 256) and t[0, 0xC3] == 1 and t[1, 0xA9] == 2 and t[2, 0xA9] == 2 and list(a) == [0, 0, 1]


def test_program_options():
    out = subprocess.run([GEN, "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert "--regex PATTERN" in out.stdout and "exactly --count" in out.stdout and "last byte" in out.stdout
    base = [GEN, "--load", "nowhere", "--count", "8"]
    run = lambda *a: subprocess.run(base + list(a), capture_output=True, text=True, timeout=60)
    assert run("--regex").returncode == 2  # a missing value
    r = run("--regex", "ab", "--beams", "2")  # the old refusal stands without --constrain-search
    assert r.returncode == 2 and "--regex is an option of drawing: with --beams it needs --constrain-search" in r.stderr
    assert run("--regex", "ab", "--score", "some.txt").returncode == 2
    # a pattern error: the library's message with the position, status 1, before any checkpoint is looked for
    r = run("--regex", "ab**")
    assert r.returncode == 1 and "dfa_regex: a quantifier at byte 3 follows a quantifier" in r.stderr, r.stderr
    r = run("--regex", "[0-9", "--stop-byte", "10")
    assert r.returncode == 1 and "the class opened at byte 0 is not closed" in r.stderr, r.stderr
    r = run("--regex", "a\\s", "--stop-byte", "10")
    assert r.returncode == 1 and "the pattern can match the stop byte 0x0a" in r.stderr, r.stderr
    r = run("--regex", "[\\x80-\\xbf]+", "--utf8")  # continuation bytes alone are never well formed
    assert r.returncode == 1 and "--regex with --utf8" in r.stderr and "empty language" in r.stderr, r.stderr
    r = run("--regex", "[a-c]+", "--ban", "0x61-0x63")
    assert r.returncode == 2 and "leave nothing to draw" in r.stderr, r.stderr
    # good patterns get past the options: the checkpoint is what fails (status 1, its message)
    for good in (["--regex", "[0-9]{3}-[0-9]{4}", "--stop-byte", "10"], ["--regex", "(?:é|[a-z])+", "--utf8"],
                 ["--regex", "[a-z]+", "--beams", "2", "--constrain-search"], ["--regex", "[a-z ]+", "--ban", "32"]):
        r = run(*good)
        assert r.returncode == 1 and "nowhere" in r.stderr, (good, r.returncode, r.stderr)


@pytest.mark.parametrize("name", dr.ORACLE_TABLES)
def test_control_of_the_gpu_oracle_comparison(oracle32, name):
    """The GPU test (tests/test_generate_accepting.py) skips draws whose masked distribution is ambiguous and asserts that
    they are at most 5 %: here the same parameters, prompts, draws, tables and settings on the float32 oracle alone, the
    reference rule of tests/deadline_ref.py choosing the bytes.  Every state draws, draws with R <= 3 occur, every stream
    ends in an accepting state, and under the UTF-8 table the deadline cuts something the table alone allows."""
    import lstm_hip
    utf8 = lstm_hip.dfa_utf8()
    P, prompts, u, table, accept, stop = dr.oracle_case(name, utf8)
    N, Cn = 64, dr.ORACLE_COUNT
    F = dr.f_table(table, accept, stop, Cn)
    for top_k, top_p, tau in cr.ORACLE_SETTINGS:
        amb, drawing, late, cut = [], set(), 0, 0
        for s in range(len(prompts)):
            xi = np.full((2, 1), -1, np.int32)
            xi[1, 0] = prompts[s][0]
            ti = np.full((2, 1), -1, np.int32)
            fw = oracle32.forward(N, M, 2, 1, P, xi, ti, np.zeros((1, N), np.float32), np.zeros((1, N), np.float32))
            h, c, q = fw["h"][1], fw["c"][1], cr.walk(table, 0, prompts[s])
            assert F[Cn][q]
            p1 = np.asarray(fw["probs"][1, 0], np.float64)
            for i in range(Cn):
                R = Cn - i
                drawing.add(q)
                late += R <= 3
                cut += dr.exists(table, accept, F, stop, q, R).sum() < cr.counts(table)[q]
                keep, mask, pp, p = dr.filter64(p1, table, accept, F, stop, q, R, tau, top_k, top_p)
                amb.append(dr.ambiguous(p, table, accept, F, stop, q, R, top_k, top_p))
                cdf = np.cumsum(pp)
                x = int(min(np.searchsorted(cdf, u[i, s], side="right"), np.nonzero(mask)[0].max()))
                assert mask[x] and dr.exists(table, accept, F, stop, q, R)[x]
                q = int(table[q, x])
                if x == stop:
                    break
                xi[1, 0] = x  # one more step from (h, c) with input x
                fw = oracle32.forward(N, M, 2, 1, P, xi, ti, np.asarray(h, np.float32).reshape(1, N), np.asarray(c, np.float32).reshape(1, N))
                h, c = fw["h"][1], fw["c"][1]
                p1 = np.asarray(fw["probs"][1, 0], np.float64)
            assert accept[q], (s, q)
        print(f"{name} top_k {top_k} top_p {top_p} tau {tau}: ambiguous {np.mean(amb):.4f} of {len(amb)} draws, drawing states "
              f"{sorted(drawing)}, draws with R <= 3: {late}, draws the deadline cuts: {cut}")
        assert np.mean(amb) <= 0.05, (top_k, top_p, tau, np.mean(amb))
        assert drawing == set(range(table.shape[0])) and late >= 1
        if name == "utf8_accept":
            assert cut >= 1
