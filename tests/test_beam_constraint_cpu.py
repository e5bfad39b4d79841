"""CPU: the references of tests/beam_constraint_ref.py -- what the rule of lstm_hip_beam_search_constrained (include/lstm_hip.h;
DESIGN.md section 3.12) implies -- and the control of the oracle comparison in tests/test_beam_constraint.py: on its cases the
float64 reference keeps a margin between the last selected and the first rejected existing candidate that float32 cannot
cross.  Also the boundary: the call is declared, exported and listed, and refuses a null handle; the program takes the constraint
options with --beams --constrain-search."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import beam_constraint_ref as bcr
import beam_ref as br
import constraint_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
FORBID = bcr.FORBID


def _tied_model(seed, levels=9):
    """test_beam_search_cpu's toy model: a row of logits per (position, last byte), few levels, so that many logits tie"""
    T = (np.random.RandomState(seed).randint(0, levels, size=(64, 257, 256)) / 4).astype(f32)

    def logits(prefixes):
        return np.stack([T[len(p), p[-1] if p else 256] for p in prefixes])
    return logits, T


def _small_table(rs, Q, alphabet, density=0.6):
    """a random table over a few bytes in which no state is empty"""
    t = np.full((Q, 256), FORBID, np.uint16)
    for q in range(Q):
        for b in alphabet:
            if rs.random_sample() < density:
                t[q, b] = rs.randint(0, Q)
        if (t[q] == FORBID).all():
            t[q, alphabet[0]] = rs.randint(0, Q)
    return t


def test_the_call_is_declared_exported_and_listed():
    import lstm_hip
    lib = lstm_hip.load_library()
    name = "lstm_hip_beam_search_constrained"
    assert hasattr(lib, name) and name in lstm_hip.SYMBOLS
    header = open(os.path.join(ROOT, "include", "lstm_hip.h")).read()
    assert re.search(r"int lstm_hip_beam_search_constrained\(lstm_hip_t \*h, int32_t streams,", header)
    m = re.search(r"typedef struct lstm_hip_beam_constraint \{(.*?)\} lstm_hip_beam_constraint;", header, re.S)
    assert m
    fields = re.findall(r"^\s*(?:const\s+)?(\w+)\s+\*?(\w+);", m.group(1), re.M)
    assert fields == [("uint32_t", "size"), ("lstm_hip_constraint", "con"), ("uint8_t", "accept")], fields
    decl = header[header.index("int lstm_hip_beam_search_constrained("):]
    decl = decl[:decl.index(";")]
    assert re.search(r"const lstm_hip_beam_constraint \*bc.*const int32_t \*start_state.*int32_t \*end_state", decl, re.S)
    assert C.sizeof(lstm_hip._BeamConstraint) == 24 and lstm_hip._BeamConstraint.con.offset == 8
    assert "The coders and lstm_hip_sample take no constraint" in header
    assert lstm_hip.coder_version() == 1  # the search moves nothing the coder depends on


def test_the_call_refuses_a_null_handle_with_a_message():
    import lstm_hip
    lib = lstm_hip.load_library()
    opt = lstm_hip._Beam(C.sizeof(lstm_hip._Beam), 4, -1)
    out, n, bits = (C.c_uint8 * 16)(), (C.c_int32 * 4)(), (C.c_double * 4)()
    rc = lib.lstm_hip_beam_search_constrained(None, 1, None, None, None, None, C.byref(opt), 4, out, n, bits, None, None, None,
                                              None, None)
    assert rc != 0 and lib.lstm_hip_last_error()


def test_program_takes_the_constraint_options_with_beams_and_constrain_search():
    GEN = os.path.join(ROOT, "eigen-lstm_amd", "lstm_generate")
    out = subprocess.run([GEN, "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "--constrain-search" in out.stdout
    base = [GEN, "--load", "nowhere", "--count", "5", "--beams", "4"]
    for good in (["--utf8"], ["--allow", "0x20-0x7e,10"], ["--ban", "0"], ["--utf8", "--ban", "0xc3", "--nbest", "2"]):
        r = subprocess.run(base + good + ["--constrain-search"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1, (good, r.returncode, r.stderr)  # past the options: the checkpoint is what fails
        r = subprocess.run(base + good, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--constrain-search" in r.stderr, (good, r.returncode, r.stderr)
    for bad in (["--constrain-search"], ["--constrain-search", "--utf8", "--temperature", "0.5"],
                ["--constrain-search", "--allow", "65", "--ban", "65"]):
        r = subprocess.run(base + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (bad, r.returncode, r.stderr)
    r = subprocess.run([GEN, "--load", "nowhere", "--count", "5", "--utf8", "--constrain-search"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2, r.stderr  # (an option of --beams)


@pytest.mark.parametrize("W", [1, 4, 32])
def test_one_state_that_allows_everything_is_the_unconstrained_search(W):
    logits, _ = _tied_model(10 + W)
    free = br.beam32(logits, W, 12)
    for stop in (-1, free["hyps"][0][4]):
        want = br.beam32(logits, W, 12, stop)
        got = bcr.beam32(logits, W, 12, bcr.trivial_table(), 0, stop)
        for name in ("hyps", "bits", "length", "fin", "parent", "byte", "x_next"):
            assert got[name] == want[name], (stop, name)
        assert got["margin"] == want["margin"] and got["state"] == [0] * W


def test_f_is_reachability_by_brute_force():
    rs = np.random.RandomState(5)
    alphabet, seen = [3, 4, 5], [0, 0]
    for trial in range(40):
        Q = rs.randint(1, 6)
        table = _small_table(rs, Q, alphabet, density=0.45)
        accept = (rs.random_sample(Q) < 0.35).astype(np.uint8)
        stop = [-1, 3, 4][trial % 3]
        F = bcr.f_table(table, accept, stop, 5)
        for R in range(6):
            for q in range(Q):
                want = len(bcr.strings(table, q, R, stop, accept)) > 0 if R else bool(accept[q])
                assert bool(F[R][q]) == want, (trial, R, q)
                seen[want] += 1
    assert min(seen) > 100, seen  # both answers occur often


def test_a_live_slot_always_has_a_candidate_and_finite_hypotheses_are_accepted():
    """the reference asserts inside every selection that every live slot offers a candidate and that W are found"""
    rs = np.random.RandomState(6)
    alphabet = [10, 97, 98, 99, 200, 201]
    searched = absent = stopped = 0
    for trial in range(60):
        Q, W, count = rs.randint(1, 7), [1, 3, 8][trial % 3], rs.randint(1, 7)
        table = _small_table(rs, Q, alphabet)
        accept = (rs.random_sample(Q) < 0.4).astype(np.uint8)
        stop = 10 if trial % 2 else -1
        q0 = rs.randint(0, Q)
        if not bcr.f_table(table, accept, stop, count)[count][q0]:
            continue  # (the call refuses these)
        logits, _ = _tied_model(100 + trial)
        res = bcr.beam32(logits, W, count, table, q0, stop, accept)
        searched += 1
        for hyp, bits, n, fin, q in zip(res["hyps"], res["bits"], res["length"], res["fin"], res["state"]):
            if bits == br.INF:
                assert n == 0 and hyp == b"" and q == q0 and fin
                absent += 1
                continue
            assert accept[q] and cr.walk(table, q0, hyp) == q and len(hyp) == n
            sb = bytes([stop]) if stop >= 0 else b"none"
            assert (hyp.endswith(sb) and sb not in hyp[:-1]) if fin else (n == count and sb not in hyp)
            stopped += fin
        assert res["bits"] == sorted(res["bits"])
    assert searched >= 20 and absent >= 1 and stopped >= 1, (searched, absent, stopped)


def test_a_search_wider_than_the_language_is_the_brute_force_list():
    """when the table accepts at most W strings no prefix that can be completed is ever dropped: the finite hypotheses are
    all accepted strings, in the order of their costs"""
    table, accept = bcr.pattern_ab_newline()
    logits, T = _tied_model(7, levels=200)  # (few ties: the brute-force order is then the search's)
    one = lambda pre: T[len(pre), pre[-1] if pre else 256]
    res = bcr.beam32(logits, 16, 5, table, 0, 10, accept)
    want = sorted((bcr.cost32(one, table, 0, s), s) for s, _ in bcr.strings(table, 0, 5, 10, accept))
    assert len(want) == 14 and all(2 <= len(s) <= 4 and s.endswith(b"\n") for _, s in want)
    assert res["hyps"][:14] == [s for _, s in want] and res["bits"][:14] == [c for c, _ in want]
    assert res["bits"][14:] == [br.INF] * 2 and res["length"][14:] == [0, 0] and res["state"][14:] == [0, 0]
    chain = bcr.chain_table([(97, 98), (99, 100), (101, 102), (103, 104)])
    res = bcr.beam32(logits, 32, 4, chain)
    want = sorted((bcr.cost32(one, chain, 0, s), s) for s, _ in bcr.strings(chain, 0, 4))
    assert len(want) == 16 and res["hyps"][:16] == [s for _, s in want] and res["bits"][16:] == [br.INF] * 16
    assert res["state"] == [4] * 16 + [0] * 16


def _control_cases(orc):
    """(prompt byte, W, table name, (table, accept, stop), the constrained beam64's result) of the oracle comparison"""
    import lstm_hip
    utf8 = lstm_hip.dfa_utf8()
    N, count, P = br.CONTROL_N, br.CONTROL_COUNT, bcr.control_params()
    for b in br.CONTROL_PROMPTS:
        for W in br.CONTROL_BEAMS:
            for name in bcr.ORACLE_TABLES:
                table, accept, stop = bcr.oracle_table(name, utf8)
                yield b, W, name, (table, accept, stop), bcr.beam64(orc, N, P, [b], W, count, table, 0, stop, accept)


def test_control_of_the_oracle_comparison(oracle64, oracle32):
    """The float64 reference separates the W-th from the (W+1)-th existing candidate by at least 5e-5 bits at EVERY selection
    of every case (the threshold tests/test_beam_search_cpu.py uses; measured: 1.5e-4), and the float32 restatement -- the
    oracle's float32 recurrence with the device's selection arithmetic on the masked logits -- finds the same hypotheses,
    lengths and end states with costs within 1e-4 bits, so the GPU test skips nothing.  And the case shows what a constraint
    is for: the unconstrained search returns text that is not well-formed UTF-8, and the UTF-8 search without accepting
    states ends hypotheses inside a character."""
    import lstm_hip
    utf8 = lstm_hip.dfa_utf8()
    N, count, P = br.CONTROL_N, br.CONTROL_COUNT, bcr.control_params()
    smallest, worst, cases, inside, stopped = br.INF, 0.0, 0, 0, 0
    for b, W, name, (table, accept, stop), ref in _control_cases(oracle64):
        assert len(ref["margins"]) == count and min(ref["margins"]) >= 5e-5, (b, W, name, min(ref["margins"]))
        smallest = min(smallest, ref["margin"])
        low = bcr.beam32_oracle(oracle32, N, P, [b], W, count, table, 0, stop, accept)
        assert low["hyps"] == ref["hyps"] and low["length"] == ref["length"] and low["state"] == ref["state"], (b, W, name)
        worst = max(worst, np.abs(np.array(low["bits"]) - np.array(ref["bits"])).max())
        assert all(np.isfinite(ref["bits"]))
        if name == "utf8":
            inside += sum(q != 0 for q in ref["state"])
        if name == "utf8_accept":
            assert ref["state"] == [0] * W and all(bcr.well_formed_utf8(t, utf8) for t in ref["hyps"])
        if name == "ascii_stop":
            assert all(all(c == 10 or 0x20 <= c <= 0x7e for c in t) for t in ref["hyps"])
            stopped += sum(ref["fin"])
        cases += 1
    broken = sum(not bcr.well_formed_utf8(t, utf8) for b in br.CONTROL_PROMPTS for W in br.CONTROL_BEAMS
                 for t in br.beam64(oracle64, N, P, [b], W, count)["hyps"])
    print("smallest margin %.3g bits, largest float32 - float64 cost difference %.3g bits; %d unconstrained hypotheses are not "
          "UTF-8, %d UTF-8 hypotheses end inside a character, %d stopped" % (smallest, worst, broken, inside, stopped))
    assert cases == 36 and broken >= 1 and inside >= 1
    assert worst <= 1e-4, worst
