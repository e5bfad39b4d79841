"""CPU: constrained generation (lstm_hip_generate_constrained, include/lstm_hip.h) without a device
-- the UTF-8 automaton of lstm_hip_dfa_utf8 against Python's strict decoder, lstm_hip_dfa_restrict, the header, the Python
names, the program's options, and the control of the GPU oracle comparison (how often its distributions are ambiguous, and
whether every state of the automaton draws)."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import constraint_ref as cr
import sampling_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "eigen-lstm_amd", "lstm_generate")
M = 256


def _decodes(data):
    try:
        bytes(data).decode("utf-8", "strict")
        return True
    except UnicodeDecodeError:
        return False


def _accepts(table, strings):
    """per row of `strings` ([n, len] uint8): does the walk from state 0 end in state 0?  (vectorised over the rows)"""
    strings = np.asarray(strings, np.uint8)
    ext = np.vstack([table, np.full((1, 256), len(table), np.uint16)])  # a dead state for rejected walks
    ext[ext == cr.FORBID] = len(table)
    q = np.zeros(len(strings), np.int64)
    for j in range(strings.shape[1]):
        q = ext[q, strings[:, j]].astype(np.int64)
    return q == 0


def test_utf8_table_accepts_what_the_strict_decoder_accepts():
    import lstm_hip
    lib = lstm_hip.load_library()
    assert lib.lstm_hip_dfa_utf8(None) == 8
    table = lstm_hip.dfa_utf8()
    assert table.shape == (8, 256) and table.dtype == np.uint16
    assert list(cr.counts(table)) == [179, 64, 64, 32, 32, 64, 48, 16]
    assert ((table < 8) | (table == cr.FORBID)).all()
    groups = [
        [range(256)],                                                                  # all 1-byte strings
        [range(256), range(256)],                                                      # all 2-byte strings
        [(0xE0, 0xE1, 0xEC, 0xED, 0xEE, 0xEF), range(0x70, 0xD0), range(0x70, 0xD0)],  # the 3-byte edge ranges
        [(0xF0, 0xF1, 0xF3, 0xF4, 0xF5), range(0x78, 0xC8), (0x7F, 0x80, 0xBF, 0xC0), (0x7F, 0x80, 0xBF, 0xC0)],
    ]
    checked = 0
    for g in groups:
        strings = np.array(list(itertools.product(*g)), np.uint8)
        want = np.array([_decodes(row) for row in strings])
        got = _accepts(table, strings)
        assert np.array_equal(got, want), strings[np.nonzero(got != want)[0][:5]]
        assert want.any() and not want.all()
        checked += len(strings)
    points = sorted(set(range(0, 0xD800, 7)) | set(range(0xE000, 0x110000, 101)) |
                    {0, 0x7F, 0x80, 0x7FF, 0x800, 0xFFF, 0x1000, 0xCFFF, 0xD000, 0xD7FF, 0xE000, 0xFFFF, 0x10000, 0x3FFFF,
                     0x40000, 0xFFFFF, 0x100000, 0x10FFFF})
    for cp in points:  # every encoding is accepted, and every proper prefix of it ends off the boundary
        enc = chr(cp).encode("utf-8")
        assert cr.walk(table, 0, enc) == 0, hex(cp)
        for n in range(1, len(enc)):
            assert cr.walk(table, 0, enc[:n]) not in (0, None), hex(cp)
    checked += len(points)
    assert checked >= 145000
    # only state 0 is a character boundary: whatever any other state accepts next, the text so far does not decode
    for lead, q in zip(cr.UTF8_STATE_PROMPTS, range(8)):
        assert cr.walk(table, 0, bytes([lead])) == q


def test_dfa_restrict():
    import lstm_hip
    utf8 = lstm_hip.dfa_utf8()
    ascii_only = np.zeros(256, np.uint8)
    ascii_only[:128] = 1
    t = lstm_hip.dfa_restrict(utf8, ascii_only)
    assert t.shape == utf8.shape and cr.counts(t)[0] == 128 and (t[0, :128] == 0).all()
    assert np.array_equal(utf8, lstm_hip.dfa_utf8())  # a copy was restricted
    with_c3 = ascii_only.copy()
    with_c3[0xC3] = 1
    t = lstm_hip.dfa_restrict(utf8, with_c3)
    assert t[0, 0xC3] == cr.FORBID and cr.counts(t)[0] == 128  # its continuation state became empty
    latin = with_c3.copy()
    latin[0x80:0xC0] = 1
    t = lstm_hip.dfa_restrict(utf8, latin)
    assert t[0, 0xC3] == 1 and cr.counts(t)[0] == 129 and cr.counts(t)[1] == 64
    # the numbering is unchanged: what is still allowed leads where it led
    still = t != cr.FORBID
    assert np.array_equal(t[still], utf8[still]) and not (still & (utf8 == cr.FORBID)).any()
    # a chain: forbidding 80-BF empties states 1, 2, 5 and with them every state that only leads there
    no_cont = np.ones(256, np.uint8)
    no_cont[0x80:0xC0] = 0
    t = lstm_hip.dfa_restrict(utf8, no_cont)
    assert list(cr.counts(t)) == [128, 0, 0, 0, 0, 0, 0, 0]
    with pytest.raises(lstm_hip.LstmHipError, match="state 0"):
        lstm_hip.dfa_restrict(utf8, np.zeros(256, np.uint8))
    lib = lstm_hip.load_library()
    assert lib.lstm_hip_dfa_restrict(lstm_hip._ptr(utf8.copy(), lstm_hip.C.c_uint16), 8,
                                     lstm_hip._ptr(np.zeros(256, np.uint8), lstm_hip.C.c_uint8)) == lstm_hip.EINVAL
    # a one-state table
    one = lstm_hip.dfa_restrict(np.zeros((1, 256), np.uint16), with_c3)
    assert cr.counts(one)[0] == 129 and (one[0, :128] == 0).all()


def test_header_and_python_names():
    import ctypes as C
    import lstm_hip
    header = open(os.path.join(ROOT, "include", "lstm_hip.h")).read()
    assert re.search(r"int lstm_hip_generate_constrained\(lstm_hip_t \*h, int32_t streams,", header)
    assert re.search(r"int32_t lstm_hip_dfa_utf8\(uint16_t \*next\);", header)
    assert re.search(r"int lstm_hip_dfa_restrict\(uint16_t \*next, int32_t states, const uint8_t allow\[256\]\);", header)
    m = re.search(r"typedef struct lstm_hip_constraint \{(.*?)\} lstm_hip_constraint;", header, re.S)
    assert m
    fields = re.findall(r"^\s*(?:const\s+)?(\w+)\s+\*?(\w+);", m.group(1), re.M)
    assert fields == [("uint32_t", "size"), ("int32_t", "states"), ("uint16_t", "next")], fields
    decl = header[header.index("int lstm_hip_generate_constrained("):]
    decl = decl[:decl.index(";")]
    assert re.search(r"const lstm_hip_constraint \*con,\s*const int32_t \*start_state.*int32_t \*end_state", decl, re.S)
    for name in ("lstm_hip_generate_constrained", "lstm_hip_dfa_utf8", "lstm_hip_dfa_restrict"):
        assert name in lstm_hip.SYMBOLS and hasattr(lstm_hip.load_library(), name), name
    assert C.sizeof(lstm_hip._Constraint) == 16 and lstm_hip._Constraint.next.offset == 8  # the C layout on this ABI
    assert [f[0] for f in lstm_hip._Constraint._fields_] == ["size", "states", "next"]


def test_program_options():
    out = subprocess.run([GEN, "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    for flag in ("--utf8", "--allow", "--ban"):
        assert flag in out.stdout, flag
    base = [GEN, "--load", "nowhere", "--count", "1"]
    bad_specs = ["", "x", "256", "0x100", "10-", "-10", "9-3", "1,,2", "1,", "0x", "0xg1", "1-2-3", " 1", "1.5"]
    for opt in ("--allow", "--ban"):
        for spec in bad_specs:
            r = subprocess.run(base + [opt, spec], capture_output=True, text=True, timeout=60)
            assert r.returncode == 2, (opt, spec, r.returncode, r.stderr)
    for combo in (["--utf8", "--beams", "2"], ["--allow", "0x61-0x7a", "--beams", "2"], ["--ban", "10", "--beams", "2"],
                  ["--utf8", "--score", "some.txt"], ["--allow", "65", "--score", "some.txt"], ["--ban", "65", "--score", "some.txt"],
                  ["--allow", "65", "--ban", "65"],               # nothing left to draw
                  ["--utf8", "--allow", "0xc3"]):                 # a lead byte without its continuation: nothing left either
        r = subprocess.run(base + combo, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (combo, r.returncode, r.stderr)
    no_count = subprocess.run([GEN, "--load", "nowhere", "--score", "f", "--utf8"], capture_output=True, text=True, timeout=60)
    assert no_count.returncode == 2
    # good SPECs get past the options: the checkpoint is what fails (status 1)
    for good in (["--allow", "0x20-0x7e,10"], ["--ban", "0,255"], ["--utf8", "--allow", "0x20-0x7E,0xC3,0x80-0xbf"], ["--utf8"]):
        r = subprocess.run(base + good, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1, (good, r.returncode, r.stderr)


def test_control_of_the_gpu_oracle_comparison(oracle32):
    """The GPU test (tests/test_constraint.py) skips draws whose masked distribution is ambiguous and asserts that they are
    at most 5 %: here the same parameters, prompts, draws and settings on the float32 oracle alone, the reference rule of
    tests/constraint_ref.py choosing the bytes.  The eight one-byte prompts put the streams into the eight states of the
    UTF-8 automaton, so every state draws at least once; and the constraint must cut something: the mean kept count is
    below 256."""
    import lstm_hip
    table = lstm_hip.dfa_utf8()
    N, Cn = sr.ORACLE_N, sr.ORACLE_COUNT
    P, prompts, u = cr.oracle_case()
    assert len(prompts) == 8 and [cr.walk(table, 0, p) for p in prompts] == list(range(8))
    for top_k, top_p, tau in cr.ORACLE_SETTINGS:
        amb, keeps, drawing = [], [], set()
        for s in range(cr.ORACLE_STREAMS):
            xi = np.full((2, 1), -1, np.int32)
            xi[1, 0] = prompts[s][0]
            ti = np.full((2, 1), -1, np.int32)
            fw = oracle32.forward(N, M, 2, 1, P, xi, ti, np.zeros((1, N), np.float32), np.zeros((1, N), np.float32))
            h, c, q = fw["h"][1], fw["c"][1], s
            p1 = np.asarray(fw["probs"][1, 0], np.float64)
            for i in range(Cn):
                drawing.add(q)
                keep, mask, pp, p = cr.filter64(p1, table, q, tau, top_k, top_p)
                amb.append(cr.ambiguous(p, table, q, top_k, top_p))
                keeps.append(keep)
                cdf = np.cumsum(pp)
                x = int(min(np.searchsorted(cdf, u[i, s], side="right"), np.nonzero(mask)[0].max()))
                assert mask[x]
                q = int(table[q, x])
                xi[1, 0] = x  # one more step from (h, c) with input x
                fw = oracle32.forward(N, M, 2, 1, P, xi, ti, np.asarray(h, np.float32).reshape(1, N), np.asarray(c, np.float32).reshape(1, N))
                h, c = fw["h"][1], fw["c"][1]
                p1 = np.asarray(fw["probs"][1, 0], np.float64)
        print(f"top_k {top_k} top_p {top_p} tau {tau}: ambiguous {np.mean(amb):.4f}, mean kept {np.mean(keeps):.2f}, "
              f"drawing states {sorted(drawing)}")
        assert np.mean(amb) <= 0.05, (top_k, top_p, tau, np.mean(amb))
        assert drawing == set(range(8)), drawing
        assert np.mean(keeps) < 256, np.mean(keeps)
