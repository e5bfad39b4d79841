"""CPU: the logic of k_code_head (eigen-lstm_amd/csrc/heads/code_head.inc) run on the host -- the kernel's
own text compiled with one thread per work-item (tests/code_head_emulation.cc) -- against the float32 statement of the table
rule in tests/code_table_ref.py and the Python copy of the range coder in tests/range_coder_ref.py, bit for bit: the trace
row of every coded byte (so cum, freq and T of the table the head built), the codes, their lengths, the coder's final state,
the bits, the inputs handed to the recurrence at every step and the error word; then the decoder on the emulated encoder's
codes, whole, truncated and damaged.  expf and log2 are the C library's on both sides.

Round trips cannot see a wrong table (encoder and decoder build the same one); this module can: profiles/code_table/mutants.txt
lists four one-token mutants of code_head.inc and the test of this module each one fails."""
import ctypes
import subprocess

import numpy as np
import pytest

import code_table_ref as ct
import head_emulation
import range_coder_ref as rc
from logits_ref import logits32

f32 = np.float32
M = 256
SENTINEL = 0xA5
FRONT, TAIL = 5, 7  # sentinel bytes before the first and after the last stream's code range
ERR_BOUND = 2       # CODE_ERR_BOUND of heads/head_args.h

_libm = ctypes.CDLL("libm.so.6")
_libm.log2.restype, _libm.log2.argtypes = ctypes.c_double, [ctypes.c_double]


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    return head_emulation.build(tmp_path_factory.mktemp("code_head"), "code_head_emulation")


def _bound(n):
    return 3 * n + 4 if n else 0


def _emulate(emulator, d, sb, Why, by, Hs, lengths, decode, text, code, code_base):
    """one run of the program: the outputs as a dict"""
    steps, K, N = Hs.shape[0] - 1, Hs.shape[1], Hs.shape[2]
    text_off = np.zeros(K + 1, np.uint64)
    text_off[1:] = np.cumsum(lengths)
    total = int(text_off[-1])
    assert text.size == total + 1
    for name, arr in (("why", Why), ("by", by), ("hs", Hs), ("text_off", text_off), ("text", text), ("code", code),
                      ("code_base", np.asarray(code_base, np.uint64))):
        np.ascontiguousarray(arr).tofile(f"{d}/{name}.bin")
    subprocess.check_call([emulator, d, str(N), str(K), str(steps), str(sb), str(int(decode))], timeout=300)
    return dict(code=np.fromfile(f"{d}/code_out.bin", np.uint8), text=np.fromfile(f"{d}/text_out.bin", np.uint8),
                trace=np.fromfile(f"{d}/trace.bin", np.uint32).reshape(total + 1, 3), bits=np.fromfile(f"{d}/bits.bin", np.float64),
                code_len=np.fromfile(f"{d}/code_len.bin", np.uint64), state=np.fromfile(f"{d}/state.bin", np.uint32).reshape(K, 6),
                xlog=np.fromfile(f"{d}/xlog.bin", np.int32).reshape(steps + 1, K), err=int(np.fromfile(f"{d}/err.bin", np.uint32)[0]),
                text_off=text_off)


def _tables(Why, by, Hs, lengths, exact):
    """tables[s][j] = (q, cum, T) of the state before byte j of stream s, by tests/code_table_ref.py"""
    out = []
    for s, L in enumerate(lengths):
        rows = []
        for j in range(L):
            if exact:  # every product and partial sum is a multiple of 1/256 below 2^8: float64 gives the float32 logits
                z = (Why.T.astype(np.float64) @ Hs[j, s].astype(np.float64) + by).astype(f32)
            else:
                with np.errstate(invalid="ignore"):
                    z = logits32(np.ascontiguousarray(Why.T), by, Hs[j, s])
            rows.append(ct.table32(z))
        out.append(rows)
    return out


def _state_words(st):
    """CoderState as its six 32-bit words: low, range, code, pad, pos (two words)"""
    return [st.low, st.range, st.code, 0, st.pos & 0xFFFFFFFF, st.pos >> 32]


def _check_encode(emulator, d, sb, Why, by, Hs, texts, exact, short=None):
    """Encodes `texts` in the emulator and holds every output to the reference.  short = (s, cap): stream s gets a code range of
    only cap bytes.  Returns (codes, tables, the Python coder's Stats per stream)."""
    K = len(texts)
    lengths = [len(t) for t in texts]
    caps = [_bound(n) for n in lengths]
    if short is not None:
        caps[short[0]] = short[1]
    code_base = FRONT + np.concatenate([[0], np.cumsum(caps)])
    code0 = np.full(int(code_base[-1]) + TAIL, SENTINEL, np.uint8)
    text = np.frombuffer(b"".join(texts) + b"\0", np.uint8)
    got = _emulate(emulator, d, sb, Why, by, Hs, lengths, False, text, code0, code_base)
    tables = _tables(Why, by, Hs, lengths, exact)
    steps = Hs.shape[0] - 1
    want_code = code0.copy()
    codes, stats = [], []
    for s, t in enumerate(texts):
        L, o = lengths[s], int(got["text_off"][s])
        rows = [(int(tables[s][j][1][x]), int(tables[s][j][0][x]), tables[s][j][2]) for j, x in enumerate(t)]
        assert [tuple(int(v) for v in r) for r in got["trace"][o:o + L]] == rows, s
        st = rc.Stats()
        code = rc.encode(rows, st)
        codes.append(code)
        stats.append(st)
        assert len(code) <= _bound(L)
        beg = int(code_base[s])
        n = min(len(code), caps[s])
        want_code[beg:beg + n] = np.frombuffer(code[:n], np.uint8)
        assert int(got["code_len"][s]) == len(code), s
        assert list(got["xlog"][:, s]) == list(t) + [-1] * (steps + 1 - L), s
        bits = 0.0
        for _, freq, T in rows:
            bits += -_libm.log2(freq / T)
        assert got["bits"][s] == bits, s
        if L:
            assert list(got["state"][s]) == _state_words(st), (s, list(got["state"][s]), _state_words(st))
        else:
            assert (got["state"][s] == 0xEEEEEEEE).all(), s  # an empty stream's state is never touched
    assert np.array_equal(got["code"], want_code)  # every code, and every sentinel outside the codes
    assert np.array_equal(got["text"], text)
    assert not got["trace"][-1].any()
    assert got["err"] == (ERR_BOUND if short is not None and len(codes[short[0]]) > short[1] else 0)
    return codes, tables, stats


def _check_decode(emulator, d, sb, Why, by, Hs, lengths, tables, codes):
    """Decodes `codes` (any bytes) in the emulator: the text, the inputs handed on and the final state are those of
    range_coder_ref.decode on the same codes and tables.  Between the streams' code ranges lie bytes of 0xFF that belong to
    a stream with no text, so a read past a stream's own range (which must read 0) would show.  Returns (the texts, the clamped steps)."""
    K = len(lengths)
    gap = 6
    # stream 2i is the i-th real stream, stream 2i + 1 an empty one that owns the 0xFF bytes behind its code
    lengths2, codes2, Hs2 = [], [], np.zeros((Hs.shape[0], 2 * K, Hs.shape[2]), f32)
    for s in range(K):
        lengths2 += [lengths[s], 0]
        codes2 += [codes[s], b"\xff" * gap]
        Hs2[:, 2 * s] = Hs[:, s]
    code = np.frombuffer(b"".join(codes2) + b"\xff", np.uint8)
    code_base = np.concatenate([[0], np.cumsum([len(c) for c in codes2])])
    total = sum(lengths)
    text0 = np.full(total + 1, SENTINEL, np.uint8)
    got = _emulate(emulator, d, sb, Why, by, Hs2, lengths2, True, text0, code, code_base)
    assert got["err"] == 0
    assert np.array_equal(got["code"], code)
    assert got["text"][-1] == SENTINEL
    steps = Hs.shape[0] - 1
    back, clamps = [], 0
    for s in range(K):
        L, o = lengths[s], int(got["text_off"][2 * s])
        st = rc.Stats()
        want = rc.decode(codes[s], L, rc.table_model([tables[s][j][0].tolist() for j in range(L)]), st)
        assert list(got["text"][o:o + L]) == want, s
        assert list(got["xlog"][:, 2 * s]) == want + [-1] * (steps + 1 - L), s
        assert (got["xlog"][:, 2 * s + 1] == -1).all()
        if L:
            assert list(got["state"][2 * s]) == _state_words(st), s
        clamps += st.clamps
        back.append(bytes(want))
    return back, clamps


def _ragged(sb, rs):
    """stream lengths for groups of sb: a mixed group with an empty and one-byte streams; a group that has ended (lengths
    0 and 1) while the others go on; a group where only the last stream is still active after step 1; a partial last group"""
    if sb == 1:
        return [5, 0, 1, 7, 3]
    mixed = [5, 0, 1, 3, 1, 6, 2, 0, 4, 1, 0, 7, 3, 1, 2, 5]
    lengths = mixed[:sb] + [int(v) for v in rs.randint(0, 2, size=sb)] + [1] * (sb - 1) + [7]
    lengths += ([4, 0, 1, 6, 2, 1, 0, 3] * 2)[:max(sb - 1, 1)]
    return lengths


@pytest.mark.parametrize("sb", [1, 2, 4, 8, 16])
def test_every_group_size_with_ragged_lengths(emulator, tmp_path, sb):
    """exact logits (N = 16; Why, by and h multiples of 1/16), so the table is the statement's whatever the summation order"""
    N = 16
    rs = np.random.RandomState(100 + sb)
    lengths = _ragged(sb, rs)
    K = len(lengths)
    assert (K % sb != 0 or sb == 1) and 0 in lengths and 1 in lengths
    Why = (rs.randint(-32, 33, size=(N, M)) / 16).astype(f32)  # [k][m]
    by = (rs.randint(-16, 17, size=M) / 16).astype(f32)
    Hs = (rs.randint(-16, 17, size=(max(lengths) + 1, K, N)) / 16).astype(f32)
    texts = [bytes(rs.randint(0, 256, size=n).astype(np.uint8)) for n in lengths]
    codes, tables, _ = _check_encode(emulator, str(tmp_path), sb, Why, by, Hs, texts, exact=True)
    # the streams of a group do not share a table: their maxima differ
    assert len({t[0][2] for t in tables if t}) > 1
    assert _check_decode(emulator, str(tmp_path), sb, Why, by, Hs, lengths, tables, codes)[0] == texts


def test_random_float32_values_follow_the_k_order(emulator, tmp_path):
    """N = 48, random float32 parameters and states: the logits are the sequential sum of tests/logits_ref.py, bit for bit"""
    N, sb = 48, 2
    rs = np.random.RandomState(7)
    lengths = [6, 3, 0, 5, 1]
    K = len(lengths)
    # a large part common to all bytes (it cancels in z - max z) under the part that tells them apart: the partial sums are in the
    # hundreds, so their rounding, which depends on the order of k, moves z by 1e-4 and several q of every table by one
    Why = (64.0 * rs.standard_normal((N, 1)) + 0.6 * rs.standard_normal((N, M))).astype(f32)
    by = rs.standard_normal(M).astype(f32)
    Hs = rs.uniform(-1, 1, size=(max(lengths) + 1, K, N)).astype(f32)
    texts = [bytes(rs.randint(0, 256, size=n).astype(np.uint8)) for n in lengths]
    codes, tables, _ = _check_encode(emulator, str(tmp_path), sb, Why, by, Hs, texts, exact=False)
    # (the order matters here: the same sum taken from k = N - 1 down gives other logits, and another table)
    rows = [(s, j) for s in range(K) for j in range(lengths[s])]
    other = sum(not np.array_equal(ct.table32(logits32(np.ascontiguousarray(Why.T[:, ::-1]), by, Hs[j, s][::-1]))[0], tables[s][j][0])
                for s, j in rows)
    assert 2 * other > len(rows), (other, len(rows))
    assert _check_decode(emulator, str(tmp_path), sb, Why, by, Hs, lengths, tables, codes)[0] == texts


def _saturated_case(seed):
    """by puts byte 77 forty above the rest (h = 0): q_77 = 65025, every other q = 1, T = 65280.  Streams: a run of the likely
    byte; unlikely bytes only; a mixture."""
    rs = np.random.RandomState(seed)
    by = np.zeros(M, f32)
    by[77] = 40.0
    texts = [b"\x4d" * 14, bytes(rs.randint(0, 256, size=12).astype(np.uint8)),
             bytes(np.where(rs.random_sample(40) < 0.5, 77, rs.randint(0, 256, size=40)).astype(np.uint8)), b"\x4d", b"\x00"]
    return by, texts


def _paths(stats):
    """(steps with a cut, steps that moved three bytes, the longest run of steps that moved no byte) of the Python coder"""
    quiet = 0
    for st in stats:
        run = 0
        for n in st.moves:
            run = 0 if n else run + 1
            quiet = max(quiet, run)
    return sum(st.cuts for st in stats), sum(n == 3 for st in stats for n in st.moves), quiet


SATURATED_SEED = 11  # chosen on the CPU: with it the reference alone takes the cut and a three-move step (asserted below)


def test_saturated_table(emulator, tmp_path):
    N, sb = 16, 4
    by, texts = _saturated_case(SATURATED_SEED)
    q, cum, T = ct.table32(by)
    assert q[77] == 65025 and T == 65280 and (np.delete(q, 77) == 1).all()
    lengths = [len(t) for t in texts]
    Why = np.zeros((N, M), f32)
    Hs = np.zeros((max(lengths) + 1, len(texts), N), f32)
    codes, tables, stats = _check_encode(emulator, str(tmp_path), sb, Why, by, Hs, texts, exact=True)
    cuts, three, quiet = _paths(stats)  # of the Python coder, whose bytes and final states the emulation has just matched
    assert cuts >= 1 and three >= 1 and quiet >= 5, (cuts, three, quiet)
    assert len(codes[0]) == 4  # fourteen likely bytes moved nothing: the flush alone
    assert _check_decode(emulator, str(tmp_path), sb, Why, by, Hs, lengths, tables, codes)[0] == texts


def test_entries_at_the_threshold_of_one(emulator, tmp_path):
    """p * 65024 within 4 % of 1 for 255 bytes, on both sides: q is 1 or 2 as the float32 product says"""
    N, sb = 16, 2
    by = np.zeros(M, f32)
    by[1:] = np.linspace(-11.12, -11.04, 255).astype(f32)  # 65024 e^d / s = 1 at d = -11.0786 (s = 1 + 255 e^d ~ 1.0039)
    v = ct.statement64(by)
    assert v[1:].min() < 0.97 and v[1:].max() > 1.03 and np.abs(v[1:] - 1).min() < 2e-4
    q = ct.table32(by)[0]
    assert set(q[1:].tolist()) == {1, 2} and (q[1:] == 1).sum() > 50 and (q[1:] == 2).sum() > 50
    texts = [bytes(range(120, 146)), bytes(range(255, 0, -12)), b"\x00\x01"]  # (the change from q = 1 to q = 2 lies in 120..145)
    assert {int(q[x]) for x in texts[0]} == {1, 2}
    lengths = [len(t) for t in texts]
    Why = np.zeros((N, M), f32)
    Hs = np.zeros((max(lengths) + 1, len(texts), N), f32)
    _check_encode(emulator, str(tmp_path), sb, Why, by, Hs, texts, exact=True)


@pytest.mark.parametrize("which", ["nan_in_h", "inf_in_by"])
def test_a_row_that_is_not_finite_has_a_flat_table(emulator, tmp_path, which):
    N, sb = 16, 4
    rs = np.random.RandomState(11)
    lengths = [4, 4, 3, 0, 2]
    K = len(lengths)
    Why = (rs.randint(-32, 33, size=(N, M)) / 16).astype(f32)
    by = (rs.randint(-16, 17, size=M) / 16).astype(f32)
    Hs = (rs.randint(-16, 17, size=(max(lengths) + 1, K, N)) / 16).astype(f32)
    if which == "nan_in_h":
        Hs[2, 1, 5] = np.nan  # byte 2 of stream 1 alone
        flat = {(1, 2)}
    else:
        by[200] = np.inf      # every row
        flat = {(s, j) for s in range(K) for j in range(lengths[s])}
    texts = [bytes(rs.randint(0, 256, size=n).astype(np.uint8)) for n in lengths]
    codes, tables, _ = _check_encode(emulator, str(tmp_path), sb, Why, by, Hs, texts, exact=which == "inf_in_by")
    for s in range(K):
        for j in range(lengths[s]):
            is_flat = np.array_equal(tables[s][j][0], ct.FLAT[0]) and tables[s][j][2] == ct.FLAT[2]
            assert is_flat == ((s, j) in flat), (s, j)  # trace (x, 1, 256) there (the trace was held to the tables), and only there
    assert _check_decode(emulator, str(tmp_path), sb, Why, by, Hs, lengths, tables, codes)[0] == texts


def test_truncated_and_damaged_codes_decode_as_the_python_coder(emulator, tmp_path):
    N, sb = 16, 2
    rs = np.random.RandomState(21)
    lengths = [9, 6, 1]
    K = len(lengths)
    Why = (rs.randint(-32, 33, size=(N, M)) / 16).astype(f32)
    by = (rs.randint(-16, 17, size=M) / 16).astype(f32)
    Hs = (rs.randint(-16, 17, size=(max(lengths) + 1, K, N)) / 16).astype(f32)
    texts = [bytes(rs.randint(0, 256, size=n).astype(np.uint8)) for n in lengths]
    codes, tables, _ = _check_encode(emulator, str(tmp_path), sb, Why, by, Hs, texts, exact=True)
    clamps = 0
    for cut in (0, 1, len(codes[0]) // 2):
        back, n = _check_decode(emulator, str(tmp_path), sb, Why, by, Hs, lengths, tables, [codes[0][:cut], codes[1], codes[2][:cut]])
        clamps += n
        assert [len(b) for b in back] == lengths and back[1] == texts[1]
    # a code of 0xFF bytes: (code - low) / r is at least T at the first step
    clamps += _check_decode(emulator, str(tmp_path), sb, Why, by, Hs, lengths, tables, [b"\xff" * 8, codes[1], b"\xff"])[1]
    assert clamps >= 1  # (counted by the Python coder, which the emulated decoder matched)


def test_a_code_range_shorter_than_the_code(emulator, tmp_path):
    """the error word carries CODE_ERR_BOUND, the code's prefix fills the range, and nothing outside it is written: the
    neighbours' codes and the sentinels around them are as without the fault"""
    N, sb = 16, 4
    rs = np.random.RandomState(31)
    lengths = [6, 8, 5]
    Why = (rs.randint(-32, 33, size=(N, M)) / 16).astype(f32)
    by = (rs.randint(-16, 17, size=M) / 16).astype(f32)
    Hs = (rs.randint(-16, 17, size=(max(lengths) + 1, len(lengths), N)) / 16).astype(f32)
    texts = [bytes(rs.randint(0, 256, size=n).astype(np.uint8)) for n in lengths]
    codes, _, _ = _check_encode(emulator, str(tmp_path), sb, Why, by, Hs, texts, exact=True)
    assert len(codes[1]) > 7
    for cap in (len(codes[1]) - 1, 3, 0):  # (short by the last flush byte; short within the steps; no range at all)
        _check_encode(emulator, str(tmp_path), sb, Why, by, Hs, texts, exact=True, short=(1, cap))  # asserts err == CODE_ERR_BOUND
