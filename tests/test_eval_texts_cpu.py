"""CPU side of lstm_hip_eval_texts (include/lstm_hip.h): the header and the exports, the schedule
(lstm_hip_eval_plan runs on the host) against the numpy restatement of tests/eval_texts_ref.py, the refusals that need no
device, the split of one text into streams, and the controls of the GPU comparison: the float32 statement passes it, the two
mutants of the float64 reference fail it, and D32, the yardstick of its per-byte tolerance, is what the table says."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import eval_texts_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def test_header_declares_and_library_exports():
    import lstm_hip
    text = open(os.path.join(ROOT, "include", "lstm_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("lstm_hip_eval_plan", "lstm_hip_eval_texts"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(lstm_hip.load_library(), name) and name in lstm_hip.SYMBOLS
    assert re.search(r"#define\s+LSTM_HIP_EVAL_STEPS\s+128\b", code) and lstm_hip.EVAL_STEPS == er.STEPS == 128
    assert "lstm_hip_eval_opt" in code and C.sizeof(lstm_hip._EvalOpt) == 8


def _cases():
    rs = np.random.RandomState(5)
    edges = [0, 1, 2, 128, 129, 130, 257]
    yield edges
    yield edges[::-1] + edges
    yield [257]
    yield [0, 1, 0]
    for n in (2, 5, 40, 200):          # fewer streams than lanes and more
        yield list(rs.randint(0, 700, size=n))
        yield list(rs.choice(edges, size=n)) + list(rs.randint(0, 3000, size=3))


@pytest.mark.parametrize("lanes", [1, 3, 64])
def test_plan_is_the_restatement(lanes):
    import lstm_hip
    for lengths in _cases():
        windows, lane_of, first = lstm_hip.eval_plan(lanes, lengths)
        w_ref, l_ref, f_ref = er.plan_ref(lanes, lengths)
        assert windows == w_ref and np.array_equal(lane_of, l_ref) and np.array_equal(first, f_ref), (lanes, lengths)
        # the properties, stated on their own
        need = np.array([-(-max(int(L) - 1, 0) // er.STEPS) for L in lengths])
        taken = set()
        free = np.zeros(lanes, np.int64)
        for s in range(len(lengths)):
            if need[s] == 0:
                assert lane_of[s] == -1 and first[s] == -1
                continue
            assert 0 <= lane_of[s] < lanes
            assert first[s] == free[lane_of[s]] == free.min() and lane_of[s] == int(np.argmin(free)), (s, lengths)   # first free
            for w in range(int(first[s]), int(first[s] + need[s])):
                assert (int(lane_of[s]), w) not in taken
                taken.add((int(lane_of[s]), w))
            free[lane_of[s]] += need[s]
        assert windows == free.max()
        if lanes == 1:
            assert windows == need.sum()


def test_plan_refusals():
    import lstm_hip
    lib = lstm_hip.load_library()
    ok = np.array([0, 3, 3, 10], np.uint64)
    p = lstm_hip._ptr(ok, C.c_uint64)
    assert lib.lstm_hip_eval_plan(2, 3, p, None, None) == 1          # outputs may be NULL
    for lanes, streams, off, word in ((0, 3, ok, "lanes"), (4097, 3, ok, "lanes"), (-1, 3, ok, "lanes"), (2, 0, ok, "streams"),
                                      (2, 3, None, "null text_off"), (2, 3, np.array([1, 3, 3, 10], np.uint64), "must be 0"),
                                      (2, 3, np.array([0, 3, 2, 10], np.uint64), "decreases")):
        rc = lib.lstm_hip_eval_plan(lanes, streams, lstm_hip._ptr(off, C.c_uint64) if off is not None else None, None, None)
        assert rc == EINVAL and word in lib.lstm_hip_last_error().decode(), (lanes, streams, lib.lstm_hip_last_error())
    with pytest.raises(lstm_hip.LstmHipError):
        lstm_hip.eval_plan(0, [5])


def test_split_scores_every_byte_once():
    import lstm_hip
    for L in (2, 3, 100, 257, 1000):
        for pieces in (1, 2, 7, 64):
            for warm in (0, 5, 64, 5000):
                cut = lstm_hip.eval_split_pieces(L, pieces, warm)
                assert cut == er.split_ref(L, pieces, warm)
                hits = np.zeros(L, int)
                for a, b, skip in cut:
                    assert 0 <= a and b <= L and a + skip >= 1
                    hits[a + max(skip, 1):b] += 1          # the bytes the stream scores, at their place in the text
                    assert a == max(0, a + skip - 1 - warm)
                assert hits[0] == 0 and (hits[1:] == 1).all(), (L, pieces, warm)
    for bad in ((1, 1, 0), (10, 0, 0), (10, 2, -1)):
        with pytest.raises(lstm_hip.LstmHipError):
            lstm_hip.eval_split_pieces(*bad)


def test_split_with_full_warmup_is_the_single_stream(oracle64):
    import gpu_util as gu
    N = 16
    P = gu.random_case(N, 2, 1, seed=3, scale=0.3)[0]
    text = gu.text_bytes(90, 4)
    one = er.eval64(oracle64, N, P, [text])
    whole = float(one["bits"][0]) / (text.size - 1)
    assert abs(er.split_bits64(oracle64, N, P, text, 1, 0) - whole) == 0
    for pieces in (3, 8):
        assert abs(er.split_bits64(oracle64, N, P, text, pieces, text.size) - whole) <= 1e-12 * whole
        assert abs(er.split_bits64(oracle64, N, P, text, pieces, 0) - whole) > 1e-6     # (without warm-up it is another figure)
        # every byte once, on the reference: the pieces' entries, laid over the text, cover 1 .. L - 1
        cut = er.split_ref(text.size, pieces, 7)
        res = er.eval64(oracle64, N, P, [text[a:b] for a, b, _ in cut], skip=[k for _, _, k in cut])
        hits = np.zeros(text.size, int)
        for (a, b, _), sur in zip(cut, res["surprisal"]):
            hits[a:b] += sur > 0
        assert hits[0] == 0 and (hits[1:] == 1).all()


@pytest.mark.parametrize("N", sorted(er.D32))
def test_float32_statement_passes_and_pins_d32(N, oracle32, oracle64):
    """The yardstick of the GPU test's per-byte tolerance: D32 = max |score32 - score64| over the GPU case."""
    P, txts, h0, c0 = er.case(N)
    want = er.eval64(oracle64, N, P, txts, h0, c0)
    got = er.eval32(oracle32, N, P, txts, h0, c0)
    figures, fails = er.compare(got, want, N)
    print(f"N={N}: D32 = {figures['surprisal']:.3g} bits per byte, bits per scored byte off by {figures['bits_per_byte']:.3g}")
    assert not fails, fails
    assert figures["surprisal"] <= er.D32_CEILING * er.D32[N], (N, figures)
    assert figures["surprisal"] >= er.D32[N] / 8, (N, figures)   # (the table is not a loose guess either)


def test_mutants_of_the_reference_are_caught(oracle64):
    N = 64
    P, txts, h0, c0 = er.case(N)
    skip = [0, 1, 1, 40, 0, 129, 200, 36, 2, 0]
    want = er.eval64(oracle64, N, P, txts, h0, c0, skip=skip)
    _, fails = er.compare(want, want, N, skip)
    assert not fails
    late = er.eval64(oracle64, N, P, txts, h0, c0, skip=skip, late=True)
    _, fails = er.compare(late, want, N, skip)
    assert any("surprisal differs" in f for f in fails) and any("bits" in f for f in fails), fails
    noskip = er.eval64(oracle64, N, P, txts, h0, c0, skip=skip, ignore_skip=True)
    _, fails = er.compare(noskip, want, N, skip)
    assert any("unscored" in f for f in fails), fails
    # counts of scored bytes
    assert list(er.scored([0, 1, 2, 130], None)) == [0, 0, 1, 129] and list(er.scored([130, 130, 5], [1, 129, 9])) == [129, 1, 0]
