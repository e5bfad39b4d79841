"""CPU side of lstm_hip_embed_texts (include/lstm_hip.h): the header, the export and SYMBOLS, the
schedule -- lstm_hip_text_plan on offsets that count every stream one byte longer -- against the numpy restatement of
tests/embed_ref.py, and the controls of the GPU comparison: H32, the yardstick of its tolerance, is what the table says, the
float32 statement passes it, and four mutants of the float64 reference fail it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import embed_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports():
    import lstm_hip
    text = open(os.path.join(ROOT, "include", "lstm_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\blstm_hip_embed_texts\s*\(", code)
    assert hasattr(lstm_hip.load_library(), "lstm_hip_embed_texts") and "lstm_hip_embed_texts" in lstm_hip.SYMBOLS
    assert "lstm_hip_embedding" in code
    assert C.sizeof(lstm_hip._Embedding) == 8 + 10 * C.sizeof(C.c_void_p)      # size (padded to a pointer), ten pointers
    assert "off'[s] = text_off[s] + s" in text                               # the plan is stated where a caller reads it
    assert hasattr(lstm_hip.Lstm, "embed_texts")


def _cases():
    rs = np.random.RandomState(6)
    edges = [0, 1, 2, 127, 128, 129, 256, 257]
    yield list(er.LENGTHS)
    yield edges[::-1] + edges
    yield [257]
    yield [0, 1, 0]
    for n in (2, 5, 40, 200):          # fewer streams than lanes and more
        yield list(rs.randint(0, 700, size=n))
        yield list(rs.choice(edges, size=n)) + list(rs.randint(0, 3000, size=3))


@pytest.mark.parametrize("lanes", [1, 3, 64])
def test_shifted_plan_is_the_restatement(lanes):
    import lstm_hip
    for lengths in _cases():
        windows, lane_of, first = lstm_hip.text_plan(er.STEPS, lanes, [int(L) + 1 for L in lengths])   # off'[s] = off[s] + s
        w_ref, l_ref, f_ref = er.plan_ref(lanes, lengths)
        assert windows == w_ref and np.array_equal(lane_of, l_ref) and np.array_equal(first, f_ref), (lanes, lengths)
        need = np.array([-(-int(L) // er.STEPS) for L in lengths])                # n = L steps: ceil(L / 128) windows
        free = np.zeros(lanes, np.int64)
        for s in range(len(lengths)):
            if need[s] == 0:
                assert lengths[s] == 0 and lane_of[s] == -1 and first[s] == -1
                continue
            assert first[s] == free[lane_of[s]] == free.min() and lane_of[s] == int(np.argmin(free)), (s, lengths)
            free[lane_of[s]] += need[s]
        assert windows == free.max()
        if lanes == 1:
            assert windows == need.sum()


def test_lengths_hold_the_window_edges():
    ends = {L % er.STEPS for L in er.LENGTHS if L}
    assert 0 in er.LENGTHS and 0 in ends and 1 in ends and er.STEPS - 1 in ends       # ends on the last row / single row / one short
    assert any(L > 2 * er.STEPS for L in er.LENGTHS)                                   # a stream of three windows


@pytest.mark.parametrize("N", sorted(er.H32))
def test_float32_statement_passes_and_pins_h32(N, oracle32, oracle64):
    """The yardstick of the GPU test's tolerance: H32 = max |state32 - state64| over the GPU case."""
    fresh = er.h32(oracle32, oracle64, N)
    print(f"N={N}: H32 = {fresh:.3g}, tolerance {er.tolerance(N):.3g}")
    assert fresh <= er.H32_CEILING * er.H32[N], (N, fresh)
    assert fresh >= er.H32[N] / 8, (N, fresh)        # (the table is not a loose guess either)
    if N > 128:
        return                                       # the comparison's control at the small widths: the states are the same run
    P, txts, h0, c0 = er.case(N)
    skip = _skip()
    want = er.embed(oracle64, N, P, txts, h0, c0, skip=skip)
    got = er.embed(oracle32, N, P, txts, h0, c0, skip=skip)
    figures, fails = er.compare(got, want, N)
    assert not fails, fails
    assert all(got[k].dtype == np.float32 for k in figures)


def _skip():
    # per LENGTHS (0, 1, 2, 127, 128, 129, 256, 257, 37, 5): none, past the end, inside, on a window's edge
    return [0, 1, 1, 40, 0, 128, 200, 130, 36, 9]


def test_pooling_as_stated():
    x = np.array([[1.0, -2.0], [3.0, -5.0], [-4.0, 0.5]], np.float32)
    start = np.array([9.0, 9.0], np.float32)
    mean, mx, last, count = er.pool_one(x, start, 3, 1)
    assert count == 2 and list(mean) == [-0.5, -2.25] and list(mx) == [3.0, 0.5] and list(last) == [-4.0, 0.5]
    mean, mx, last, count = er.pool_one(x, start, 3, 7)            # an empty pool: +0.0f, last unaffected by skip
    assert count == 0 and not mean.any() and not mx.any() and not np.signbit(mean).any() and list(last) == [-4.0, 0.5]
    mean, mx, last, count = er.pool_one(x[:0], start, 0, 0)        # the empty stream: the start state
    assert count == 0 and not mean.any() and not mx.any() and list(last) == [9.0, 9.0]
    assert mean.dtype == np.float32
    # the sum is a double sum: float32 accumulation would lose the small terms
    big = np.array([[1e8]] + [[1.0]] * 64, np.float32)
    assert er.pool_one(big, start[:1], 65, 0)[0][0] == np.float32((1e8 + 64) / 65)


def test_mutants_of_the_reference_are_caught(oracle64):
    N = 64
    P, txts, h0, c0 = er.case(N)
    skip = _skip()
    want = er.embed(oracle64, N, P, txts, h0, c0, skip=skip)
    assert list(want["count"]) == [0, 0, 1, 87, 128, 1, 56, 127, 1, 0]
    _, fails = er.compare(want, want, N)
    assert not fails
    before = er.embed(oracle64, N, P, txts, h0, c0, skip=skip, before=True)
    _, fails = er.compare(before, want, N)
    assert any(f.startswith("last_h") for f in fails) and any(f.startswith("mean_c") for f in fails), fails
    noskip = er.embed(oracle64, N, P, txts, h0, c0, skip=skip, ignore_skip=True)
    _, fails = er.compare(noskip, want, N)
    assert any(f.startswith("count") for f in fails) and any(f.startswith("mean_h") for f in fails), fails
    assert not any(f.startswith("last") for f in fails), fails                       # skip does not affect last
    dead = er.embed(oracle64, N, P, txts, h0, c0, skip=skip, dead=True)
    _, fails = er.compare(dead, want, N)
    assert any(f.startswith("mean_h") for f in fails) and any(f.startswith("max_") for f in fails), fails
    assert not any("stream 4 " in f or "stream 6 " in f for f in fails), fails       # 128 and 256 bytes: no dead row
    over = er.embed(oracle64, N, P, txts, h0, c0, skip=skip, over_steps=True)
    _, fails = er.compare(over, want, N)
    assert fails and all(f.startswith("mean_") for f in fails), fails
    assert not any("stream 4 " in f for f in fails), fails                           # count = 128: the same figure
