"""The input generators of gpu_util (window_bytes) and the reference-only control of tests/test_input_statistics.py.

The control: for every (shape, distribution) case the GPU file checks against the float64 oracle, the float32 oracle -- a
correct float32 implementation with another summation order and libm -- goes through the same assertions
(input_stats_cases.check_window) with every tolerance cut to a quarter.  A case that could not meet this would be one whose
tolerance sits inside float32 rounding, and would have to shrink.

Measured, float32 against float64 oracle, worst over the 95 fp32 cases: last h 6.4e-7 of scale (a quarter of the tolerance:
5e-6), loss 3.3e-6 bits per step (5e-6), gradients per tensor 9.1e-6 (5e-5), dW per used byte column 9.1e-6 (5e-5), db minus
the dW columns 4.5e-6 of max|db| (5e-5); absent bytes' columns, all_empty's loss and dW exactly 0.  One case did not meet it
and shrank: one byte as input and target over 18 216 columns, where the float32 oracle's serial sums are off by 8.1e-5 in dW
and 9.7e-4 bits -- the target variants run on windows of at most 1 300 columns (input_stats_cases.TARGET_VARIANT_MAX_T).
"""
import os
import re

import numpy as np
import pytest

import gpu_util as gu
import input_stats_cases as isc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES_SB = sorted({(sh.S, sh.B) for sh in isc.SHAPES} | {(20, 32)})


@pytest.mark.parametrize("kind", gu.DISTRIBUTIONS)
def test_generators_are_seeded_and_well_formed(kind):
    for S, B in SHAPES_SB:
        for target in gu.TARGETS:
            xi, ti = gu.window_bytes(kind, S, B, 5, target)
            xj, tj = gu.window_bytes(kind, S, B, 5, target)
            assert np.array_equal(xi, xj) and np.array_equal(ti, tj)
            assert xi.shape == ti.shape == (S, B) and xi.dtype == ti.dtype == np.int32
            assert xi.min() >= -1 and xi.max() <= 255 and ti.min() >= -1 and ti.max() <= 255
            assert np.array_equal(xi < 0, ti < 0)                       # an empty column is empty on both sides
            if target == "one_byte":
                assert np.all(ti[xi >= 0] == gu.ONE_BYTE)
            if target == "same":
                assert np.array_equal(xi, ti)


def test_uniform_is_the_control_draw():
    xi, _ = gu.window_bytes("uniform", 100, 64, 1)
    sizes = gu.bucket_sizes(xi)
    assert sizes[256] == 0 and np.count_nonzero(sizes) == 256 and sizes.max() < 3 * 99 * 64 / 256


def test_text_follows_the_byte_histogram():
    counts = gu.byte_histogram()
    assert np.count_nonzero(counts) == 195 and abs(counts.max() / counts.sum() - 0.134) < 1e-3
    xi, _ = gu.window_bytes("text", 100, 272, 2)
    sizes = gu.bucket_sizes(xi)
    T = 99 * 272
    assert sizes[256] == 0 and not np.any(sizes[:256][counts == 0])     # only bytes the text has
    top = int(np.argmax(counts))
    assert top == 32 and abs(sizes[top] / T - 0.134) < 0.01             # a bucket of thousands: > 100 chunks of DW_CHUNK
    assert sizes[top] > 100 * 32
    assert np.count_nonzero(sizes == 1) > 0                             # and bytes seen once


def test_one_byte_and_edges_and_empties():
    S, B = 70, 264
    T = (S - 1) * B
    sizes = gu.bucket_sizes(gu.window_bytes("one_byte", S, B, 3)[0])
    assert sizes[gu.ONE_BYTE] == T and np.count_nonzero(sizes) == 1
    for s, b in SHAPES_SB:
        sizes = gu.bucket_sizes(gu.window_bytes("edges", s, b, 3)[0])
        assert sizes[0] + sizes[255] == (s - 1) * b and sizes[255] >= 1 and sizes[0] > 50 * sizes[255]
    sizes = gu.bucket_sizes(gu.window_bytes("edges", 100, 1000, 4)[0])
    assert 0.0003 < sizes[255] / 99000 < 0.003                          # 999 : 1
    xi, ti = gu.window_bytes("empty_head", S, B, 3)
    half = (S + 1) // 2
    assert np.all(xi[:half] == -1) and np.all(ti[:half] == -1) and np.all(xi[half:] >= 0) and np.all(ti[half:] >= 0)
    xi, ti = gu.window_bytes("all_empty", S, B, 3)
    assert np.all(xi == -1) and np.all(ti == -1) and gu.bucket_sizes(xi)[256] == T


@pytest.mark.parametrize("k", [8, 4])
def test_group_collide_shares_one_byte_per_column_group(k):
    S, B = 40, 33
    xi, _ = gu.window_bytes(f"group_collide{k}", S, B, 7)
    for g in range((B + k - 1) // k):
        cols = xi[:, g * k:(g + 1) * k]
        assert np.all(cols == cols[:, :1])                              # depends only on (t, b // k)
        if g > 0:
            assert np.all(xi[:, g * k] != xi[:, g * k - 1])             # neighbouring groups differ
    assert np.unique(xi[:, 0]).size > S // 2                            # and the byte changes from step to step


def test_chunk_edges_has_the_chunk_boundary_buckets():
    for S, B in SHAPES_SB:
        T = (S - 1) * B
        if T < gu.CHUNK_EDGE_MIN_T:
            with pytest.raises(AssertionError):
                gu.window_bytes("chunk_edges", S, B, 0)
            continue
        xi, _ = gu.window_bytes("chunk_edges", S, B, 0)                 # (the generator asserts its layout itself)
        sizes = gu.bucket_sizes(xi)
        assert sorted(sizes[sizes > 0]) == sorted([1, 31, 32, 33, 64, 65, T - 226])
        assert sizes[gu.CHUNK_EDGE_ABSENT] == 0 and sizes[0] == 31 and sizes[255] == 1
    assert all((sh.S - 1) * sh.B >= gu.CHUNK_EDGE_MIN_T for sh in isc.SHAPES)


def test_dW_byte_report_sees_a_lost_column_the_tensor_figure_hides():
    """The reason for the per-column bound: drop the one column of a byte seen once under a skewed distribution."""
    N, S, B = 32, 30, 16
    rs = np.random.RandomState(1)
    xi, _ = gu.window_bytes("chunk_edges", S, B, 0)
    dg = rs.randn((S - 1) * B, 4 * N)
    ref = np.zeros(gu.random_case(N, 2, 1, 0)[0].size)
    W = ref[:4 * N * 256].reshape(256, 4 * N)
    np.add.at(W, xi[1:].ravel(), dg)
    bad = ref.copy()
    bad[:4 * N * 256].reshape(256, 4 * N)[255] = 0.0                    # the bucket of one column, lost
    assert gu.grads_report(bad, ref, N)["W"] < 0.5
    worst, byte, size, nonzero_absent = gu.dW_byte_report(bad, ref, N, xi)
    assert (worst, byte, size, nonzero_absent) == (1.0, 255, 1, [])
    bad = ref.copy()
    bad[:4 * N * 256].reshape(256, 4 * N)[gu.CHUNK_EDGE_ABSENT, 3] = 1e-30   # a stray write into an absent byte's column
    assert gu.dW_byte_report(bad, ref, N, xi)[3] == [gu.CHUNK_EDGE_ABSENT]


def test_case_table_covers_every_path_and_distribution():
    by_path = {}
    for c in isc.CASES:
        by_path.setdefault(c.shape.path, set()).add(c.dist)
    assert len(by_path) == 8
    for path, dists in by_path.items():
        assert set(isc.CORE) <= dists, path
    for fused in (0, 1):
        dists = {c.dist for c in isc.CASES if c.shape.plan["fused"] == fused}
        assert dists == set(gu.DISTRIBUTIONS), fused
    assert {c.target for c in isc.CASES} == set(gu.TARGETS)
    assert len({isc.case_id(c) for c in isc.CASES}) == len(isc.CASES)
    for sh in isc.SHAPES:                                               # the sums' thresholds, by window length
        T = (sh.S - 1) * sh.B
        want = "fold" if sh.plan["fused"] else "table" if T <= isc.DWT_MAX_T else "rank" if T <= isc.RANK_MAX_T else "sort"
        assert sh.dw == want, sh


def test_thresholds_match_the_kernel_source():
    src = open(os.path.join(ROOT, "eigen-lstm_amd", "csrc", "kernels.hip")).read()
    assert int(re.search(r"DWT_MAX_T = (\d+)", src).group(1)) == isc.DWT_MAX_T
    assert 64 * 16 * int(re.search(r"constexpr int RANK_SLOTS = (\d+)", src).group(1)) == isc.RANK_MAX_T
    assert "T <= 64 * 16 * RANK_SLOTS" in src and "T <= DWT_MAX_T" in src


FP32_CASES = [c for c in isc.CASES if not isc.bf16(c)]


@pytest.fixture(scope="module")
def references(request):
    pool = isc.ReferencePool(isc.selected_cases(request), with_f32=True)
    yield pool
    pool.close()


@pytest.mark.parametrize("case", FP32_CASES, ids=isc.case_id)
def test_float32_oracle_meets_a_quarter_of_every_tolerance(case, references):
    ref64, ref32 = references.get(case)
    xi = isc.inputs(case)[1]
    isc.check_window(case, ref32, ref64, xi, fraction=0.25)
