"""The parameter and state generators of gpu_util (regime_params, regime_state, tile_params) and the reference-only control of
tests/test_param_statistics.py.

The control: for every fp32 input the GPU file checks against the float64 oracle, the float32 oracle -- a correct float32
implementation with another summation order and libm -- goes through the same assertions (param_stats_cases.check_window) with
every tolerance cut to a quarter; at the extremes that is param_stats_cases.CONTROL_DISTANCE itself, which is how those
constants were fixed, before any device figure was seen.  It runs where (S-1) * B * N^2 <= CONTROL_MAX_WORK; the four larger
inputs' control figures are computed beside their references by the GPU file, asserted there and recorded.

The regime assertions keep the cases from drifting back to the linear regime.  The mutation proves the gap: the float32 oracle
with every gate pre-activation clamped to +-8 (ref_set_gate_clamp) returns the SAME BITS on every `gauss` case -- so no test
on Gaussian parameters can see it -- and fails check_window at the full tolerances on every `saturated` case.

Measured, float32 against float64 oracle, worst over the fp32 inputs (the larger ones included):
h, c, g, probs at their worst step 4.7e-6 of scale (a quarter of the tolerance: 5e-6; 512x100x64 tiled_A), loss 1.5e-6 bits
per step (5e-6), gradients per tensor 4.0e-6 (5e-5), per row of dW and dU and per column of dWhy 3.0e-5 (5e-5; 100x24x16
saturated), update step 1.5e-6 of lr (5e-5), last h after it 1.9e-6 (5e-6); at the extremes small gates 7.4e-6, 1 - g 1.04e-3,
1 - |c| 3.8e-6, p(target) 1.5e-5: param_stats_cases.CONTROL_DISTANCE, rounded up.  Three cases did not meet the quarter on
probs and were dropped, one shrank (param_stats_cases.DROPPED, and the comment at the (64, 40, 1) row).  The regimes, on the
float64 reference: `saturated` 25-27 % of the sigmoid gates outside (0.01, 0.99), p(target) 3e-11 ... 0.9; tiled_A 2-3 %,
p(target) 9e-6 ... 0.997, median 0.06-0.13; `gauss` none, p(target) 3e-3 ... 5e-3.  The clamped oracle on `saturated`: h off by
4.3e-4 ... 4.1e-3 of scale, small gates by a factor 270 ... 29 000, 1 - g by 5.5 floors, rows of dW by 9e-3 ... 0.18.
"""
import numpy as np
import pytest

import gpu_util as gu
import param_stats_cases as psc
from oracle_lib import split_params


@pytest.mark.parametrize("regime", gu.PARAM_REGIMES)
def test_generators_are_seeded_and_well_formed(regime, oracle64):
    N = 64
    P, Q = gu.regime_params(regime, N, 5), gu.regime_params(regime, N, 5)
    assert P.dtype == np.float32 and P.size == oracle64.param_count(N) and np.array_equal(P, Q)
    assert np.isfinite(P).all()
    for kind in gu.STATE_REGIMES:
        h0, c0 = gu.regime_state(kind, N, 9, 5)
        assert h0.shape == c0.shape == (9, N) and h0.dtype == c0.dtype == np.float32
        assert np.array_equal(h0, gu.regime_state(kind, N, 9, 5)[0])
        assert np.abs(c0).max() < 1.0 and (kind == "small" or np.all(np.abs(h0) <= np.abs(c0)))
    h0, c0 = gu.regime_state("carried", 4096, 64, 1)
    assert 0.999 < np.abs(c0).max() < 1.0 and np.abs(c0.astype(np.float64)).max() <= 0.9995 + 1e-7
    h0, c0 = gu.regime_state("carried", N, 3, 5, tile=4)
    assert np.array_equal(h0[:, :16], h0[:, 48:]) and np.array_equal(c0[:, 16:32], c0[:, 32:48])


def test_saturated_has_the_forget_offset_and_unit_scales_scales_whole_units():
    N = 128
    p = split_params(gu.regime_params("saturated", N, 3), N)
    b = p["b"][:, 0]
    assert abs(b[2 * N:3 * N].mean() - 3.0) < 0.6 and abs(b[:2 * N].mean()) < 0.5 and 2.5 < p["W"].std() < 3.5
    base = split_params(gu.random_case(N, 2, 1, 3, scale=0.08)[0], N)
    p = split_params(gu.regime_params("unit_scales", N, 3), N)
    f = p["Why"][0] / base["Why"][0]                                    # one factor per hidden unit ...
    assert 0.0099 < f.min() < 0.05 and 1.0 < f.max() < 3.01
    for k in ("W", "U", "b"):                                           # ... on the unit's four rows of W, U and b
        np.testing.assert_allclose(p[k], base[k] * np.tile(f, 4)[:, None], rtol=1e-6)
    np.testing.assert_allclose(p["Why"], base["Why"] * f[None, :], rtol=1e-6)
    assert np.array_equal(p["by"], base["by"])


def test_text_windows_are_overlapping_windows_of_the_text():
    text = gu.fixture("A")["text"]
    xi, ti = gu.text_windows(text, 100, 64)
    assert xi.shape == ti.shape == (100, 64) and xi.dtype == ti.dtype == np.int32
    assert np.array_equal(xi[2:], ti[1:-1])                             # target = the next byte
    assert np.array_equal(ti[1:, 0], text[1:100]) and np.array_equal(ti[1:, 63], text[-99:])
    assert xi.min() >= 0 and xi.max() <= 255


@pytest.mark.parametrize("name", ["A", "B"])
def test_tiled_model_has_the_small_models_loss(name, oracle64):
    """The tiling identity at k = 1, 4 and 16: same float64 window loss from the fixture's weights and the tiled ones."""
    fx = gu.fixture(name)
    n, S, B = fx["N"], 40, 6
    xi, ti = gu.text_windows(fx["text"], S, B)
    want = None
    for k in (1, 4, 16):
        P = gu.tile_params(fx["params"], n, k)
        if k == 1:
            assert np.array_equal(P, fx["params"])
        h0, c0 = gu.regime_state("carried", n * k, B, 11, tile=k)
        fw = oracle64.forward(n * k, 256, S, B, P.astype(np.float64), xi, ti, h0, c0)
        if want is None:
            want = fw
        assert abs(fw["loss_bits"] - want["loss_bits"]) <= 1e-10 * want["loss_bits"], (k, fw["loss_bits"], want["loss_bits"])
        np.testing.assert_allclose(fw["h"][:, :, -n:], want["h"], rtol=0, atol=1e-12)      # every block carries the small h
        np.testing.assert_allclose(fw["probs"], want["probs"], rtol=1e-9, atol=0)


def test_block_figures_see_one_column_group_of_dU_gone_wrong():
    case = next(c for c in psc.CASES if c.regime == "tiled_A" and c.shape.N == 128)
    n, k = 32, 4
    rs = np.random.RandomState(0)
    small = rs.randn(gu.fixture("A")["params"].size).astype(np.float32)
    d = gu.tile_params(small, n, k)
    p = split_params(d, 128)
    p["Why"][:] *= k
    assert psc.block_figures(case, d) == dict(blocks_dU=0.0, blocks_dW=0.0)
    p["U"][69, 64:72] *= 1.01                                           # one row over one 8-column group, inside block 2
    assert psc.block_figures(case, d)["blocks_dU"] > 1e-3 and psc.block_figures(case, d)["blocks_dW"] == 0.0


def test_case_table_covers_every_pair_of_forms_and_every_regime():
    pairs = {(sh.plan["fwd"], sh.plan["bwd"]) for sh in psc.SHAPES}
    assert pairs >= {(psc.FWD_TWO_HALF, psc.BWD_SCATTER), (psc.FWD_PERSISTENT, psc.BWD_COLS8), (psc.FWD_COLS8, psc.BWD_COLS8),
                     (psc.FWD_PERSISTENT, psc.BWD_PERSISTENT), (psc.FWD_SMALL, psc.BWD_SMALL), (psc.FWD_STEP, psc.BWD_STEP),
                     (psc.FWD_BF16_HALVES, psc.BWD_BF16_SCATTER), (psc.FWD_BF16, psc.BWD_BF16)}
    assert {sh.forms for sh in psc.SHAPES if sh.every} == set(psc.FAMILIES)
    by_shape = {}
    for c in psc.CASES:
        by_shape.setdefault(psc.SHAPES.index(c.shape), set()).add(c.regime)
    for i, regimes in by_shape.items():
        sh = psc.SHAPES[i]
        assert "saturated" in regimes, sh
        gone = {d[4] for d in psc.DROPPED if d[:4] == (sh.N, sh.S, sh.B, "BF16_RECURRENCE" in sh.flags)}
        assert ("tiled_A" in regimes | gone) == (sh.N % 32 == 0 and "BF16_RECURRENCE" not in sh.flags), sh
        assert "mild" in regimes or "BF16_RECURRENCE" not in sh.flags, sh
        assert (regimes | gone | {"tiled_A"} == set(gu.PARAM_REGIMES)) == sh.every, sh
    assert len({psc.case_id(c) for c in psc.CASES}) == len(psc.CASES)
    assert all(not psc.bf16(c) for c in psc.CONTROL_CASES)
    assert sum(psc.has_update(c) for c in psc.CASES) == 2 * len(psc.FAMILIES)
    assert psc.EXTREME == {k: 4.0 * v for k, v in psc.CONTROL_DISTANCE.items()}


def test_gate_clamp_switched_off_leaves_the_oracle_as_it_was(oracle32):
    N, S, B = 32, 6, 3
    _, xi, ti, h0, c0 = gu.random_case(N, S, B, seed=2)
    P = gu.regime_params("saturated", N, 2)
    before = oracle32.forward(N, 256, S, B, P, xi, ti, h0, c0)
    oracle32.set_gate_clamp(8.0)
    try:
        clamped = oracle32.forward(N, 256, S, B, P, xi, ti, h0, c0)
    finally:
        oracle32.set_gate_clamp(0.0)
    after = oracle32.forward(N, 256, S, B, P, xi, ti, h0, c0)
    assert not np.array_equal(clamped["g"], before["g"])
    for k in ("h", "c", "g", "probs"):
        assert np.array_equal(after[k], before[k]), k
    assert after["loss_bits"] == before["loss_bits"]


@pytest.fixture(scope="module")
def references(request):
    pool = psc.reference_pool(psc.selected_cases(request), "control")
    yield pool
    pool.close()


@pytest.mark.parametrize("case", psc.CONTROL_CASES, ids=psc.case_id)
def test_float32_oracle_meets_a_quarter_of_every_tolerance(case, references):
    r = references.get(case)
    st = r["stats"]
    print(psc.case_id(case), st)
    # the regime, on the float64 reference
    assert st["finite"], "the unshifted softmax of the reference is not finite"
    if case.regime == "saturated":
        assert st["saturated"] >= 0.15, st
    elif psc.tiled(case):
        assert st["p_median"] >= 0.02, st
        assert st["p_max"] >= 0.9 or st["targets"] < 200, st            # (a window of 39 targets need not hold one)
    elif case.regime == "gauss":
        assert st["saturated"] == 0.0 and st["p_max"] < 0.02, st
    psc.check_window(case, r["control"], fraction=0.25)
    # the mutation
    if case.regime == "gauss":
        assert r["clamp_same_bits"], "the clamped oracle differs on Gaussian parameters"
    if case.regime == "saturated":
        assert not r["clamp_same_bits"]
        with pytest.raises(AssertionError):
            psc.check_window(case, r["clamp"], fraction=1.0)
        hit = [k for k, v in psc.tolerances(case).items() if k in r["clamp"] and r["clamp"][k] > v]
        assert {"g", "one_minus_g", "g_small"} <= set(hit), hit


BF16_CASES = [c for c in psc.CASES if psc.bf16(c)]


@pytest.fixture(scope="module")
def bf16_references(request):
    pool = psc.reference_pool(BF16_CASES, False)
    yield pool
    pool.close()


@pytest.mark.parametrize("case", BF16_CASES, ids=psc.case_id)
def test_bf16_cases_are_within_the_cap(case, bf16_references):
    """Every bf16 case's bounds, max(TOL_BF16, 4 x the distance between the two summation orders), are at most 5 x TOL_BF16,
    also by the distance from one float32 spacing of W (param_stats_cases.BF16_CAP); and the oracle summed in descending
    order passes its own case."""
    r = bf16_references.get(case)
    tol = psc.check_window(case, r["dist"], dist=r["dist"], dist_ulp=r["dist_ulp"])
    base = psc.base_tolerances(case)
    assert all(v <= psc.BF16_CAP * base[k] for k, v in tol.items() if k not in psc.EXTREME)
