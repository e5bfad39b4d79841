"""The cases of tests/test_param_statistics.py (-m gpu) and of its reference-only control, tests/test_param_statistics_cpu.py:
one table, one set of inputs, one set of checks, so that the control covers exactly what the GPU file asserts.

A case is one training window (forward, loss, backward; on some rows the update and the window after it) at a shape that puts
the handle on one pair of recurrence forms (csrc/kernels.h), with parameters and a carried state from one of
gpu_util.PARAM_REGIMES.  input_stats_cases.py varies the input bytes over the paths of the gradient sums with parameters from
one Gaussian; this table varies the parameters over the forms of the recurrences: saturated gates, cells at +-0.999, peaked
outputs, weights of order 1-10.  The reference of an fp32 handle is the float64 oracle, of a bf16 handle the float32 oracle in
bf16 mode.  References come from input_stats_cases.ReferencePool (worker processes).

Tolerances.  fp32 handles: the project's (activations 2e-5 of the step's scale, loss 2e-5 bits per step, gradients 2e-4 of
scale), per tensor and per row.  The element-wise bounds at the extremes (EXTREME) are 4 x the largest distance of the float32
oracle from the float64 oracle over the fp32 cases (tests/test_param_statistics_cpu.py records them): the device's v_exp /
v_rcp forms are documented at about 2 ulp against libm's 1, and its summation order is a third order.  bf16 handles: per case
max(TOL_BF16, 4 x the distance between the bf16-mode oracle summed in ascending and in descending order) -- both orders are
correct, and on these regimes they differ by more than TOL_BF16 -- capped at 5 x TOL_BF16 (BF16_CAP).
"""
import collections

import numpy as np

import gpu_util as gu
import input_stats_cases as isc
from input_stats_cases import FWD_STEP, FWD_SMALL, BWD_STEP, BWD_SMALL, BWD_PERSISTENT, BWD_COLS8, BWD_SCATTER, BWD_BF16, \
    BWD_BF16_SCATTER, TOL_FP32, TOL_BF16, parse_plan, assert_plan, selected_cases  # noqa: F401  (the GPU file uses them)
from oracle_lib import split_params

FWD_PERSISTENT, FWD_COLS8, FWD_TWO_HALF, FWD_BF16, FWD_BF16_HALVES = 2, 3, 4, 5, 6
HALVES_OFF = {"LSTM_HIP_FWD_HALVES": "0", "LSTM_HIP_BWD_HALVES": "0"}

Shape = collections.namedtuple("Shape", "forms N S B flags env plan every")
# forms: the row of the table; plan: what lstm_hip_plan_identity must say on the device at hand (256 CUs); every: all regimes
# (one row per family), and the update step with the window after it.
SHAPES = [
    Shape("TwoHalf / Scatter, fused", 512, 100, 64, (), {}, dict(fwd=FWD_TWO_HALF, bwd=BWD_SCATTER, fused=1, gc=8, lc=64), False),
    Shape("TwoHalf / Scatter, 4-column pinned groups", 512, 12, 24, (), {}, dict(fwd=FWD_TWO_HALF, bwd=BWD_SCATTER, fused=1, gc=4, gp=4), True),
    Shape("TwoHalf / Scatter, several launches", 256, 10, 272, (), {}, dict(fwd=FWD_TWO_HALF, bwd=BWD_SCATTER, fused=1, gc=8, lc=128), False),
    Shape("Persistent / Cols8, fused", 128, 25, 16, (), {}, dict(fwd=FWD_PERSISTENT, bwd=BWD_COLS8, fused=1, bc=8), True),
    Shape("Cols8 / Cols8, fused, halves off", 512, 9, 64, (), HALVES_OFF, dict(fwd=FWD_COLS8, bwd=BWD_COLS8, fused=1, bc=8), False),
    Shape("TwoHalf / unfused Scatter on the side stream", 256, 100, 64, ("NO_FUSED_GRADS",), {}, dict(fwd=FWD_TWO_HALF, bwd=BWD_SCATTER, fused=0, side=1), False),
    Shape("Cols8 / Cols8, unfused", 1024, 100, 16, (), {}, dict(fwd=FWD_COLS8, bwd=BWD_COLS8, fused=0), False),
    Shape("Persistent / Persistent, 16-column backward groups", 128, 70, 264, (), {}, dict(fwd=FWD_PERSISTENT, bwd=BWD_PERSISTENT, fused=0, bc=16), False),
    Shape("Small / Small", 128, 301, 1, (), {}, dict(fwd=FWD_SMALL, bwd=BWD_SMALL, fused=0), True),
    # (the sweep's (64, 9, 1) has eight columns: a dW row of a saturated unit is then the sum of a few terms of 1e-6 of the
    # tensor's scale, and the float32 oracle's own rows are off by 1.7e-4 of theirs; with 39 columns by 9.4e-6)
    Shape("Small / Small", 64, 40, 1, (), {}, dict(fwd=FWD_SMALL, bwd=BWD_SMALL, fused=0), False),
    Shape("Step / Step", 64, 130, 130, ("STEP_KERNELS",), {}, dict(fwd=FWD_STEP, bwd=BWD_STEP, fused=0), True),
    # bf16 rows: windows of at most 12 steps and `mild` in place of tiled_A, see BF16_CAP
    Shape("Bf16Halves / Bf16Scatter, direct dg image", 1024, 12, 16, ("BF16_RECURRENCE",), {}, dict(fwd=FWD_BF16_HALVES, bwd=BWD_BF16_SCATTER, dgt=1), False),
    Shape("Bf16Halves / Bf16Scatter, several launches", 256, 10, 272, ("BF16_RECURRENCE",), {}, dict(fwd=FWD_BF16_HALVES, bwd=BWD_BF16_SCATTER, dgt=0), False),
    Shape("Bf16Halves / Bf16Scatter", 512, 12, 64, ("BF16_RECURRENCE",), {}, dict(fwd=FWD_BF16_HALVES, bwd=BWD_BF16_SCATTER), True),
    Shape("Bf16 / Bf16, halves off", 256, 10, 64, ("BF16_RECURRENCE",), HALVES_OFF, dict(fwd=FWD_BF16, bwd=BWD_BF16), False),
    # padded widths: 500 and 100 are no multiple of a fixture's hidden size, so the synthetic regimes only
    Shape("padded, TwoHalf / Scatter", 500, 7, 64, ("PAD_HIDDEN",), {}, dict(np=512, fwd=FWD_TWO_HALF, bwd=BWD_SCATTER, fused=1), False),
    Shape("padded, Persistent / Cols8", 100, 24, 16, ("PAD_HIDDEN",), {}, dict(np=128, fwd=FWD_PERSISTENT, bwd=BWD_COLS8, fused=1), False),
    Shape("stable softmax, TwoHalf / Scatter", 512, 12, 24, ("STABLE_SOFTMAX",), {}, dict(fwd=FWD_TWO_HALF, bwd=BWD_SCATTER, fused=1, gc=4), False),
    Shape("stable softmax, Persistent / Cols8", 128, 25, 16, ("STABLE_SOFTMAX",), {}, dict(fwd=FWD_PERSISTENT, bwd=BWD_COLS8, fused=1), False),
    Shape("fast math, Persistent", 128, 25, 16, ("FAST_MATH",), {}, dict(fwd=FWD_PERSISTENT, bwd=BWD_COLS8, fused=1), False),
    Shape("fast math, Step", 64, 130, 130, ("STEP_KERNELS", "FAST_MATH"), {}, dict(fwd=FWD_STEP, bwd=BWD_STEP), False),
]
FAMILIES = ("TwoHalf / Scatter, 4-column pinned groups", "Persistent / Cols8, fused", "Small / Small", "Step / Step",
            "Bf16Halves / Bf16Scatter")   # the rows marked `every`: fp32 two-half, fp32 one-recurrence, small, step, bf16

Case = collections.namedtuple("Case", "shape regime")
UPDATE_REGIMES = ("saturated", "tiled_A")
UPDATE_REGIMES_BF16 = ("saturated", "mild")
UPDATE_LR = 0.01
# The control (the float32 oracle through the same checks at a quarter of every tolerance) runs where (S-1) * B * N^2 is at
# most this (the serial oracle needs about 20 s for both precisions at the headline shape, 1.7e9); the larger fp32 cases'
# control figures are computed beside their references by the GPU file and recorded in profiles/param_statistics.
CONTROL_MAX_WORK = 5e8


def bf16(case):
    return "BF16_RECURRENCE" in case.shape.flags


def fast_math(case):
    return "FAST_MATH" in case.shape.flags


def tiled(case):
    return case.regime.startswith("tiled_")


def has_update(case):
    return case.shape.every and case.regime in (UPDATE_REGIMES_BF16 if bf16(case) else UPDATE_REGIMES)


def work(case):
    sh = case.shape
    return (sh.S - 1) * sh.B * sh.N * sh.N


# Cases the control sent away: their float32 oracle does not stay within a quarter of the activation tolerance (5e-6) on
# probs, so the tolerance would sit inside float32 rounding.  The fixtures' logits reach 20, and p follows a logit's absolute
# error: ascending float32 sums of 1024 terms at hidden 1024 (probs 7.4e-6 at S = 100, 1.3e-5 at 50, 7.1e-6 at 25), fixture
# B's sharper model (p up to 1 - 8e-8) at (512, 12, 24) 5.4e-6 and at (64, 130, 130) 7.0e-6.  tiled_A stays on every other
# row, tiled_B on the one-recurrence, the small and the bf16 row.
DROPPED = {(1024, 100, 16, False, "tiled_A"), (512, 12, 24, False, "tiled_B"), (64, 130, 130, False, "tiled_B")}


def _cases():
    out = []
    for sh in SHAPES:
        second = "mild" if "BF16_RECURRENCE" in sh.flags else "tiled_A"
        regimes = ["saturated", second] + ([r for r in gu.PARAM_REGIMES if r not in ("saturated", second, "tiled_A")] if sh.every else [])
        for r in regimes:
            if r.startswith("tiled_") and sh.N % gu.fixture(r[-1])["N"] != 0:
                continue
            if (sh.N, sh.S, sh.B, "BF16_RECURRENCE" in sh.flags, r) in DROPPED:
                continue
            out.append(Case(sh, r))
    return out


CASES = _cases()
FP32_CASES = [c for c in CASES if not bf16(c) and not fast_math(c)]
CONTROL_CASES = [c for c in FP32_CASES if work(c) <= CONTROL_MAX_WORK and not c.shape.env and
                 "STABLE_SOFTMAX" not in c.shape.flags]     # (the oracle has one softmax and no forms: one control per input)


def case_id(case):
    sh = case.shape
    tag = "".join("-" + f.lower() for f in sh.flags) + "".join(f"-{k[9:].lower()}{v}" for k, v in sh.env.items())
    return f"{sh.N}x{sh.S}x{sh.B}{tag}-{case.regime}"


def input_id(case):
    """Cases with one input_id have the same inputs and the same reference (flags that do not change what is computed)."""
    sh = case.shape
    return f"{sh.N}x{sh.S}x{sh.B}-{case.regime}" + ("-bf16" if bf16(case) else "")


def inputs(case):
    """P, xi, ti, h0, c0 of a case.  Synthetic regimes: text-distributed input bytes with uniform targets; tiled_*: the
    fixture's own held-out text as overlapping windows, target = the next byte.  State: `carried` with saturated and
    tiled_* (tiled like the parameters), `small` otherwise."""
    sh = case.shape
    seed = sh.N + 3 * sh.S + 7 * sh.B + 13 * gu.PARAM_REGIMES.index(case.regime)
    scale = (0.05 if sh.N <= 256 else 0.02) if bf16(case) else (0.08 if sh.N <= 256 else 0.02)
    P = gu.regime_params(case.regime, sh.N, seed, scale=scale)
    if tiled(case):
        fx = gu.fixture(case.regime[-1])
        xi, ti = gu.text_windows(fx["text"], sh.S, sh.B)
        h0, c0 = gu.regime_state("carried", sh.N, sh.B, seed, tile=sh.N // fx["N"])
    else:
        xi, ti = gu.window_bytes("text", sh.S, sh.B, seed, "uniform")
        h0, c0 = gu.regime_state("carried" if case.regime == "saturated" else "small", sh.N, sh.B, seed)
    return P, xi, ti, h0, c0


def update_memory(case, d_ref):
    """The Adagrad memory before the update step: (d_ref^2 + max|d_ref|^2 of the tensor) * U(1, 50).  The step
    lr * d / sqrt(m + d^2) is then smooth in d (the first step from m = 0 is +-lr and flips with the sign of a gradient that is
    noise), and its slope is at most lr / max|d_ref|: a gradient within tol of its tensor's scale gives a step within tol * lr,
    for every element, so that nothing has to be masked."""
    sh = case.shape
    d = np.asarray(d_ref, np.float64)
    top = np.concatenate([np.full(v.size, np.abs(v).max()) for v in split_params(d, sh.N).values()])
    u = np.random.RandomState(sh.N + sh.S + sh.B).uniform(1.0, 50.0, d.size)
    return ((d * d + top * top) * u).astype(np.float32)


# ---- the references, in worker processes --------------------------------------------------------------------------------
def _window(orc, sh, P, xi, ti, h0, c0):
    fw = orc.forward(sh.N, 256, sh.S, sh.B, P, xi, ti, h0, c0)
    d = orc.backward(sh.N, 256, sh.S, sh.B, P, xi, ti, fw)
    return dict(h=fw["h"][1:], c=fw["c"][1:], g=fw["g"][1:], probs=fw["probs"][1:], loss=fw["loss_bits"], grads=d)


def _update(orc, case, P, xi, ti, h0, c0, d, mem0, restate):
    """The update step and the window after it.  restate: the float64 restatement of Adagrad (R/lstm.cc:261-272) on d, the
    reference; otherwise the oracle's own ref_adagrad in its precision."""
    sh = case.shape
    if restate:
        d64 = np.asarray(d, np.float64)
        m = mem0.astype(np.float64) + d64 * d64
        p = np.asarray(P, np.float64) - UPDATE_LR * d64 / np.sqrt(m + 1e-10)
    else:
        p, m = np.array(P, orc.np_t), mem0.astype(orc.np_t)
        orc.adagrad(p, np.asarray(d, orc.np_t), m, UPDATE_LR)
    fw = orc.forward(sh.N, 256, sh.S, sh.B, p.astype(orc.np_t), xi, ti, h0, c0)
    return dict(p=p, m=m, h_last=fw["h"][sh.S - 1].copy(), loss=fw["loss_bits"])


def reference(case, mode=False):
    """The case's reference, computed in a worker: dict(ref, upd, mem0, and per mode).  fp32 cases: ref from the float64
    oracle; mode True adds control = figures(float32 oracle, ref); mode "control" returns the control's figures only (no
    arrays), with the gate-clamp mutation's on `saturated` and `gauss` cases.  bf16 cases: ref from the float32 oracle in
    bf16 mode, dist = figures(the same summed in descending order, ref), dist_ulp = figures(the same from W one float32
    spacing up, ref)."""
    from oracle_lib import Oracle
    sh = case.shape
    P, xi, ti, h0, c0 = inputs(case)
    out = dict(upd=None, mem0=None, control=None, dist=None, dist_ulp=None)
    o32 = Oracle("f32")
    if bf16(case):
        o32.set_bf16_recurrence(True)
        o32.set_bf16_products(True)
        try:
            ref = _window(o32, sh, P, xi, ti, h0, c0)
            if has_update(case):
                out["mem0"] = update_memory(case, ref["grads"])
                out["upd"] = _update(o32, case, P, xi, ti, h0, c0, ref["grads"], out["mem0"], True)
            o32.set_descending_sums(True)
            alt = _window(o32, sh, P, xi, ti, h0, c0)
            out["dist"] = figures(case, alt, ref, ti)
            o32.set_descending_sums(False)
            W = 4 * sh.N * 256
            P1 = P.copy()
            P1[:W] = np.nextafter(P1[:W], np.float32(np.inf))
            out["dist_ulp"] = figures(case, _window(o32, sh, P1, xi, ti, h0, c0), ref, ti)
            if has_update(case):
                out["dist"].update(update_figures(_update(o32, case, P, xi, ti, h0, c0, alt["grads"], out["mem0"], True), out["upd"]))
        finally:
            o32.set_descending_sums(False)
            o32.set_bf16_recurrence(False)
            o32.set_bf16_products(False)
        out["ref"] = ref
        return out
    o64 = Oracle("f64")
    ref = _window(o64, sh, P.astype(np.float64), xi, ti, h0, c0)
    if has_update(case):
        out["mem0"] = update_memory(case, ref["grads"])
        out["upd"] = _update(o64, case, P, xi, ti, h0, c0, ref["grads"], out["mem0"], True)
    if mode:
        r32 = _window(o32, sh, P, xi, ti, h0, c0)
        out["control"] = figures(case, r32, ref, ti)
        if has_update(case):
            out["control"].update(update_figures(_update(o32, case, P, xi, ti, h0, c0, r32["grads"], out["mem0"], False), out["upd"]))
    if mode == "control":
        out["stats"] = regime_stats(case, ref, ti)
        if case.regime in ("saturated", "gauss"):
            o32.set_gate_clamp(GATE_CLAMP)
            try:
                mut = _window(o32, sh, P, xi, ti, h0, c0)
            finally:
                o32.set_gate_clamp(0.0)
            out["clamp_same_bits"] = all(np.array_equal(np.asarray(mut[k]), np.asarray(r32[k])) for k in r32)
            out["clamp"] = figures(case, mut, ref, ti)
        return out
    out["ref"] = ref
    return out


GATE_CLAMP = 8.0   # the mutation of the control: gate pre-activations clamped to +-8 (oracle/lstm_ref.c, ref_set_gate_clamp)


def reference_pool(cases, mode=False):
    return isc.ReferencePool(cases, mode, fn=reference, key=input_id)


# ---- the checks ---------------------------------------------------------------------------------------------------------
# Below 1 - g = 2^-14 (and 1 - |c|) the spacing of float32 at g, 2^-24 or 2^-25, is itself above 5e-4 of 1 - g: a bound on
# the relative error of 1 - g there would be a statement about float32, not about a kernel.  Those elements are measured
# against the floor, which still sees a gate clamped at +-8 (1 - g = 3.4e-4 where it should be 1e-6: 5 floors off).
ONE_MINUS_FLOOR = 2.0 ** -14
# A stored cell is tanh(i * u + f * c_prev) with all four factors inside (-1, 1), so past the carried state |c| stays below
# tanh(2) = 0.964: "the cells near 1" are those above 0.9, not above 0.99 as for a gate.
C_LARGE = 0.9
# Element-wise at the extremes: 4 x the float32 oracle's largest distance from the float64 oracle over the fp32 cases
# (CONTROL_DISTANCE; tests/test_param_statistics_cpu.py asserts that no case is above it, the GPU file does so for the four
# inputs too large for that file, beside their references).
# Largest over the 37 fp32 inputs: g_small 7.4e-6 (128x25x16 tiled_B), one_minus_g 1.04e-3 (every saturated case: the float32
# spacing of g against the floor), one_minus_c 3.8e-6 (1024x100x16 saturated), p_target 1.5e-5 (512x12x24 tiled_A); rounded up.
CONTROL_DISTANCE = dict(g_small=7.5e-6, one_minus_g=1.1e-3, one_minus_c=3.9e-6, p_target=1.6e-5)
EXTREME = {k: 4.0 * v for k, v in CONTROL_DISTANCE.items()}
# A bf16 bound above BF16_CAP x its TOL_BF16 value means that the case is ill-conditioned for bf16, and the case is replaced
# (a shorter window, a milder regime).  The distance between the two summation orders alone does not tell: where U is block-
# diagonal with 16 or 32 non-zero terms per row (tiled_*), the products of two bf16 operands have 16-bit significands and
# their float32 sums are mostly exact in either order, so that the orders agree to 3e-7 over 11 steps -- while the same oracle
# with W one float32 spacing up (the second control of tests/trajectory_util.py) is 3.8e-3 of scale away in h, the size of
# one bf16 rounding of an h that falls the other way times a trained recurrent weight.  So the cap also looks at that
# distance, dist_ulp; the bound itself stays max(TOL_BF16, 4 x the order distance).  What the cap sent away, float32 oracle in
# bf16 mode, h / c / g of scale: saturated at (1024, 100, 16) 2.8e-3 / 3.3e-3 / 3.2e-3 between the orders, at (256, 100, 272)
# 3.3e-3 / 3.9e-3 / 4.2e-3, still 2.9e-3 in c at (1024, 20, 16) and 3.9e-3 in g at (256, 20, 272) -- the bf16 rows have at most
# 12 steps, and (256, 12, 64) saturated, 2.5e-3 in g from one spacing of W, has 10; tiled_A at (512, 12, 64) and (256, 12, 64)
# 3.7e-3 and 3.8e-3 from one spacing of W -- the bf16 rows take `mild`.
BF16_CAP = 5.0
FAST_MATH_TOL = 1e-4      # forward and loss of an LSTM_HIP_FAST_MATH handle (tests/test_hip_parity.py)
ACT = ("h", "c", "g", "probs")
GRAD = ("dW", "dU", "db", "dWhy", "dby", "dW_row", "dU_row", "dWhy_col")
BLOCKS = ("blocks_dU", "blocks_dW")


def _per_step(a, b):
    """max over the steps of max|a[t] - b[t]| / max|b[t]|, and the step it is at"""
    n = a.shape[0]
    a, b = np.asarray(a, np.float64).reshape(n, -1), np.asarray(b, np.float64).reshape(n, -1)
    e = np.abs(a - b).max(axis=1) / np.maximum(np.abs(b).max(axis=1), 1e-30)
    return float(e.max()), int(np.argmax(e)) + 1


def _worst(e):
    return float(e.max()) if e.size else 0.0


def _rows(a, b, axis):
    """max over the rows of max|a - b| / max|b| of the row (axis: the one reduced inside a row); a row of zeros in b counts
    by the tensor's scale"""
    scale = np.abs(b).max(axis=axis)
    scale = np.where(scale > 0, scale, max(np.abs(b).max(), 1e-30))
    return float((np.abs(a - b).max(axis=axis) / scale).max())


def block_figures(case, grads):
    """tiled cases: the k diagonal blocks of dU against the first, the k row-copies of dW against the first (of its scale).
    Needs no reference."""
    sh = case.shape
    n = gu.fixture(case.regime[-1])["N"]
    k = sh.N // n
    if k == 1:
        return dict(blocks_dU=0.0, blocks_dW=0.0)
    p = split_params(np.asarray(grads, np.float64), sh.N)
    U = p["U"].T.reshape(k, n, 4, k, n)                 # [column block, column, gate, row block, row]
    dU = max(np.abs(U[c, :, :, c, :] - U[0, :, :, 0, :]).max() for c in range(1, k)) / max(np.abs(U[0, :, :, 0, :]).max(), 1e-30)
    W = p["W"].T.reshape(256, 4, k, n)
    dW = np.abs(W[:, :, 1:, :] - W[:, :, :1, :]).max() / max(np.abs(W[:, :, 0, :]).max(), 1e-30)
    return dict(blocks_dU=float(dU), blocks_dW=float(dW))


def figures(case, got, ref, ti):
    """Every figure of a window dict(h, c, g, probs: [S-1, B, rows] for t = 1..S-1; loss; grads) against the reference's."""
    sh = case.shape
    N = sh.N
    f = {}
    for k in ACT:                                                               # every step, of the step's scale
        f[k], f[k + "_t"] = _per_step(got[k], ref[k])
    # element-wise at the extremes
    g, gr = np.asarray(got["g"][..., :3 * N], np.float64), np.asarray(ref["g"][..., :3 * N], np.float64)
    lo, hi = gr < 0.01, gr > 0.99
    f["g_small"] = _worst(np.abs(g[lo] - gr[lo]) / np.maximum(gr[lo], 1e-30))
    f["one_minus_g"] = _worst(np.abs(g[hi] - gr[hi]) / np.maximum(1.0 - gr[hi], ONE_MINUS_FLOOR))
    c, cr = np.abs(np.asarray(got["c"], np.float64)), np.abs(np.asarray(ref["c"], np.float64))
    big = cr > C_LARGE
    f["one_minus_c"] = _worst(np.abs(c[big] - cr[big]) / np.maximum(1.0 - cr[big], ONE_MINUS_FLOOR))
    t = np.asarray(ti)[1:]
    pt = np.take_along_axis(np.asarray(got["probs"], np.float64), np.maximum(t, 0)[..., None], axis=2)[..., 0][t >= 0]
    ptr = np.take_along_axis(np.asarray(ref["probs"], np.float64), np.maximum(t, 0)[..., None], axis=2)[..., 0][t >= 0]
    f["p_target"] = _worst(np.abs(pt - ptr) / np.maximum(ptr, 1e-300))
    f["loss"] = abs(got["loss"] - ref["loss"])
    # gradients: per tensor, per row of dW and dU (one gate unit), per column of dWhy (one hidden unit)
    a, b = split_params(np.asarray(got["grads"], np.float64), N), split_params(np.asarray(ref["grads"], np.float64), N)
    for k in a:
        f["d" + k] = gu.max_rel(a[k], b[k])
    f["dW_row"], f["dU_row"] = _rows(a["W"], b["W"], 1), _rows(a["U"], b["U"], 1)
    f["dWhy_col"] = _rows(a["Why"], b["Why"], 0)
    if tiled(case):
        f.update(block_figures(case, got["grads"]))
    return f


def update_figures(got, ref):
    """dict(p, m, h_last, loss) after the update step against the reference's.  p: |d| beyond half a float32 spacing of the
    weight (the device stores float32), in units of UPDATE_LR; m: |d| beyond 1e-3 relative, of max m."""
    p, pr = np.asarray(got["p"], np.float64), np.asarray(ref["p"], np.float64)
    m, mr = np.asarray(got["m"], np.float64), np.asarray(ref["m"], np.float64)
    half = 0.5 * np.spacing(np.abs(pr).astype(np.float32)).astype(np.float64)
    return dict(upd_p=float(np.maximum(np.abs(p - pr) - half, 0.0).max() / UPDATE_LR),
                upd_m=float(np.maximum(np.abs(m - mr) - 1e-3 * np.abs(mr), 0.0).max() / mr.max()),
                upd_h=gu.max_rel(got["h_last"], ref["h_last"]), upd_loss=abs(got["loss"] - ref["loss"]))


def regime_stats(case, ref, ti):
    """What the regime assertions of the control look at, on the float64 reference."""
    gr = np.asarray(ref["g"][..., :3 * case.shape.N])
    t = np.asarray(ti)[1:]
    pt = np.take_along_axis(np.asarray(ref["probs"]), np.maximum(t, 0)[..., None], axis=2)[..., 0][t >= 0]
    return dict(saturated=float(np.mean((gr < 0.01) | (gr > 0.99))), c_max=float(np.abs(ref["c"]).max()), targets=int(pt.size),
                p_min=float(pt.min()), p_median=float(np.median(pt)), p_max=float(pt.max()),
                finite=bool(np.isfinite(ref["probs"]).all() and np.isfinite(ref["loss"])))


def tolerances(case, dist=None):
    """figure -> bound.  fp32: the project's tolerances and EXTREME.  bf16: max(base, 4 x dist[figure]) with base TOL_BF16
    (at the extremes that of the activations: the relative error of a small gate, of 1 - g or of a probability is the
    absolute error of its pre-activation or logit); BF16_CAP is asserted by check_window."""
    S1 = case.shape.S - 1
    if fast_math(case):
        tol = {k: FAST_MATH_TOL for k in ACT}
        tol["loss"] = FAST_MATH_TOL * S1
        return tol
    base = TOL_BF16 if bf16(case) else TOL_FP32
    tol = {k: base["h"] for k in ACT + ("upd_h",)}
    tol.update({k: base["grad"] for k in GRAD + BLOCKS + ("upd_p",)})
    tol.update(loss=base["loss"] * S1, upd_loss=base["loss"] * S1, upd_m=1e-3)
    tol.update({k: base["h"] if bf16(case) else v for k, v in EXTREME.items()})
    if bf16(case):
        assert dist is not None
        tol = {k: max(v, 4.0 * dist.get(k, 0.0)) for k, v in tol.items()}
    return tol


def base_tolerances(case):
    return tolerances(case, {}) if bf16(case) else tolerances(case)


def check_window(case, fig, fraction=1.0, dist=None, dist_ulp=None):
    """Asserts every figure of a case (figures(), and update_figures() where the case has an update step) against its bound
    times fraction (the control runs the float32 oracle through this with 0.25).  Prints the figures first; returns the
    bounds used."""
    tol = tolerances(case, dist)
    print(case_id(case), " ".join(f"{k}={v:.2e}" if isinstance(v, float) else f"{k}={v}" for k, v in fig.items()))
    if bf16(case):
        base = base_tolerances(case)
        over = {k: (dist.get(k, 0.0), dist_ulp.get(k, 0.0), v) for k, v in base.items()    # (the extremes have no TOL_BF16 value)
                if k not in EXTREME and 4.0 * max(dist.get(k, 0.0), dist_ulp.get(k, 0.0)) > BF16_CAP * v}
        assert not over, f"ill-conditioned for bf16 (order distance, one-spacing distance, base), replace the case: {over}"
    missing = [k for k in tol if k not in fig and not k.startswith("upd_") and k not in BLOCKS]
    assert not missing, missing
    assert tiled(case) == ("blocks_dU" in fig), "the block relation's figures"
    off = {k: (fig[k], tol[k] * fraction) for k in tol if k in fig and not fig[k] <= tol[k] * fraction}
    assert not off, f"{case_id(case)} (figure, bound): {off}"
    return tol
