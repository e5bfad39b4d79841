"""The cases of tests/test_hidden_widths.py (-m gpu) and of its reference-only control, tests/test_hidden_widths_cpu.py: one
table, one set of inputs, one set of checks, so that the control covers exactly what the GPU file asserts.

plan_engine (csrc/persistent.hip) gives an fp32 handle a persistent recurrence at hidden 64, 128, 256, 512 and 1024 only, and
there only where the grid is co-resident.  Every other width -- 192, 320, 768, everything above 1024, a padded 30 or 1030 --
trains, evaluates and samples on the per-step engine (FwdForm::Step / BwdForm::Step: k_fwd_step and k_bwd_step per time
step, the gemm.hip products, k_eval_bits and k_sample), which the other suites run at hidden 16 to 128 and once at 512.  A
case here is one training window (forward, loss, backward, one Adagrad step) at a width the plan itself puts on that engine:
no case passes LSTM_HIP_STEP_KERNELS, every case asserts the plan.  The reference is the float64 oracle, from
input_stats_cases.ReferencePool (worker processes); the tolerances are the project's (input_stats_cases.TOL_FP32).

The evaluator's and the sampler's cases (EVAL, SAMPLE) are here too, with the LDS request of their one-workgroup kernels.
"""
import collections

import numpy as np

import gpu_util as gu
import input_stats_cases as isc
from oracle_lib import split_params
from input_stats_cases import FWD_STEP, BWD_STEP, TOL_FP32, ReferencePool, assert_plan, check_window, selected_cases  # noqa: F401

CH = 8                                   # k-steps of 16 per operand chunk of k_fwd_step and k_bwd_step (csrc/kernels.hip)
PERSISTENT_WIDTHS = (64, 128, 256, 512, 1024)   # the widths with_fwd_persistent and with_bwd_persistent resolve (csrc/persistent.hip)
STEP = dict(fwd=FWD_STEP, bwd=BWD_STEP)
LR = 0.1                                 # the Adagrad step of every case, as test_hip_parity.py::test_window_matches_oracle


def _shape(what, N, S, B, flags=(), np_=None):
    plan = dict(STEP, np=np_) if np_ else dict(STEP)
    # (the fields of input_stats_cases.Shape that its check_window and case_id read; dw and launches are not used here)
    return isc.Shape(what, N, S, B, flags, {}, plan, None, S - 1, False)


# what: what only this case reaches.  k-steps: Np / 16 (both step kernels walk them in chunks of CH, the backward kernel
# per wave); the products of gemm.hip have M = 4 Np or 256 rows, Nn = Np or T = (S - 1) B columns.
SHAPES = [
    _shape("5 k-steps; M = 320 is 2.5 tiles of 128 and Nn = 80 is 1.25 of 64; T = 531: split-K by 2 with a 3-wide k tail, "
           "the last column tile has 11 columns", 80, 10, 59),
    _shape("12 k-steps: one full chunk and a partial one of 4; a multiple of 64 without a persistent instantiation; the "
           "batch is one column past a tile", 192, 3, 17),
    _shape("20 k-steps: two full chunks and a partial one; 4N = 1280 > 1024", 320, 5, 40),
    _shape("first width above 1024: 65 k-steps, eight full chunks and one more", 1040, 3, 5),
    _shape("largest width: every chunk full, 16 times the depth of any other step-engine test", 2048, 3, 3),
    _shape("a persistent width planned onto the per-step engine (no co-resident grid on 256 CUs)", 1024, 3, 40),
    _shape("padded to 1040 on the per-step engine; reference at logical N", 1030, 3, 5, ("PAD_HIDDEN",), 1040),
    _shape("padded to 32", 30, 4, 9, ("PAD_HIDDEN",), 32),
]
CASES = [isc.Case(sh, "uniform", "uniform") for sh in SHAPES]


def internal_width(sh):
    return sh.plan.get("np", sh.N)


def k_steps(sh):
    return internal_width(sh) // 16


def case_id(case):
    sh = case.shape
    return f"{sh.N}x{sh.S}x{sh.B}" + "".join("-" + f.lower() for f in sh.flags)


def inputs(case):
    """P, xi, ti, h0, c0: gu.random_case with scale 0.08 up to hidden 256 and 0.02 above, one empty column at step 1."""
    sh = case.shape
    empty = ((1, sh.B // 2),) if sh.S > 2 else ()
    return gu.random_case(sh.N, sh.S, sh.B, seed=sh.N + sh.S + sh.B, scale=0.08 if sh.N <= 256 else 0.02, empty=empty)


# ---- the references, in worker processes --------------------------------------------------------------------------------
def _window(orc, sh, P, xi, ti, h0, c0):
    """One window and one Adagrad step from m = 0 in the oracle's precision.  The stepped parameters and the memory travel
    as float32 (what the device stores; the blocks of hidden 2048 have 19 million entries)."""
    P = np.ascontiguousarray(P, orc.np_t)
    fw = orc.forward(sh.N, 256, sh.S, sh.B, P, xi, ti, h0, c0)
    d = orc.backward(sh.N, 256, sh.S, sh.B, P, xi, ti, fw)
    p, m = P.copy(), np.zeros_like(P)
    orc.adagrad(p, d.copy(), m, LR)
    out = {k: fw[k][1:].copy() for k in ("h", "c", "g", "probs")}
    out.update(h_last=fw["h"][sh.S - 1].copy(), loss=fw["loss_bits"], grads=d, params=p.astype(np.float32), mem=m.astype(np.float32))
    return out


def drop_last_k_step(P, N):
    """The parameters with the last 16 columns of U zeroed: the window a recurrence that dropped its final k-step computes."""
    P = np.array(P, np.float32)
    split_params(P, N)["U"][:, N - 16:] = 0.0   # (a view: [4N, N], column k multiplies h[k])
    return P


def reference(case, mode=False):
    """The float64 oracle's window.  mode "control": no arrays but what the control asserts, computed in the worker --
    dict(fig: check_case's figures of the float32 oracle at a quarter of every tolerance (a miss raises here and in the
    test), mutant: the first assertion that the float32 oracle without its last k-step fails at the full tolerances, or
    None, mutant_act: its activation figures)."""
    from oracle_lib import Oracle
    sh = case.shape
    P, xi, ti, h0, c0 = inputs(case)
    ref = _window(Oracle("f64"), sh, P, xi, ti, h0, c0)
    if mode != "control":
        return ref
    o32 = Oracle("f32")
    out = dict(fig=check_case(case, _window(o32, sh, P, xi, ti, h0, c0), ref, xi, 0.25), mutant=None)
    mut = _window(o32, sh, drop_last_k_step(P, sh.N), xi, ti, h0, c0)
    out["mutant_act"] = act_figures(case, mut, ref)
    try:
        check_case(case, mut, ref, xi)
    except AssertionError as e:
        out["mutant"] = str(e)[:300]
    return out


# ---- the checks ---------------------------------------------------------------------------------------------------------
def act_figures(case, got, ref):
    """h, c, g and probs: the largest distance over the steps, each of its step's scale"""
    return {k: max(gu.max_rel(got[k][t], ref[k][t]) for t in range(case.shape.S - 1)) for k in ("h", "c", "g", "probs")}


def check_case(case, got, ref, xi, fraction=1.0):
    """Every assertion of a case on dict(h, c, g, probs: [S-1, B, rows] for t = 1..S-1; h_last, loss, grads, params, mem)
    against the reference; fraction scales every tolerance (the control runs the float32 oracle through this with 0.25).
    Prints the figures, then asserts; returns them."""
    fig = act_figures(case, got, ref)
    d = np.asarray(ref["grads"], np.float64)
    # Adagrad: first step from m = 0.  Entries whose gradient is about 0 may flip sign (p moves by +-lr either way), so
    # compare where |d| is well above the gradient noise (test_hip_parity.py::test_window_matches_oracle).
    mask = np.abs(d) > 1e-3 * np.abs(d).max()
    fig["upd_p"] = float(np.abs(got["params"].astype(np.float64)[mask] - ref["params"].astype(np.float64)[mask]).max())
    m, mr = got["mem"].astype(np.float64), ref["mem"].astype(np.float64)
    fig["upd_m"] = float(np.maximum(np.abs(m - mr) - 1e-3 * fraction * np.abs(mr), 0.0).max() / mr.max())
    print(case_id(case), " ".join(f"{k}={v:.2e}" for k, v in fig.items()))
    for k in ("h", "c", "g", "probs"):
        assert fig[k] <= TOL_FP32["h"] * fraction, (k, fig)
    fig.update({k: v for k, v in check_window(case, got, ref, xi, fraction).items() if k != "h"})   # (its h: the last step's)
    assert fig["upd_p"] <= (2e-4 * LR + 1e-6) * fraction, fig
    assert fig["upd_m"] <= 1e-3 * fraction, fig       # |m - mr| <= rtol |mr| + atol max(mr), rtol = atol = 1e-3
    return fig


# ---- the device loop ----------------------------------------------------------------------------------------------------
# (N, S, B, windows, learning rate) of train_windows in lock step with the oracle's trainer, with the assertions of
# test_hip_parity.py::test_device_resident_loop_follows_the_oracle_trainer (loss 2e-5 (S-1), carry 2e-5, parameters after the
# step 2e-4 lr + 1e-6 where the gradient is above noise).  Hidden 1040 runs at 0.01: at that test's 0.1 the first steps
# move all 5.4 million weights by 0.1 each, the window's loss goes from 8 to 94 bits, and from the same state the float32
# oracle's own step is 1.8e-5, 1.9e-5 and 2.5e-5 away from the float64 oracle's in windows 3, 4 and 8, where 2.1e-5 is allowed
# (an MI355X: 2.9e-5 in window 8).  At 0.01 the float32 oracle stays within 1.4e-7 of 3e-6, and (192, 6, 17) at 0.1 within
# 2.4e-6 of 2.1e-5 (the control: tests/test_hidden_widths_cpu.py).
LOOPS = [(192, 6, 17, 25, 0.1), (1040, 4, 5, 10, 0.01)]


# ---- evaluator and sampler ----------------------------------------------------------------------------------------------
# k_eval_bits / k_sample: one workgroup of 1024 threads, h, c, the gates and the outputs in dynamic LDS.  b1_step's row loop
# makes a second pass when 4N > 1024 (320), its j < N loop when N > 1024 (1040); the request passes 64 KB -- what a launch is
# granted unasked -- between 2688 and 2704; gfx950 has 160 KB per CU, so a launch at 6800 is always refused.
Aux = collections.namedtuple("Aux", "kind N count scale")
# Parameters: scale 0.1 up to hidden 320 and 0.05 above (a recurrent gain scale * sqrt(N) of 1.4 to 2.6: at the table's 0.02
# every text scores 8.00 bits and a lost k-step moves that by less than the tolerance; at (1040, 0.1) the float32 and float64
# oracle samplers agree on 70-78 % of the draws only).  tests/test_hidden_widths_cpu.py holds the control.
EVAL = [Aux("eval", N, 300 if N <= 1040 else 24, 0.1 if N <= 320 else 0.05) for N in (192, 320, 1040, 2688, 2704)]
SAMPLE = [Aux("sample", 192, 200, 0.1), Aux("sample", 1040, 200, 0.05), Aux("sample", 2704, 8, 0.05)]
EVAL_TOL = 1e-4                      # bits per character (test_hip_parity.py, the evaluator tests)
LDS_UNASKED, LDS_GFX950 = 64 * 1024, 160 * 1024
N_PAST_LDS = 6800


def lds_bytes(N):
    return (6 * N + 256) * 4


def aux_id(a):
    return f"{a.N}-{a.count}"


def aux_inputs(a):
    """eval: P, text (seeded, printable).  sample: P, h0, c0, u (seeds 7 / 8 / 9, as test_generate.py's oracle test)."""
    if a.kind == "eval":
        return gu.random_case(a.N, 2, 1, seed=13 + a.N, scale=a.scale)[0], np.random.RandomState(a.N).randint(32, 127, size=a.count).astype(np.uint8)
    rs = np.random.RandomState(8)
    h0, c0 = (rs.randn(a.N) * 0.1).astype(np.float32), (rs.randn(a.N) * 0.1).astype(np.float32)
    return gu.random_case(a.N, 2, 1, seed=7, scale=a.scale)[0], h0, c0, np.random.RandomState(9).random_sample(a.count)


def aux_reference(a, kind="f32"):
    from oracle_lib import Oracle
    orc = Oracle(kind)
    if a.kind == "eval":
        P, text = aux_inputs(a)
        return orc.eval_bits(a.N, 256, P, text)
    P, h0, c0, u = aux_inputs(a)
    return orc.sample(a.N, 256, P, h0, c0, u)


def aux_control(a, _mode=None):
    """(float32 oracle, float64 oracle, float32 oracle without the last k-step of U) of an evaluator or sampler case"""
    from oracle_lib import Oracle
    P, *rest = aux_inputs(a)
    out = []
    for kind, Q in (("f32", P), ("f64", P), ("f32", drop_last_k_step(P, a.N))):
        orc = Oracle(kind)
        out.append(orc.eval_bits(a.N, 256, Q, *rest) if a.kind == "eval" else orc.sample(a.N, 256, Q, *rest))
    return out


def any_reference(case, mode=False):
    """ReferencePool's fn for a module with both kinds of cases."""
    return aux_reference(case) if isinstance(case, Aux) else reference(case, mode)


def any_id(case):
    return f"{case.kind}-{aux_id(case)}" if isinstance(case, Aux) else case_id(case)
