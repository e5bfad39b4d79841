"""The cases of tests/test_input_statistics.py (-m gpu) and of its reference-only control, tests/test_input_statistics_cpu.py:
one table, one set of inputs, one set of checks, so that the control covers exactly what the GPU file asserts.

A case is one training window (forward, loss, backward) at a shape that puts the handle on one path of the per-byte gradient
sums, with input bytes from one of gpu_util.DISTRIBUTIONS.  The reference of an fp32 handle is the float64 oracle, of a bf16
handle the float32 oracle in bf16 mode.  The oracle is serial and dominates the time, so the references of all cases are
computed in worker processes (ReferencePool), one case per worker at a time.
"""
import collections
import concurrent.futures
import multiprocessing
import re

import numpy as np

import gpu_util as gu
from oracle_lib import cpu_share

# forms as lstm_hip_plan_identity prints them (csrc/kernels.h: FwdForm, BwdForm)
FWD_STEP, FWD_SMALL = 0, 1
BWD_STEP, BWD_SMALL, BWD_PERSISTENT, BWD_COLS8, BWD_SCATTER, BWD_BF16, BWD_BF16_SCATTER = range(7)
# csrc/kernels.hip: dW_db takes k_dW_table up to DWT_MAX_T columns, dW_sort takes k_bucket_columns_rank up to
# 64 * 16 * RANK_SLOTS columns and k_bucket_columns above (test_input_statistics_cpu.py checks these against the source)
DWT_MAX_T, RANK_MAX_T = 2560, 16384

CORE = ("text", "one_byte", "chunk_edges", "all_empty")
REST = tuple(d for d in gu.DISTRIBUTIONS if d not in CORE)
TARGET_VARIANTS = (("text", "one_byte"), ("text", "same"), ("one_byte", "same"))
TARGET_VARIANT_MAX_T = 1300

Shape = collections.namedtuple("Shape", "path N S B flags env plan dw launches every")
# path: the row of the table; plan: what lstm_hip_plan_identity must say on the device at hand (256 CUs); dw: who sums dW and
# db ("fold": inside the backward recurrence, group partials folded; "table": k_dW_table; "rank": k_bucket_columns_rank and
# the segment sums; "sort": k_bucket_columns and the segment sums); launches: launches of the backward recurrence per window
# (column ranges); every: all distributions and the target variants, not only CORE.
SHAPES = [
    Shape("fused scatter, 4-column pinned groups", 512, 12, 24, (), {}, dict(bwd=BWD_SCATTER, fused=1, gc=4, gp=4, lc=64), "fold", 1, True),
    Shape("fused scatter, 8-column groups, one launch", 512, 100, 64, (), {}, dict(bwd=BWD_SCATTER, fused=1, gc=8, lc=64), "fold", 1, False),
    Shape("fused scatter, 8-column groups, one launch", 256, 50, 128, (), {}, dict(bwd=BWD_SCATTER, fused=1, gc=8, lc=128), "fold", 1, False),
    Shape("fused scatter, several launches", 256, 10, 272, (), {}, dict(bwd=BWD_SCATTER, fused=1, gc=8, lc=128), "fold", 3, False),
    Shape("fused scatter, several launches", 512, 7, 1024, (), {}, dict(bwd=BWD_SCATTER, fused=1, gc=8, lc=64), "fold", 16, False),
    # the reference's best model: hidden 500, window 7, 1024 streams, at the padded width 512
    Shape("fused scatter, several launches", 500, 7, 1024, ("PAD_HIDDEN",), {}, dict(np=512, bwd=BWD_SCATTER, fused=1, gc=8, lc=64), "fold", 16, False),
    Shape("fused one-recurrence 8-column form", 128, 25, 16, (), {}, dict(bwd=BWD_COLS8, fused=1, bc=8, gp=8), "fold", 1, False),
    Shape("fused one-recurrence 8-column form", 64, 40, 33, (), {}, dict(bwd=BWD_COLS8, fused=1, bc=8, gp=8), "fold", 1, True),
    Shape("fused one-recurrence 8-column form", 512, 9, 64, (), {"LSTM_HIP_BWD_HALVES": "0"}, dict(bwd=BWD_COLS8, fused=1, bc=8, gp=8), "fold", 1, False),
    Shape("unfused, k_dW_table", 1024, 100, 16, (), {}, dict(bwd=BWD_COLS8, fused=0, bc=8, side=0), "table", 1, False),
    Shape("unfused, k_dW_table", 1024, 100, 16, ("BF16_RECURRENCE",), {}, dict(bwd=BWD_BF16_SCATTER, fused=0, side=0), "table", 1, False),
    # single-CU form; 300 columns (the table's starting shape has 100, fewer than chunk_edges needs)
    Shape("unfused, k_dW_table", 128, 301, 1, (), {}, dict(fwd=FWD_SMALL, bwd=BWD_SMALL, fused=0), "table", 1, False),
    Shape("unfused on the side stream, rank sort", 256, 100, 64, ("NO_FUSED_GRADS",), {}, dict(bwd=BWD_SCATTER, fused=0, side=1, gc=4), "rank", 1, True),
    Shape("unfused, generic sort", 256, 100, 272, ("NO_FUSED_GRADS",), {}, dict(bwd=BWD_SCATTER, fused=0, side=1, lc=128), "sort", 3, False),
    Shape("unfused, generic sort", 256, 100, 272, ("BF16_RECURRENCE",), {}, dict(bwd=BWD_BF16_SCATTER, fused=0, lc=128), "sort", 3, False),
    Shape("unfused, generic sort", 64, 130, 130, ("STEP_KERNELS",), {}, dict(fwd=FWD_STEP, bwd=BWD_STEP, fused=0), "sort", 129, False),
    Shape("16-column backward groups, unfused", 128, 70, 264, (), {}, dict(bwd=BWD_PERSISTENT, fused=0, bc=16), "sort", 1, True),
    # (the table's (1024, 5, 64) has no co-resident persistent grid on 256 CUs and plans the per-step engine)
    Shape("16-column backward groups, unfused", 128, 10, 264, (), {}, dict(bwd=BWD_PERSISTENT, fused=0, bc=16), "table", 1, True),
]

Case = collections.namedtuple("Case", "shape dist target")


def _cases():
    out = []
    for sh in SHAPES:
        for d in CORE + (REST if sh.every else ()):
            out.append(Case(sh, d, "uniform"))
        # (on the short windows: with one byte in and out over 18 216 columns the float32 oracle's own serial sums miss a
        # quarter of the tolerances -- dW 8.1e-5, loss 9.7e-4 bits at (128, 70, 264) -- so that case shrank to these)
        if sh.every and (sh.S - 1) * sh.B <= TARGET_VARIANT_MAX_T:
            out += [Case(sh, d, t) for d, t in TARGET_VARIANTS]
    return out


CASES = _cases()


def bf16(case):
    return "BF16_RECURRENCE" in case.shape.flags


def case_id(case):
    sh = case.shape
    tag = "".join("-" + f.lower() for f in sh.flags) + "".join(f"-{k[9:].lower()}{v}" for k, v in sh.env.items())
    return f"{sh.N}x{sh.S}x{sh.B}{tag}-{case.dist}" + ("" if case.target == "uniform" else f"-t_{case.target}")


def inputs(case):
    """P, xi, ti, h0, c0 of a case: random_case's parameters and state, the window from gpu_util.window_bytes."""
    sh = case.shape
    seed = sh.N + 3 * sh.S + 7 * sh.B + 11 * gu.DISTRIBUTIONS.index(case.dist) + 101 * gu.TARGETS.index(case.target)
    scale = (0.05 if sh.N <= 256 else 0.02) if bf16(case) else (0.08 if sh.N <= 256 else 0.02)
    P, _, _, h0, c0 = gu.random_case(sh.N, sh.S, sh.B, seed=seed, scale=scale)
    xi, ti = gu.window_bytes(case.dist, sh.S, sh.B, seed, case.target)
    return P, xi, ti, h0, c0


# ---- the references, in worker processes --------------------------------------------------------------------------------
_oracles = {}


def _oracle(kind):
    if kind not in _oracles:
        from oracle_lib import Oracle
        _oracles[kind] = Oracle(kind)
    return _oracles[kind]


def _window(orc, sh, P, xi, ti, h0, c0):
    fw = orc.forward(sh.N, 256, sh.S, sh.B, P, xi, ti, h0, c0)
    d = orc.backward(sh.N, 256, sh.S, sh.B, P, xi, ti, fw)
    return dict(h_last=fw["h"][sh.S - 1].copy(), loss=fw["loss_bits"], grads=d)


def reference(case, with_f32=False):
    """The case's reference window: dict(h_last, loss, grads).  with_f32 (fp32 cases): (float64, float32) oracle results."""
    sh = case.shape
    P, xi, ti, h0, c0 = inputs(case)
    if bf16(case):
        orc = _oracle("f32")
        orc.set_bf16_recurrence(True)
        orc.set_bf16_products(True)
        try:
            return _window(orc, sh, P, xi, ti, h0, c0)
        finally:
            orc.set_bf16_recurrence(False)
            orc.set_bf16_products(False)
    ref = _window(_oracle("f64"), sh, P.astype(np.float64), xi, ti, h0, c0)
    if with_f32:
        return ref, _window(_oracle("f32"), sh, P, xi, ti, h0, c0)
    return ref


def selected_cases(request):
    """The cases of the requesting module's tests that this session actually runs (-k, a node id): only their references
    are computed."""
    return [it.callspec.params["case"] for it in request.session.items
            if it.module is request.module and "case" in getattr(getattr(it, "callspec", None), "params", {})]


class ReferencePool:
    """reference() of every case, computed ahead in worker processes (spawned: the parent may hold a GPU context)."""

    def __init__(self, cases, with_f32=False, fn=None, key=None):
        """fn(case, with_f32) computes a reference (default: reference), key(case) names it (default: case_id); cases with
        one key share one reference, which get() hands to each of them and then lets go."""
        workers = max(1, min(16, cpu_share()))
        self.ex = concurrent.futures.ProcessPoolExecutor(max_workers=workers, mp_context=multiprocessing.get_context("spawn"))
        self.key = key or case_id
        self.users = collections.Counter(self.key(c) for c in cases)
        self.futures = {}
        for c in cases:
            if self.key(c) not in self.futures:
                self.futures[self.key(c)] = self.ex.submit(fn or reference, c, with_f32)

    def get(self, case):
        k = self.key(case)
        self.users[k] -= 1
        return (self.futures[k] if self.users[k] > 0 else self.futures.pop(k)).result()

    def close(self):
        self.ex.shutdown(wait=True, cancel_futures=True)


# ---- the checks ---------------------------------------------------------------------------------------------------------
# (last h, loss per step, gradients per tensor and per dW column): the project's tolerances for an fp32 and a bf16 handle
TOL_FP32 = dict(h=2e-5, loss=2e-5, grad=2e-4)
TOL_BF16 = dict(h=2e-3, loss=1e-3, grad=1e-2)
SHARE_TOL = 2e-4   # db - sum_v dW[:, v] against the reference's, of max|db_ref|


def check_window(case, got, ref, xi, fraction=1.0):
    """Every assertion of a case on dict(h_last, loss, grads) against the reference; fraction scales every tolerance (the
    control runs the float32 oracle through this with 0.25).  Prints the figures, then asserts; returns the figures."""
    sh = case.shape
    tol = TOL_BF16 if bf16(case) else TOL_FP32
    fig = dict(h=gu.max_rel(got["h_last"], ref["h_last"]), loss=abs(got["loss"] - ref["loss"]))
    rep = gu.grads_report(got["grads"], ref["grads"], sh.N)
    fig.update({"d" + k: v for k, v in rep.items()})
    worst, byte, size, nonzero_absent = gu.dW_byte_report(got["grads"], ref["grads"], sh.N, xi)
    fig.update(dW_col=worst, dW_col_byte=byte, dW_col_bucket=size)
    share_ref = gu.db_minus_dW(ref["grads"], sh.N)
    db_ref = np.abs(np.asarray(ref["grads"], np.float64)[4 * sh.N * 256 + 4 * sh.N * sh.N:][:4 * sh.N]).max()
    fig["share"] = float(np.abs(gu.db_minus_dW(got["grads"], sh.N) - share_ref).max() / max(db_ref, 1e-30))
    print(case_id(case), " ".join(f"{k}={v:.2e}" if isinstance(v, float) else f"{k}={v}" for k, v in fig.items()))
    assert fig["h"] <= tol["h"] * fraction, fig
    assert fig["loss"] <= tol["loss"] * (sh.S - 1) * fraction, fig
    assert max(rep.values()) <= tol["grad"] * fraction, rep
    assert worst <= tol["grad"] * fraction, f"dW column of byte {byte} (a bucket of {size} columns) is off by {worst:.2e} of its scale"
    assert not nonzero_absent, f"dW columns of bytes that do not occur are not exactly 0: {nonzero_absent[:16]}"
    assert fig["share"] <= SHARE_TOL * fraction, fig
    if case.dist == "all_empty":
        assert got["loss"] == 0.0, got["loss"]
        assert not np.any(np.asarray(got["grads"])[:4 * sh.N * 256] != 0.0), "dW of a window without inputs is not exactly 0"
    return fig


def parse_plan(text):
    """'np512 fwd4 bwd4 fused1 ...' -> {'np': 512, 'fwd': 4, ...}"""
    return {k: int(v) for k, v in re.findall(r"([a-z]+)(\d+)", text)}


def assert_plan(L, want):
    """The handle's plan string, after asserting the fields of `want` in it: a case fails, not skips, on another path."""
    text = L.plan_identity()
    plan = parse_plan(text)
    off = {k: (plan.get(k), v) for k, v in want.items() if plan.get(k) != v}
    assert not off, f"not the intended path: plan '{text}' (got, wanted): {off}"
    return text
