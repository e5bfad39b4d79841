"""Gradient accumulation (lstm_hip_set_grad_accumulation) on the oracle: the rule, three wrong rules, and the comparison that
tests/test_grad_accumulation.py makes against the oracle.  No GPU here; tests/test_grad_accumulation_cpu.py shows that the
comparison separates the rule from the wrong ones.

Tolerance.  tests/test_hip_parity.py holds one window's gradient to GRAD_TOL = 2e-4 per tensor in gpu_util.grads_report's
measure, max |a - b| / max |b|.  An accumulator is the sum of n such windows taken at the same parameters, so by the triangle
inequality its error is at most GRAD_TOL * sum_w max |g_w|, and in the same measure, relative to max |sum_w g_w|,
    tol[tensor] = GRAD_TOL * sum_w max |g_w[tensor]| / max |sum_w g_w[tensor]|  +  n * 2^-24
(the last term: one fp32 rounding per add of the running sum).  Nothing in it comes from the code under test."""
import numpy as np

import gpu_util as gu
from oracle_lib import split_params

GRAD_TOL = 2e-4  # tests/test_hip_parity.py, a single window's gradient


def host_slide(xi, ti, pos, text, S, stride):
    """OV/lstm_eigen_opt/lstm.cc:190-213 on indices, `stride` times; in place."""
    for _ in range(stride):
        ev = text[pos.astype(np.int64)].astype(np.int32)
        pos += 1
        pos[pos >= len(text)] = S
        xi[:-1] = xi[1:].copy()
        ti[:-1] = ti[1:].copy()
        ti[S - 1] = ev
        xi[S - 1] = ti[S - 2]


RULES = ("right", "first-dropped", "update-every-window", "mean-unasked")


def run_rule(orc, rule, N, S, B, P0, windows, h0, c0, carry, every, mean, lr):
    """`windows` (a list of (xi, ti)) through the oracle under `rule`.  Returns per window the accumulator after it (zeros
    when nothing is pending), the pending count, that window's own gradient and the gradient block after it (the block the
    update ran on at an update window, else the window's own), and at the end the parameters and the number of updates.
    The state carries from column `carry` of a window to column 0 of the next."""
    t = orc.np_t
    P, mem = np.array(P0, dtype=t), np.zeros(len(P0), dtype=t)
    h, c = np.asarray(h0, dtype=t), np.asarray(c0, dtype=t)
    if rule == "update-every-window":
        every = 1
    if rule == "mean-unasked":
        mean = True
    acc, pending, updates, out = None, 0, 0, []
    for xi, ti in windows:
        fw = orc.forward(N, 256, S, B, P, xi, ti, h, c)
        g = orc.backward(N, 256, S, B, P, xi, ti, fw)
        h, c = fw["h"][carry].copy(), fw["c"][carry].copy()
        if pending == 0:
            acc = np.zeros_like(g) if rule == "first-dropped" and every > 1 else g.copy()
        else:
            acc = acc + g
        pending += 1
        d = g
        if pending == every:
            d = acc * t(1.0 / every) if mean else acc
            orc.adagrad(P, np.ascontiguousarray(d, dtype=t), mem, lr)
            updates += 1
            pending = 0
        out.append((np.zeros_like(g) if pending == 0 else acc.copy(), pending, g, np.array(d)))
    return out, P, updates


def accum_tolerance(grads, N):
    """per tensor, for the sum of the windows' reference gradients `grads` (the module docstring)"""
    parts = [split_params(np.asarray(g, np.float64), N) for g in grads]
    total = split_params(np.sum([np.asarray(g, np.float64) for g in grads], axis=0), N)
    return {k: GRAD_TOL * sum(float(np.abs(p[k]).max()) for p in parts) / max(float(np.abs(total[k]).max()), 1e-30)
            + len(grads) * 2.0 ** -24 for k in total}


def accumulators_agree(got, ref, N):
    """`got` and `ref` are run_rule-shaped records (accumulator, pending, gradient, gradient block) per window.  They agree
    when the pending counts are the same, an accumulator with nothing pending is zero, and every other accumulator and
    every gradient block is within accum_tolerance of the reference's: that of the cycle so far for an accumulator and for
    the block of an update window (the cycle's sum; `mean` scales both sides by one factor), that of the window alone for
    the block of an accumulating window.  Returns (ok, the worst error / tolerance)."""
    worst, cycle = 0.0, []
    for (acc_g, pend_g, _, d_g), (acc_r, pend_r, g_r, d_r) in zip(got, ref):
        if pend_g != pend_r:
            return False, float("inf")
        cycle = cycle + [g_r]
        pairs = [(d_g, d_r, accum_tolerance(cycle if pend_r == 0 else [g_r], N))]
        if pend_r > 0:
            pairs.append((acc_g, acc_r, accum_tolerance(cycle, N)))
        elif np.any(np.asarray(acc_g) != 0):
            return False, float("inf")
        else:
            cycle = []
        for a, b, tol in pairs:
            rep = gu.grads_report(a, b, N)
            worst = max(worst, max(rep[k] / tol[k] for k in rep))
    return worst <= 1.0, worst
