"""The arithmetic of lstm_hip_set_soft_targets (include/lstm_hip.h) restated with numpy and the unchanged
oracle, for tests/test_soft_targets.py (-m gpu) and its device-free control, tests/test_soft_targets_cpu.py.

The oracle does all the LSTM work.  Its ref_backward forms dy = probs - onehot(ti), so a call with ti = -1 everywhere and the
wanted dy in place of probs back-propagates any dy.  This module computes, in the oracle's precision, the student's and the
teacher's forward passes, the logits z = Why h + by from the oracle's h (operands rounded to bf16 where the oracle's bf16
product mode is on, as its own forward pass does), and per column with target k (k < 0: none)
    r     = (1 - eps) e_k + eps / 256        (k >= 0),     0 (k < 0)
    q     = softmax(z_T / tau),  p_tau = softmax(z / tau)   (max-shifted; p_tau = the oracle's probs at tau = 1)
    dy    = alpha (probs - r) + (1 - alpha) tau (p_tau - q)
    kl    = sum_m q_m (log2 q_m - log2 p_tau,m)            (log-sum-exp form; 0 where q_m is 0)
the window's KL figure sum_t (sum_b kl) / B, the gradients through the call above and the update through oracle.adagrad.
`mutant` names one of MUTANTS, a wrong rule the controls must catch."""
import numpy as np

import gpu_util as gu

# student (N, S, B, flag names) / teacher (N, flag names): the smallest shapes at which each engine form exists
# (tests/text_train_ref.py)
CASES = [
    ((16, 5, 1, ()), (32, ())),                                       # the small forms
    ((64, 6, 20, ()), (128, ())),
    ((256, 6, 3, ()), (64, ())),                                      # T = 15: an odd column count, a ragged last workgroup
    ((512, 5, 8, ()), (256, ())),                                     # two-half forward, scatter backward
    ((128, 9, 24, ("STEP_KERNELS",)), (128, ("STEP_KERNELS",))),
    ((128, 9, 24, ("NO_FUSED_GRADS",)), (256, ())),
    ((128, 6, 8, ("BF16_RECURRENCE",)), (256, ("BF16_RECURRENCE",))),  # the oracle's bf16 modes on both
    ((30, 5, 5, ("PAD_HIDDEN",)), (50, ("PAD_HIDDEN",))),
    ((64, 6, 20, ("STABLE_SOFTMAX",)), (128, ())),
]
# (alpha, tau, eps); the first runs without a teacher
SETTINGS = [(1.0, 1.0, 0.1), (0.5, 1.0, 0.0), (0.0, 1.0, 0.0), (0.5, 2.0, 0.1), (0.0, 4.0, 0.0)]
MUTANTS = ("no_tau", "smooth_empty", "no_teacher_on_empty")
LR = 0.1


def case_id(case):
    (N, S, B, flags), (Nt, tflags) = case
    return f"{N}x{S}x{B}" + "".join("-" + f.lower() for f in flags) + f"-from-{Nt}" + "".join("-" + f.lower() for f in tflags)


def is_bf16(flags):
    return "BF16_RECURRENCE" in flags


def tolerances(case):
    """(activations, loss and KL per step, gradients): tests/test_hip_parity.py's ACT_TOL, LOSS_TOL, GRAD_TOL, and for a bf16
    student the figures of its test_bf16_recurrence_matches_bf16_oracle"""
    return (2e-3, 1e-3, 1e-2) if is_bf16(case[0][3]) else (2e-5, 2e-5, 2e-4)


def case_inputs(case, seed=None, empty=True):
    """Student and teacher parameters and states, and one window.  The student's scale is 0.08 (0.05 under bf16), the teacher
    draws from seed + 1; one target of the window is empty (its input byte stays)."""
    (N, S, B, flags), (Nt, tflags) = case
    seed = N + S + B if seed is None else seed
    P, xi, ti, h0, c0 = gu.random_case(N, S, B, seed=seed, scale=0.05 if is_bf16(flags) else 0.08)
    Pt, _, _, ht0, ct0 = gu.random_case(Nt, S, B, seed=seed + 1, scale=0.05 if is_bf16(tflags) else 0.08)
    if empty:
        ti[1 + seed % (S - 1), seed % B] = -1
    return dict(P=P, xi=xi, ti=ti, h0=h0, c0=c0, Pt=Pt, ht0=ht0, ct0=ct0)


def bf16_rne(x):
    """float32 values rounded to bf16, round to nearest even (finite inputs), as float32"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def set_bf16(orc, on):
    orc.set_bf16_recurrence(on), orc.set_bf16_products(on)


def logits(orc, N, P, h, bf16):
    """z [S, B, 256] = Why h + by from the oracle's h [S, B, N] (row 0 is not a step)"""
    t = orc.np_t
    p = gu.split_params(np.asarray(P, t), N)
    Why, hh = p["Why"], np.asarray(h, t)
    if bf16:
        Why, hh = bf16_rne(Why).astype(t), bf16_rne(hh).astype(t)
    return (hh @ Why.T.astype(t) + p["by"][:, 0][None, None, :]).astype(t)


def log_softmax(z):
    """natural log of the max-shifted softmax over the last axis, and the softmax"""
    s = z - z.max(axis=-1, keepdims=True)
    lse = np.log(np.exp(s).sum(axis=-1, keepdims=True, dtype=z.dtype))
    return s - lse, np.exp(s - lse)


def forward(orc, N, P, xi, ti, h0, c0, bf16=False):
    """oracle.forward in the oracle's bf16 modes or not; they are left off"""
    if bf16:
        set_bf16(orc, True)
    try:
        return orc.forward(N, 256, xi.shape[0], xi.shape[1], np.asarray(P, orc.np_t), xi, ti, h0, c0)
    finally:
        if bf16:
            set_bf16(orc, False)


def soft_dy(orc, fw, z, zt, ti, alpha, tau, eps, mutant=None):
    """dy [S, B, 256], per-column kl in bits [S, B] and the objective alpha CE(r, p) + (1 - alpha) tau^2 KL(q || p_tau) in
    nats summed over the window's columns, from the oracle's probs, the student's logits z and the teacher's zt (None: no
    teacher).  Row 0 of each is zero."""
    t = orc.np_t
    S, B, M = z.shape
    alpha, tau, eps = t(alpha), t(tau), t(eps)
    has = (ti >= 0)[:, :, None]
    onehot = (np.arange(M)[None, None, :] == ti[:, :, None])
    r = np.where(has, (t(1) - eps) * onehot + eps / t(M), t(0)).astype(t)
    if mutant == "smooth_empty":
        r = ((t(1) - eps) * onehot + eps / t(M)).astype(t)
    p = np.asarray(fw["probs"], t)
    logp = log_softmax(z)[0]
    dy = alpha * (p - r)
    kl = np.zeros((S, B), t)
    value = -(alpha * r * logp)[1:].sum(dtype=np.float64)
    if zt is not None:
        logq, q = log_softmax((zt / tau).astype(t))
        logpt, pt = (logp, p) if tau == 1 else log_softmax((z / tau).astype(t))
        term = (t(1) - alpha) * (pt - q) * (t(1) if mutant == "no_tau" else tau)
        if mutant == "no_teacher_on_empty":
            term = np.where(has, term, t(0))
        dy = dy + term
        kln = np.where(q > 0, q * (logq - logpt), t(0)).sum(axis=-1, dtype=t)
        kl = (kln / t(np.log(2.0))).astype(t)
        value += float((t(1) - alpha) * tau * tau) * kln[1:].sum(dtype=np.float64)
    dy, kl = dy.astype(t), kl.astype(t)
    dy[0], kl[0] = 0, 0
    return dy, kl, value


def backward_dy(orc, N, P, xi, fw, dy, bf16=False):
    """the gradients of any dy through the unchanged oracle: ti = -1 everywhere, dy in place of probs"""
    S, B = xi.shape
    none = np.full((S, B), -1, np.int32)
    sub = dict(h=fw["h"], c=fw["c"], g=fw["g"], probs=np.ascontiguousarray(dy, orc.np_t))
    if bf16:
        set_bf16(orc, True)
    try:
        return orc.backward(N, 256, S, B, np.asarray(P, orc.np_t), xi, none, sub)
    finally:
        if bf16:
            set_bf16(orc, False)


def window(orc, case, inp, setting, teacher=True, mutant=None, P=None, h0=None, c0=None, ht0=None, ct0=None, xi=None, ti=None):
    """One window of the student of `case` under `setting`, from the inputs of case_inputs (each may be replaced).  Returns
    fw (the student's oracle.forward: h, c, g, probs, loss_bits), fwt (the teacher's, or None), dy, kl (the window's figure in
    bits), colkl [S, B], grads (the flat block) and value (the objective in nats)."""
    (N, S, B, flags), (Nt, tflags) = case
    alpha, tau, eps = setting
    P = inp["P"] if P is None else P
    xi, ti = inp["xi"] if xi is None else xi, inp["ti"] if ti is None else ti
    h0, c0 = inp["h0"] if h0 is None else h0, inp["c0"] if c0 is None else c0
    bf = is_bf16(flags)
    fw = forward(orc, N, P, xi, ti, h0, c0, bf)
    z = logits(orc, N, P, fw["h"], bf)
    fwt, zt = None, None
    if teacher:
        ht0, ct0 = inp["ht0"] if ht0 is None else ht0, inp["ct0"] if ct0 is None else ct0
        fwt = forward(orc, Nt, inp["Pt"], xi, ti, ht0, ct0, is_bf16(tflags))
        zt = logits(orc, Nt, inp["Pt"], fwt["h"], is_bf16(tflags))
    dy, colkl, value = soft_dy(orc, fw, z, zt, ti, alpha, tau, eps, mutant)
    grads = backward_dy(orc, N, P, xi, fw, dy, bf)
    kl = float(sum(float(colkl[t].sum(dtype=orc.np_t) / orc.np_t(B)) for t in range(1, S)))
    return dict(fw=fw, fwt=fwt, dy=dy, kl=kl, colkl=colkl, grads=grads, value=value)


def adagrad_ref(orc, P, grads, mem, lr):
    """the oracle's Adagrad step from (P, mem): returns the stepped (P, mem) in the oracle's precision"""
    t = orc.np_t
    P, mem = np.array(P, dtype=t), np.array(mem, dtype=t)
    orc.adagrad(P, np.ascontiguousarray(grads, dtype=t), mem, lr)
    return P, mem


def compare(a, b, S):
    """the figures the tolerances bound, of window result a against b: activations (max_rel of h, c, g, probs over the
    steps), loss and kl (absolute, per step), gradients (grads_report's worst tensor)"""
    act = max(gu.max_rel(a["fw"][k][1:], b["fw"][k][1:]) for k in ("h", "c", "g", "probs"))
    N = a["fw"]["h"].shape[2]
    return dict(act=act, loss=abs(a["fw"]["loss_bits"] - b["fw"]["loss_bits"]) / (S - 1), kl=abs(a["kl"] - b["kl"]) / (S - 1),
                grad=max(gu.grads_report(a["grads"], b["grads"], N).values()))
