"""The logit processors of lstm_hip_generate_processed (include/lstm_hip.h) in numpy, on
tests/sampling_ref.py, tests/constraint_ref.py and tests/deadline_ref.py: an additive bias, the no-repeat n-gram ban with its
drop rule, and min-p as one more cap on keep.

draw32 follows the device's arithmetic (float32, sequential sums, the C library's expf) from the logits on; filter64 states
the same rule in float64 for comparisons against the oracle."""
import numpy as np

import constraint_ref as cr
import deadline_ref as dr
import sampling_ref as sr

M = 256
FORBID = cr.FORBID
f32 = np.float32


def ngram_banned(T, n):
    """[256] bool: B_m of the n-gram rule for the text T (bytes or a uint8 array): with suf the last n - 1 bytes of T, byte m
    is banned iff some j with j + n - 1 < len(T) has T[j : j + n - 1] == suf and T[j + n - 1] == m.  Empty when
    len(T) < n - 1 (or n == 0); n == 1 bans every byte that occurs in T."""
    T = bytes(np.asarray(T, np.uint8).tobytes()) if not isinstance(T, (bytes, bytearray)) else bytes(T)
    B = np.zeros(M, bool)
    if n < 1 or len(T) < n - 1:
        return B
    suf = T[len(T) - (n - 1):]
    for j in range(len(T) - n + 1):  # j + n - 1 < len(T)
        if T[j:j + n - 1] == suf:
            B[T[j + n - 1]] = True
    return B


def valid(table=None, q=0, accept=None, F=None, stop=-1, R=0):
    """[256] bool: V_m -- every byte without a table, the allowed bytes of state q with one, the bytes that exist with R draws
    left under accepting states"""
    if table is None:
        return np.ones(M, bool)
    if accept is None:
        return np.asarray(table[q]) != FORBID
    return dr.exists(table, accept, F, stop, q, R)


def survivors(V, T, n):
    """(survivor mask, banned mask, dropped): V without the banned bytes, or V itself where that leaves nothing"""
    B = ngram_banned(T, n) if n > 0 else np.zeros(M, bool)
    S = V & ~B
    if not S.any():
        return V.copy(), B, True
    return S, B, False


def min_p_keep32(by_rank, min_p):
    """keep_m in float32: the first rank whose term is below (float)min_p * the largest term, 256 if none"""
    if not min_p > 0:
        return M
    thr = f32(f32(min_p) * f32(by_rank[0]))
    for r in range(1, M):
        if f32(by_rank[r]) < thr:
            return r
    return M


def min_p_keep64(p_sorted, min_p):
    """the same in float64 on a descending distribution"""
    if not min_p > 0:
        return M
    below = np.nonzero(np.asarray(p_sorted, np.float64) < min_p * p_sorted[0])[0]
    return int(below[0]) if below.size else M


def draw32(z, V, T, mode, tau, top_k, top_p, u, bias=None, min_p=0.0, n=0, forget_prompt=0):
    """One processed draw as the head computes it from the float32 logits z (before the bias): returns (byte, kept, banned a
    valid byte, dropped).  V: valid(); T: history ++ prompt ++ drawn bytes.  mode 0: expf(z') unshifted, 1:
    expf((z' - max) / tau), 2: greedy.  forget_prompt: a mutant for the control -- the ban skips that many leading bytes of T."""
    z = np.asarray(z, f32)
    if bias is not None:
        z = (z + np.asarray(bias, f32)).astype(f32)
    S, B, dropped = survivors(V, bytes(T)[forget_prompt:], n)
    bit = bool((B & V).any())
    zm = np.where(S, z, f32(-np.inf)).astype(f32)
    if mode == 2:
        return int(np.argmax(zm)), 1, bit, dropped
    zmax = zm.max()
    with np.errstate(invalid="ignore"):
        e = np.array([cr._libm.expf(float(zm[m])) if mode == 0 else cr._libm.expf(float(f32(f32(zm[m] - zmax) / f32(tau))))
                      for m in range(M)], f32)
    s = f32(0)
    for m in range(M):
        s = f32(s + e[m])
    p = (e / s).astype(f32)
    r = sr.ranks(zm)
    by_rank = p[np.argsort(r)]
    keep = min(top_k if 1 <= top_k <= 255 else 256, int(S.sum()))
    if top_p < 1.0:
        acc, edge = f32(0.0), f32(top_p)
        for i in range(keep):
            acc = f32(acc + by_rank[i])
            if acc >= edge:
                keep = i + 1
                break
    keep = min(keep, min_p_keep32(by_rank, min_p))
    mask = r < keep
    q = np.where(mask, p, f32(0.0)).astype(f32)
    s = f32(0.0)
    for m in range(M):
        s = f32(s + q[m])
    q = (q / s).astype(f32)
    x, cdf, uf = int(np.nonzero(mask)[0].max()), f32(0.0), f32(u)
    for m in range(M):
        cdf = f32(cdf + q[m])
        if uf < cdf:
            x = m
            break
    return x, keep, bit, dropped


def filter64(p1, S, tau, top_k, top_p, min_p=0.0, bias=None):
    """(keep, kept mask, renormalised p'', p before the filter) of a processed tempered draw in float64, from the oracle's
    temperature-1 probabilities p1 and the survivor mask S"""
    w = np.asarray(p1, np.float64)
    if bias is not None:
        w = w * np.exp(np.asarray(bias, np.float64))
    t = np.where(S, w, 0.0) ** (1.0 / tau)
    p = t / t.sum()
    key = np.where(S, w, -1.0)
    k = min(top_k if 1 <= top_k <= 255 else 256, int(S.sum()))
    keep, _, _ = sr.filter64(key, p, k if k <= 255 else 0, top_p)
    r = sr.ranks(key)
    keep = min(keep, int(S.sum()), min_p_keep64(p[np.argsort(r)], min_p))
    mask = r < keep
    pp = np.where(mask, p, 0.0)
    return keep, mask, pp / pp.sum(), p


def ambiguous(p, S, top_k, top_p, min_p=0.0):
    """sampling_ref.ambiguous under the survivor cap, extended: some term within 1e-6 relative of the min-p threshold"""
    k = min(top_k if 1 <= top_k <= 255 else 256, int(S.sum()))
    if sr.ambiguous(p, k if k <= 255 else 0, top_p):
        return True
    if min_p > 0:
        thr = min_p * np.max(p)
        rest = np.sort(np.asarray(p, np.float64))[::-1][1:]  # (the largest term is kept whatever the threshold)
        if (np.abs(rest - thr) < 1e-6 * thr).any():
            return True
    return False


def repeats_ngram(T, n):
    """does some n-gram occur twice in T?"""
    T = bytes(T)
    seen = set()
    for j in range(len(T) - n + 1):
        g = T[j:j + n]
        if g in seen:
            return True
        seen.add(g)
    return False


# ---- the case of the GPU oracle comparison (tests/test_logit_processors.py) and of its CPU control
# (tests/test_logit_processors_cpu.py): sampling_ref.oracle_case() (the peaked one) with min-p and a bias of +-2 on sixteen bytes
ORACLE_SETTINGS = (  # (min_p, biased, top_k, top_p, temperature)
    (0.05, False, 0, 1.0, 1.0),
    (0.3, False, 0, 1.0, 0.8),
    (0.05, True, 0, 1.0, 1.0),
    (0.3, True, 40, 0.9, 1.0),
)


def oracle_bias():
    """+2 on eight bytes, -2 on eight others"""
    rs = np.random.RandomState(44)
    pick = rs.choice(np.arange(32, 127), 16, replace=False)
    bias = np.zeros(M, f32)
    bias[pick[:8]] = 2.0
    bias[pick[8:]] = -2.0
    return bias
