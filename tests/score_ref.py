"""The rule of lstm_hip_score (include/lstm_hip.h) in numpy, stated twice, and the comparison the
oracle tests share.

statement64 / score64 state it in float64 on the oracle's forward probabilities.  statement32 / score32 follow the device's
arithmetic from the float32 logits on: every sum sequential in index order, expf and log2f the C library's (the ones the host
emulation of the head calls).  Both return what Lstm.score returns: per text the arrays surprisal, entropy, rank, top_byte,
top_bits, and bits per stream; score64 adds lnp, the natural-log probabilities compare() judges near-ties by."""
import ctypes

import numpy as np

import sampling_ref as sr
from oracle_lib import split_params

M = 256
FORBID = 0xFFFF
f32 = np.float32
LOG2E = f32(1.44269504088896341)

_libm = ctypes.CDLL("libm.so.6")
for _name in ("expf", "log2f"):
    getattr(_libm, _name).restype, getattr(_libm, _name).argtypes = ctypes.c_float, [ctypes.c_float]


def _expf(v):
    return np.array([_libm.expf(float(x)) for x in v], f32)


def _log2f(v):
    return np.array([_libm.log2f(float(x)) for x in v], f32)


def _seq_sum(v):
    s = f32(0.0)
    for x in v:
        s = f32(s + x)
    return s


def statement32(z, x, stable, ok=None, top_n=0):
    """One scored byte from its float32 logits: (surprisal, entropy, rank, top_byte [top_n], top_bits [top_n]).
    ok: the bytes the constraint allows where the byte stands (None: all)."""
    z = np.asarray(z, f32)
    if ok is not None:
        z = np.where(ok, z, f32(-np.inf)).astype(f32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if stable:
            zmax = z[0]
            for v in z[1:]:
                if v > zmax:
                    zmax = v
            e = _expf((z - zmax).astype(f32))
        else:
            e = _expf(z)
        s = _seq_sum(e)
        p = (e / s).astype(f32)
        lg = _log2f(p)
        if stable:
            sur = (_libm.log2f(float(s)) + ((zmax - z).astype(f32) * LOG2E).astype(f32)).astype(f32)
        else:
            sur = (-lg).astype(f32)
        t = np.where(p > 0, (p * lg).astype(f32), f32(0.0)).astype(f32)
    ent = f32(-_seq_sum(t))
    r = sr.ranks(z)
    order = np.argsort(r)[:top_n]
    return sur[x], ent, int(r[x]), order.astype(np.uint8), sur[order]


def statement64(p, x, ok=None, top_n=0):
    """The same from float64 probabilities: (surprisal, entropy, rank, top_byte, top_bits, lnp [256])"""
    p = np.asarray(p, np.float64)
    if ok is not None:
        p = np.where(ok, p, 0.0)
        p = p / p.sum()
    with np.errstate(divide="ignore"):
        lnp = np.log(p)
    lg = lnp / np.log(2.0)
    ent = -np.sum(np.where(p > 0, p * np.where(p > 0, lg, 0.0), 0.0))
    r = sr.ranks(p if ok is None else np.where(ok, p, -1.0))  # forbidden bytes last, in index order
    order = np.argsort(r)[:top_n]
    return -lg[x], ent, int(r[x]), order.astype(np.uint8), -lg[order], lnp


def logits32(P, N, h):
    """z = Why*h + by as the heads sum it: sequentially in k, separate multiply and add, float32"""
    p = split_params(np.asarray(P, f32), N, M)
    Why, h = p["Why"], np.asarray(h, f32)
    y = np.zeros(M, f32)
    for k in range(N):
        y = (y + (Why[:, k] * h[k]).astype(f32)).astype(f32)
    return (y + p["by"][:, 0]).astype(f32)


def _empty(K, with_lnp):
    res = {k: [None] * K for k in ("surprisal", "entropy", "rank", "top_byte", "top_bits")}
    res["bits"] = np.zeros(K, np.float64)
    res["end_state"] = None
    if with_lnp:
        res["lnp"] = [None] * K
    return res


def _walk_states(table, q, text):
    """the state every byte of `text` stands in, and the state after the last"""
    qs = []
    for b in text:
        qs.append(q)
        q = int(table[q, b])
        assert q != FORBID
    return qs, q


def _states_after(orc, N, P, text, h0, c0):
    """forward pass over the text from (h0, c0): rows 0..len(text) hold the state (and, from row 1, the probabilities) after that
    many inputs"""
    L = len(text)
    S = L + 1
    xi = np.full((S, 1), -1, np.int32)
    xi[1:, 0] = text
    return orc.forward(N, M, S, 1, P, xi, np.full((S, 1), -1, np.int32), np.asarray(h0, f32).reshape(1, N),
                       np.asarray(c0, f32).reshape(1, N))


def _score(orc, wide, N, P, texts, h0, c0, first, top_n, table, start_state, stable, shift):
    K = len(texts)
    res = _empty(K, wide)
    if table is not None:
        res["end_state"] = np.zeros(K, np.int32)
    pp = split_params(np.asarray(P, np.float64), N, M)
    for s, text in enumerate(texts):
        text = np.asarray(text, np.uint8)
        L = text.size
        hs = np.zeros(N, f32) if h0 is None else np.asarray(h0, f32)[s]
        cs = np.zeros(N, f32) if c0 is None else np.asarray(c0, f32)[s]
        sur, ent = np.zeros(L, np.float64 if wide else f32), np.zeros(L, np.float64 if wide else f32)
        rank, tby, tbi = np.zeros(L, np.uint8), np.zeros((L, top_n), np.uint8), np.zeros((L, top_n), sur.dtype)
        lnp = np.zeros((L, M))
        qs, q_end = ([None] * L, 0) if table is None else _walk_states(table, 0 if start_state is None else int(start_state[s]), text)
        if table is not None:
            res["end_state"][s] = q_end
        fw = _states_after(orc, N, P, text, hs, cs) if L else None
        for j in range(L):
            if j == 0 and not first:
                continue  # an input only: all-zero entries
            ok = None if table is None else np.asarray(table[qs[j]]) != FORBID
            at = min(j + shift, L)  # (shift: the mutant that scores byte j on the state after j + 1 inputs)
            if wide:
                if at == 0:
                    z = pp["Why"] @ hs.astype(np.float64) + pp["by"][:, 0]
                    p = np.exp(z - z.max())
                    p /= p.sum()
                else:
                    p = np.asarray(fw["probs"][at, 0], np.float64)
                sur[j], ent[j], rank[j], tby[j], tbi[j], lnp[j] = statement64(p, text[j], ok, top_n)
            else:
                z = logits32(P, N, fw["h"][at, 0])
                sur[j], ent[j], rank[j], tby[j], tbi[j] = statement32(z, text[j], stable, ok, top_n)
            res["bits"][s] += float(sur[j])
        for k, v in (("surprisal", sur), ("entropy", ent), ("rank", rank), ("top_byte", tby), ("top_bits", tbi)):
            res[k][s] = v
        if wide:
            res["lnp"][s] = lnp
    return res


def score64(orc64, N, P, texts, h0=None, c0=None, first=False, top_n=0, table=None, start_state=None, shift=0):
    """The float64 statement on the oracle's probabilities.  shift = 1 is a mutant the comparison must catch: byte j scored on
    the state after j + 1 inputs."""
    return _score(orc64, True, N, P, texts, h0, c0, first, top_n, table, start_state, False, shift)


def score32(orc32, N, P, texts, h0=None, c0=None, first=False, top_n=0, table=None, start_state=None, stable=False):
    """The float32 statement on the float32 oracle's states"""
    return _score(orc32, False, N, P, texts, h0, c0, first, top_n, table, start_state, stable, 0)


# ---- the comparison of a float32 result with the float64 statement (tests/test_score.py, and its control and mutants in
# tests/test_score_cpu.py) ------------------------------------------------------------------------------------------------------
NEAR = 2e-5          # two bytes whose ln p lie closer than this may rightly change places in float32
MAX_LEFT_OUT = 0.01  # share of positions the rank / top-n checks may leave out


BOUND = 1e-4         # bits: the margin tests/test_generate.py and tests/test_beam_search.py hold the scorer to against float64


def compare(got, want, first, n):
    """`got` (Lstm.score's dict or score32's) against `want` (score64's).  Returns (figures, failures): figures = the largest
    surprisal and entropy differences over the scored bytes, in bits, and how many positions the rank and top-n checks left
    out of how many; failures = a list of strings, empty when `got` follows the rule:
      every unscored byte (byte 0 when not first) has all-zero entries;
      surprisal, entropy and the compared alternatives' bits lie within BOUND of the statement's, a stream's bits within
      BOUND per byte;
      rank is compared unless another byte's ln p lies within NEAR of the text byte's;
      the first n alternatives are compared unless two of the position's first n + 1 ln p do."""
    fails, d_sur, d_ent, d_top, out_rank, out_top, scored = [], 0.0, 0.0, 0.0, 0, 0, 0
    for s in range(len(want["surprisal"])):
        L = want["surprisal"][s].size
        if any(np.asarray(got[k][s]).shape[0] != L for k in ("surprisal", "entropy", "rank", "top_byte", "top_bits")):
            fails.append(f"stream {s}: lengths")
            continue
        for j in range(L):
            g = {k: np.asarray(got[k][s][j]) for k in ("surprisal", "entropy", "rank", "top_byte", "top_bits")}
            if j == 0 and not first:
                if any(np.any(v != 0) for v in g.values()):
                    fails.append(f"stream {s}: the unscored byte 0 has entries")
                continue
            scored += 1
            lnp = want["lnp"][s][j]
            x_lnp = -want["surprisal"][s][j] * np.log(2.0)
            with np.errstate(invalid="ignore"):
                d_sur = max(d_sur, abs(float(g["surprisal"]) - want["surprisal"][s][j]))
                d_ent = max(d_ent, abs(float(g["entropy"]) - want["entropy"][s][j]))
                if np.count_nonzero(np.abs(lnp - x_lnp) < NEAR) > 1:  # (the byte itself is one)
                    out_rank += 1
                elif int(g["rank"]) != int(want["rank"][s][j]):
                    fails.append(f"stream {s} byte {j}: rank {int(g['rank'])}, expected {int(want['rank'][s][j])}")
                head = np.sort(lnp)[::-1][:n + 1]
                gaps = head[:-1] - head[1:]
                if np.any(gaps[np.isfinite(gaps)] < NEAR):
                    out_top += 1
                elif not np.array_equal(g["top_byte"][:n], want["top_byte"][s][j][:n]):
                    fails.append(f"stream {s} byte {j}: alternatives {list(g['top_byte'][:n])}, expected {list(want['top_byte'][s][j][:n])}")
                else:
                    w = want["top_bits"][s][j][:n]
                    fin = np.isfinite(w)
                    if not np.array_equal(np.isfinite(g["top_bits"][:n]), fin):
                        fails.append(f"stream {s} byte {j}: alternatives' bits not infinite where forbidden")
                    elif fin.any():
                        d_top = max(d_top, float(np.abs(g["top_bits"][:n][fin] - w[fin]).max()))
        want_bits, got_bits = want["bits"][s], float(got["bits"][s])
        if not abs(got_bits - want_bits) <= BOUND * max(L, 1):
            fails.append(f"stream {s}: bits {got_bits}, expected {want_bits}")
    figures = dict(surprisal=d_sur, entropy=d_ent, top_bits=d_top, left_out_rank=out_rank, left_out_top=out_top, scored=scored)
    for k in ("surprisal", "entropy", "top_bits"):
        if not figures[k] <= BOUND:
            fails.append(f"{k} differs by {figures[k]:.3g} bits, above {BOUND}")
    if out_rank > MAX_LEFT_OUT * scored or out_top > MAX_LEFT_OUT * scored:
        fails.append(f"too many positions left out: {out_rank} / {out_top} of {scored}")
    return figures, fails


# ---- the case of the oracle comparison and of its control
def oracle_case():
    """(N, P, texts [8 x 48], h0, c0 [8, 64])"""
    import gpu_util as gu
    N = 64
    P = sr.peaked_params(N, seed=41)
    texts = gu.text_bytes(384, 7).reshape(8, 48)
    rs = np.random.RandomState(7)
    h0 = (rs.standard_normal((8, N)) * 0.3).astype(f32)
    c0 = (rs.standard_normal((8, N)) * 0.3).astype(f32)
    return N, P, texts, h0, c0
