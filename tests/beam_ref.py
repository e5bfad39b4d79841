"""Beam search as lstm_hip_beam_search states it (include/lstm_hip.h), twice:

beam64   the rule in float64, the model run through the oracle's one-step forward (costs are -log2 of its probabilities);
beam32   the device's arithmetic from given logits: float32 terms expf(z - zmax) summed sequentially, the surprisal
         log2f(s) + (zmax - z) * log2(e) in float32 (libm's expf / log2f, as a host build of the kernel uses), double
         accumulation, and the four-key order (cost, parent, z descending, byte).

Both share one driver: `first` is what the selection reads for the W slots after the prompt, feed(parents, xs) gathers the
slots by parent, feeds the inputs xs (-1: none) and returns the same for the next selection."""
import ctypes

import numpy as np

import sampling_ref as sr
from oracle_lib import split_params

f32 = np.float32
INF = float("inf")
LOG2E = f32(1.44269504088896341)

# the control of the oracle comparison (tests/test_beam_search_cpu.py) and the GPU test against beam64 (tests/test_beam_search.py)
CONTROL_N, CONTROL_COUNT = 64, 24
CONTROL_PROMPTS = (65, 101, 32, 120)
CONTROL_BEAMS = (1, 4, 8)
CONTROL_STOP_AT = 8  # the stopped runs stop at the byte the unstopped best hypothesis holds here


def control_params():
    return sr.peaked_params(CONTROL_N, seed=41)


_libm = None


def _m():
    global _libm
    if _libm is None:
        _libm = ctypes.CDLL("libm.so.6")
        for n in ("expf", "log2f"):
            getattr(_libm, n).restype, getattr(_libm, n).argtypes = ctypes.c_float, [ctypes.c_float]
    return _libm


def surprisal32(z):
    """c_m of one slot's logits z [256] float32, as the device computes it"""
    z = np.asarray(z, f32)
    zmax = z.max()
    e = np.array([_m().expf(float(d)) for d in (z - zmax).astype(f32)], f32)
    s = np.cumsum(e, dtype=f32)[-1]  # sequential, in index order
    return (f32(_m().log2f(float(s))) + ((zmax - z).astype(f32) * LOG2E).astype(f32)).astype(f32)


def _select(terms, key, cost, length, fin, W, stop):
    """One selection of one stream.  terms [W, 256]: the cost of each byte for each slot (added to the slot's cost as a
    double); key [W, 256]: z or anything monotone in it.  Returns (parent, byte, cost, length, fin, x_next, margin): lists
    of W, and the cost gap between the W-th and the (W+1)-th candidate (inf if there is no (W+1)-th)."""
    cand = []
    for j in range(W):
        if fin[j]:
            cand.append((cost[j], j, 0.0, 0))
            continue
        for m in range(256):
            v = cost[j] + float(terms[j][m])
            cand.append((INF if v != v else v, j, -float(key[j][m]), m))
    cand.sort()
    sel = cand[:W]
    margin = cand[W][0] - cand[W - 1][0] if len(cand) > W and cand[W][0] < INF else INF
    par = [c[1] for c in sel]
    byt = [c[3] for c in sel]
    new_fin = [bool(fin[p]) or b == stop for p, b in zip(par, byt)]
    return (par, byt, [c[0] for c in sel], [length[p] + (0 if fin[p] else 1) for p in par], new_fin,
            [-1 if fin[p] else b for p, b in zip(par, byt)], margin)


def select32(z, cost, length, fin, W, stop=-1):
    """the device's selection from logits z [W, 256] float32"""
    z = np.asarray(z, f32)
    terms = [None if fin[j] else surprisal32(z[j]) for j in range(W)]
    return _select(terms, z, cost, length, fin, W, stop)


def select64(p, cost, length, fin, W, stop=-1):
    """the rule in float64 from probabilities p [W, 256]"""
    p = np.asarray(p, np.float64)
    with np.errstate(divide="ignore"):
        return _select(-np.log2(p), p, cost, length, fin, W, stop)


def backtrack(parents, bytes_, length, W, count):
    """hypothesis r: the bytes on the way back from final slot r, cut to its length"""
    hyps = []
    for r in range(W):
        slot, rev = r, []
        for i in range(count - 1, -1, -1):
            rev.append(bytes_[i][slot])
            slot = parents[i][slot]
        hyps.append(bytes(rev[::-1][:length[r]]))
    return hyps


def search(select, first, feed, W, count, stop=-1):
    """dict(hyps [W] bytes, bits [W], length [W], fin [W], parent / byte [count][W], x_next [count][W], margin): margin is
    the smallest gap between the W-th and the (W+1)-th candidate over all selections"""
    cost, length, fin = [0.0] + [INF] * (W - 1), [0] * W, [False] * W
    q, tp, tb, xl, margin = first, [], [], [], INF
    for i in range(count):
        par, byt, cost, length, fin, xs, mg = select(q, cost, length, fin, W, stop)
        tp.append(par)
        tb.append(byt)
        xl.append(xs)
        margin = min(margin, mg)
        if i + 1 < count:
            q = feed(par, xs)
    return dict(hyps=backtrack(tp, tb, length, W, count), bits=cost, length=length, fin=fin, parent=tp, byte=tb, x_next=xl,
                margin=margin)


def beam32(logits, W, count, stop=-1):
    """The device's arithmetic on a model given as logits(prefixes) -> z [W, 256] float32, where prefixes are the W slots'
    inputs so far (tuples of bytes; a finished slot's prefix is no longer read)."""
    pre = [()] * W

    def feed(par, xs):
        nonlocal pre
        pre = [pre[p] + ((x,) if x >= 0 else ()) for p, x in zip(par, xs)]
        return logits(pre)

    return search(select32, logits(pre), feed, W, count, stop)


class _OracleModel:
    """W slots of one stream stepped by the oracle's forward pass (S = 2: one step), in the oracle's precision"""

    def __init__(self, orc, N, P, W):
        self.o, self.N, self.W = orc, N, W
        self.P = np.ascontiguousarray(P, orc.np_t)
        self.h = np.zeros((W, N), orc.np_t)
        self.c = np.zeros((W, N), orc.np_t)
        self.probs = None

    def step(self, par, xs):
        W = self.W
        xi = np.full((2, W), -1, np.int32)
        xi[1] = xs
        fw = self.o.forward(self.N, 256, 2, W, self.P, xi, np.full((2, W), -1, np.int32), self.h[list(par)], self.c[list(par)])
        self.h, self.c, self.probs = fw["h"][1].copy(), fw["c"][1].copy(), fw["probs"][1].copy()

    def logits32(self):
        """z in float32 from the oracle's h (numpy's product: the device's logits up to the order of the sum)"""
        sp = split_params(np.asarray(self.P, f32), self.N)
        return (self.h.astype(f32) @ np.ascontiguousarray(sp["Why"]).T + sp["by"][:, 0]).astype(f32)


def beam64(orc64, N, P, prompt, W, count, stop=-1):
    """The rule in float64 for one stream from a zero state; prompt: at least one byte."""
    assert len(prompt) >= 1 and orc64.kind == "f64"
    mdl = _OracleModel(orc64, N, P, W)
    for b in prompt:
        mdl.step(range(W), [int(b)] * W)

    def feed(par, xs):
        mdl.step(par, xs)
        return mdl.probs

    return search(select64, mdl.probs, feed, W, count, stop)


def beam32_oracle(orc32, N, P, prompt, W, count, stop=-1):
    """The float32 restatement: the oracle's float32 recurrence, float32 logits and the device's selection arithmetic."""
    assert len(prompt) >= 1 and orc32.kind == "f32"
    mdl = _OracleModel(orc32, N, P, W)
    for b in prompt:
        mdl.step(range(W), [int(b)] * W)

    def feed(par, xs):
        mdl.step(par, xs)
        return mdl.logits32()

    return search(select32, mdl.logits32(), feed, W, count, stop)
