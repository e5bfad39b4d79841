"""The rule and the schedule of lstm_hip_embed_texts (include/lstm_hip.h) in numpy on the oracle, the
comparison the GPU test holds the call to, and the case both tests/test_embed_texts.py (-m gpu) and
tests/test_embed_texts_cpu.py use.

A stream of L bytes has L steps; position i is the state after inputs 0..i: row i + 1 of score_ref._states_after.  The pool
is positions skip .. L - 1; the mean is the sequential double sum of the pooled values over their count, the max the largest
of them, last position L - 1 (the start state for L = 0).  Four mutants of the reference (the state before the byte; skip
ignored; the dead rows of the last window pooled; the mean over 128) must fail compare(), and do in the CPU file."""
import numpy as np

import score_ref as sc

STEPS = 128          # LSTM_HIP_EVAL_STEPS
ACT_TOL = 2e-5       # tests/test_hip_parity.py
SUR_FACTOR = 8       # section 3.17's factor (tests/eval_texts_ref.py): the engines add the same float32 products in another
                     # order, an error of the float32 oracle's own size; the factor leaves room for the device's expf / tanhf
BITS_TOL = 2e-5      # per scored byte, as tests/eval_texts_ref.py
# every edge of the 128-row window under n = L: a stream that ends on a window's last row (128, 256), one with a single row
# in its second or third window (129, 257), the empty one, and a ragged rest
LENGTHS = (0, 1, 2, 127, 128, 129, 256, 257, 37, 5)
# H32[N] = max |state32 - state64| over case(N), h and c at every position: the float32 oracle's own distance from float64,
# computed on the CPU (tests/test_embed_texts_cpu.py prints it and pins it under H32_CEILING x this table).  The GPU is held to
# max(ACT_TOL, SUR_FACTOR * H32[N]) per position, and so for mean and max, both 1-Lipschitz in the sup norm.  At N = 1024
# random_case's scale makes the recurrence's gain large and the float32 states drift over a 257-step stream (section 3.17).
H32 = {64: 6.73e-08, 100: 7.32e-08, 128: 8.53e-08, 256: 1.28e-07, 500: 3.03e-07, 512: 3.37e-07, 1024: 1.05e-04}
H32_CEILING = 2.0

KEYS = ("mean", "max", "last")


def tolerance(N):
    return max(ACT_TOL, SUR_FACTOR * H32[N])


def plan_ref(lanes, lengths):
    """eval_texts_ref.plan_ref's rule on L, not L - 1: a stream of L bytes needs ceil(L / 128) windows, an empty one gets
    -1, -1.  It is lstm_hip_text_plan(128, lanes, streams, off') with off'[s] = text_off[s] + s, as the header states."""
    free = np.zeros(lanes, np.int64)
    lane_of, first = np.full(len(lengths), -1, np.int32), np.full(len(lengths), -1, np.int64)
    for s, L in enumerate(lengths):
        n = int(L)
        if n == 0:
            continue
        lane = int(np.argmin(free))          # the first of the lowest
        lane_of[s], first[s] = lane, free[lane]
        free[lane] += -(-n // STEPS)
    return int(free.max()) if len(lengths) else 0, lane_of, first


def texts(lengths, seed):
    import gpu_util as gu
    data = gu.text_bytes(int(np.sum(lengths)) + 1, seed)
    cuts = np.concatenate([[0], np.cumsum(lengths)]).astype(int)
    return [data[cuts[i]:cuts[i + 1]] for i in range(len(lengths))]


def case(N):
    """(P, texts, h0, c0) of the oracle comparison at logical hidden size N"""
    import gpu_util as gu
    K = len(LENGTHS)
    P, _, _, h0, c0 = gu.random_case(N, 2, K, seed=2000 + N)
    return P, texts(LENGTHS, seed=N + 1), h0, c0


def states(orc, N, P, txts, h0=None, c0=None, before=False, dead=False):
    """Per stream (h [L, N], c [L, N]) in the oracle's precision: row i is position i.  before: the mutant that takes the
    state before byte i.  dead: the stream's last window filled up with the rows the recurrence goes on computing on empty
    inputs (ceil(L / 128) * 128 rows), for the mutant that pools them."""
    out = []
    for s, text in enumerate(txts):
        text = np.asarray(text, np.uint8)
        L = text.size
        hs = np.zeros(N, np.float32) if h0 is None else np.asarray(h0, np.float32)[s]
        cs = np.zeros(N, np.float32) if c0 is None else np.asarray(c0, np.float32)[s]
        if L == 0:
            out.append((np.zeros((0, N), orc.np_t), np.zeros((0, N), orc.np_t)))
            continue
        rows = -(-L // STEPS) * STEPS if dead else L
        fed = np.full(rows, -1, np.int32)
        fed[:L] = text
        fw = _forward(orc, N, P, fed, hs, cs)
        lo = 0 if before else 1
        out.append((np.array(fw["h"][lo:lo + rows, 0]), np.array(fw["c"][lo:lo + rows, 0])))
    return out


def _forward(orc, N, P, fed, hs, cs):
    if (fed >= 0).all():
        return sc._states_after(orc, N, P, fed.astype(np.uint8), hs, cs)
    S = fed.size + 1
    xi = np.full((S, 1), -1, np.int32)
    xi[1:, 0] = fed
    return orc.forward(N, sc.M, S, 1, P, xi, np.full((S, 1), -1, np.int32), hs.reshape(1, N), cs.reshape(1, N))


def pool_one(x, start, L, skip, over_steps=False):
    """(mean, max, last, count) of one stream's positions x [rows, N] (rows = L, or more for the dead-row mutant, which
    pools them all) in x's precision.  over_steps: the mutant that divides by 128."""
    x = np.asarray(x)
    lo = min(int(skip), L)
    pooled = x[lo:]
    count = L - lo
    if pooled.shape[0] == 0:
        mean, mx = np.zeros(x.shape[1], x.dtype), np.zeros(x.shape[1], x.dtype)
    else:
        total = np.cumsum(pooled.astype(np.float64), axis=0)[-1]          # the sequential double sum, in text order
        mean = (total / np.float64(STEPS if over_steps else pooled.shape[0])).astype(x.dtype)
        mx = pooled.max(axis=0)
    last = x[L - 1] if L else np.asarray(start, x.dtype)
    return mean, mx, last, count


def embed(orc, N, P, txts, h0=None, c0=None, skip=None, before=False, ignore_skip=False, dead=False, over_steps=False):
    """The statement in the oracle's precision: mean_h, max_h, last_h, mean_c, max_c, last_c [streams, N] and count."""
    K = len(txts)
    st = states(orc, N, P, txts, h0, c0, before=before, dead=dead)
    res = {f"{k}_{x}": np.zeros((K, N), orc.np_t) for k in KEYS for x in "hc"}
    res["count"] = np.zeros(K, np.int64)
    for s in range(K):
        L = len(txts[s])
        k = 0 if skip is None or ignore_skip else int(skip[s])
        for x, src, start in (("h", st[s][0], h0), ("c", st[s][1], c0)):
            start = np.zeros(N, np.float32) if start is None else np.asarray(start, np.float32)[s]
            mean, mx, last, count = pool_one(src, start, L, k, over_steps)
            res[f"mean_{x}"][s], res[f"max_{x}"][s], res[f"last_{x}"][s], res["count"][s] = mean, mx, last, count
    return res


def h32(orc32, orc64, N):
    """max |state32 - state64| over case(N)"""
    P, txts, h0, c0 = case(N)
    a, b = states(orc32, N, P, txts, h0, c0), states(orc64, N, P, txts, h0, c0)
    return max(float(np.abs(x.astype(np.float64) - y).max()) for sa, sb in zip(a, b) for x, y in zip(sa, sb) if x.size)


def compare(got, want, N, cell=True):
    """`got` (Lstm.embed_texts' dict, or embed()'s on the float32 oracle) against `want` (embed()'s on the float64 oracle).
    Returns (figures, failures): figures = the largest difference per output; failures is empty when every count is the
    statement's and every element of every output lies within tolerance(N)."""
    fails, figures = [], {}
    tol = tolerance(N)
    if not np.array_equal(np.asarray(got["count"]), want["count"]):
        fails.append(f"count {list(got['count'])}, expected {list(want['count'])}")
    for x in ("h", "c") if cell else ("h",):
        for k in KEYS:
            name = f"{k}_{x}"
            g, w = np.asarray(got[name], np.float64), np.asarray(want[name], np.float64)
            if g.shape != w.shape:
                fails.append(f"{name}: shape {g.shape}, expected {w.shape}")
                continue
            d = np.abs(g - w).max(axis=1)
            figures[name] = float(d.max())
            for s in np.nonzero(~(d <= tol))[0]:
                fails.append(f"{name}: stream {s} differs by {d[s]:.3g}, above {tol:.3g}")
    return figures, fails
