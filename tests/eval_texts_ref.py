"""The rule and the schedule of lstm_hip_eval_texts (include/lstm_hip.h) in numpy, the comparison the
GPU test holds the call to, and the case both tests/test_eval_texts.py (-m gpu) and tests/test_eval_texts_cpu.py use.

The float64 reference is score_ref.score64(first=False) with the skip mask applied: byte j >= 1 scored on the state after
inputs 0..j-1, entries below skip[s] zero.  Two mutants of it (the byte scored on the state one step late; skip ignored) must
fail compare(), and do in the CPU file."""
import numpy as np

import score_ref as sc

STEPS = 128          # LSTM_HIP_EVAL_STEPS
BITS_TOL = 2e-5      # per scored byte: the project's LOSS_TOL per step (tests/test_hip_parity.py)
SUR_FACTOR = 8       # per-byte surprisal within SUR_FACTOR * D32
# D32[N] = max |score32 - score64| per byte over case(N), measured (tests/test_eval_texts_cpu.py prints it): the error of the
# sequential float32 statement against float64.  The engines add the same float32 products in another order, an error of that
# size; the factor leaves room for the device's expf / log2f against the C library's.
# Up to N = 512 it is about one float32 ulp of a surprisal of 8 bits (9.5e-7): the rounding of p and of -log2f(p).  At
# N = 1024 random_case's scale 0.08 makes the recurrence's gain large (a row of U has norm 2.6) and the float32 oracle's states
# drift from the float64 ones over a 256-step stream: thirty times as much (the surprisals themselves are no larger, at most
# 10.5 bits).  The GPU's distance from float64 at that width is of the same size.
D32 = {64: 1.37e-6, 100: 1.14e-6, 128: 1.19e-6, 256: 1.19e-6, 500: 1.16e-6, 512: 1.15e-6, 1024: 3.47e-5}
D32_CEILING = 2.0    # the CPU test pins a freshly computed D32 below D32_CEILING * D32[N]

LENGTHS = (0, 1, 2, 128, 129, 130, 257, 37, 5, 64)   # every edge of the 128-step window, and a ragged rest


def plan_ref(lanes, lengths):
    """(windows, lane_of, first_window): streams in index order, each to the lane whose next free window is lowest (lowest
    lane on ties), in consecutive windows; a stream without a step (fewer than 2 bytes) gets -1, -1."""
    free = np.zeros(lanes, np.int64)
    lane_of, first = np.full(len(lengths), -1, np.int32), np.full(len(lengths), -1, np.int64)
    for s, L in enumerate(lengths):
        n = max(int(L) - 1, 0)
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
    """(P, texts, h0, c0) of the oracle comparison at logical hidden size N: gpu_util.random_case parameters and states,
    text_bytes texts of LENGTHS."""
    import gpu_util as gu
    K = len(LENGTHS)
    P, _, _, h0, c0 = gu.random_case(N, 2, K, seed=1000 + N)
    return P, texts(LENGTHS, seed=N), h0, c0


def mask_skip(res, skip):
    """score64's / score32's result with the entries below skip[s] zeroed and the bits summed again, in text order"""
    out = {"surprisal": [], "bits": np.zeros(len(res["surprisal"]))}
    for s, sur in enumerate(res["surprisal"]):
        sur = np.array(sur, copy=True)
        if skip is not None:
            sur[:int(skip[s])] = 0
        out["surprisal"].append(sur)
        total = 0.0
        for v in sur:
            total += float(v)
        out["bits"][s] = total
    return out


def eval64(orc64, N, P, txts, h0=None, c0=None, skip=None, late=False, ignore_skip=False):
    """The float64 statement.  late / ignore_skip are the two mutants."""
    res = sc.score64(orc64, N, P, txts, h0, c0, first=False, shift=1 if late else 0)
    return mask_skip(res, None if ignore_skip else skip)


def eval32(orc32, N, P, txts, h0=None, c0=None, skip=None):
    return mask_skip(sc.score32(orc32, N, P, txts, h0, c0, first=False), skip)


def scored(lengths, skip=None):
    """scored bytes per stream: bytes max(skip, 1) .. L - 1"""
    skip = np.zeros(len(lengths), np.int64) if skip is None else np.asarray(skip, np.int64)
    return np.array([max(int(L) - max(int(k), 1), 0) for L, k in zip(lengths, skip)])


def compare(got, want, N, skip=None):
    """`got` (Lstm.eval_texts' dict with surprisal, or eval32's) against `want` (eval64's).  Returns (figures, failures):
    figures = the largest per-byte difference in bits and the largest per-stream difference per scored byte; failures is
    empty when every unscored entry is 0, every scored byte lies within SUR_FACTOR * D32[N] and every stream's bits within
    BITS_TOL * (scored bytes)."""
    fails, d_sur, d_bits = [], 0.0, 0.0
    lengths = [np.asarray(w).size for w in want["surprisal"]]
    cnt = scored(lengths, skip)
    for s, L in enumerate(lengths):
        g, w = np.asarray(got["surprisal"][s]), np.asarray(want["surprisal"][s])
        if g.shape != w.shape:
            fails.append(f"stream {s}: {g.shape} entries, expected {w.shape}")
            continue
        first = L - cnt[s]
        if np.any(g[:first] != 0):
            fails.append(f"stream {s}: an unscored byte has an entry")
        if cnt[s]:
            d = float(np.abs(g[first:].astype(np.float64) - w[first:]).max())
            d_sur = max(d_sur, d)
            if not d <= SUR_FACTOR * D32[N]:
                fails.append(f"stream {s}: surprisal differs by {d:.3g} bits, above {SUR_FACTOR * D32[N]:.3g}")
        db = abs(float(got["bits"][s]) - float(want["bits"][s]))
        d_bits = max(d_bits, db / max(cnt[s], 1))
        if not db <= BITS_TOL * cnt[s]:
            fails.append(f"stream {s}: bits {float(got['bits'][s])!r}, expected {float(want['bits'][s])!r} within {BITS_TOL * cnt[s]:.3g}")
    return dict(surprisal=d_sur, bits_per_byte=d_bits), fails


def split_ref(length, pieces, warm):
    """(start, stop, skip) per piece: piece i scores bytes a_i .. a_{i+1} - 1, a_i = 1 + floor(i (length - 1) / pieces), on the
    stream text[max(0, a_i - 1 - warm) : a_{i+1}]"""
    out = []
    for i in range(pieces):
        a, b = 1 + (i * (length - 1)) // pieces, 1 + ((i + 1) * (length - 1)) // pieces
        start = max(0, a - 1 - warm)
        out.append((start, b, a - start))
    return out


def split_bits64(orc64, N, P, text, pieces, warm):
    """bits per character of the split on the float64 statement"""
    text = np.asarray(text, np.uint8)
    cut = split_ref(text.size, pieces, warm)
    res = eval64(orc64, N, P, [text[a:b] for a, b, _ in cut], skip=[k for _, _, k in cut])
    return float(res["bits"].sum()) / (text.size - 1)
