"""The schedule and the arithmetic of lstm_hip_train_text_windows (include/lstm_hip.h) restated with
numpy and the unchanged oracle, for tests/test_train_texts.py (-m gpu) and its device-free control,
tests/test_train_texts_cpu.py.

The plan is lstm_hip_text_plan's rule in Python.  The expected result of one window is built by TRUNCATION: a lane with r
filled rows, and the carry or zero in column 0, is oracle.forward / oracle.backward at S' = r + 1, B = 1 on that lane's rows,
so the oracle never sees an empty target.  The window's gradient is the plain sum of the lanes' gradients (ref_backward sums
over columns without dividing), its loss the sum of the lanes' losses divided by B.  The mutant (`mutant=True`) is the
B-column oracle on the window as it stands: there a padded row has dy = p, the reference's rule for an empty target, which is
what the text windows must not do."""
import numpy as np


# The engine plans the text windows run on: (N, S, B, flag names).  Shapes of tests/test_hip_parity.py, the smallest at which
# each form of the recurrences exists.
CASES = [
    (16, 5, 1, ()),                         # the small forms: one stream on one CU
    (64, 6, 20, ()),                        # B not a multiple of the 16-column tile
    (256, 6, 3, ()),                        # fewer streams than a column group
    (512, 5, 8, ()),                        # two-half forward, scatter backward
    (512, 5, 88, ()),                       # ... in two launches over column ranges
    (128, 9, 24, ("STEP_KERNELS",)),        # one launch per step
    (128, 9, 24, ("NO_FUSED_GRADS",)),      # the unfused gradient sums
    (128, 6, 8, ("BF16_RECURRENCE",)),      # bf16 operands, against the oracle's bf16 modes
    (30, 5, 5, ("PAD_HIDDEN",)),            # a padded internal width
]
STREAMS = ("fewer", "equal", "queue")       # fewer streams than lanes (idle lanes), as many, 3B + 1 (lanes reused)


def stream_count(kind, B):
    """None where the kind does not exist (fewer than one lane)"""
    return {"fewer": B // 2 if B > 1 else None, "equal": B, "queue": 3 * B + 1}[kind]


def case_id(case, kind=None):
    N, S, B, flags = case
    return f"{N}x{S}x{B}" + "".join("-" + f.lower() for f in flags) + (f"-{kind}" if kind else "")


def all_cases():
    return [(c, k) for c in CASES for k in STREAMS if stream_count(k, c[2]) is not None]


def case_texts(case, kind):
    N, S, B, _ = case
    n = stream_count(kind, B)
    seed = 7 * N + 3 * S + B + STREAMS.index(kind)
    return texts(lengths(S, n, seed), seed + 1)


def tolerances(case):
    """(activations, loss per step, gradients): tests/test_hip_parity.py's ACT_TOL, LOSS_TOL, GRAD_TOL, and for the bf16
    recurrence the figures of its test_bf16_recurrence_matches_bf16_oracle"""
    return (2e-3, 1e-3, 1e-2) if "BF16_RECURRENCE" in case[3] else (2e-5, 2e-5, 2e-4)


def length_kinds(S):
    """every edge of a window of S - 1 steps: no step, one, two, one row short of a window, a whole one, one over, ..."""
    L = S - 1
    return (0, 1, 2, L, L + 1, L + 2, 2 * L + 1, 3 * L + 2)


def lengths(S, streams, seed):
    """`streams` lengths drawn from length_kinds(S); the first ones walk through every kind once, in a seeded order"""
    rs = np.random.RandomState(seed)
    kinds = np.array(length_kinds(S))
    out = [int(v) for v in rs.permutation(kinds)[:streams]]
    out += [int(v) for v in kinds[rs.randint(0, kinds.size, size=max(streams - len(out), 0))]]
    if max(out) < 3:   # (one or two streams may have drawn no step or a single one: keep a text that spans windows)
        out[-1] = int(kinds[-1])
    return out


def texts(lens, seed):
    import gpu_util as gu
    data = gu.text_bytes(int(np.sum(lens)) + 1, seed)
    cuts = np.concatenate([[0], np.cumsum(lens)]).astype(int)
    return [data[cuts[i]:cuts[i + 1]] for i in range(len(lens))]


def plan_ref(steps, lanes, lens):
    """(windows, lane_of, first_window): streams in index order, each to the lane whose next free window is lowest (lowest
    lane on ties), in consecutive windows; a stream without a step (fewer than 2 bytes) gets -1, -1."""
    free = np.zeros(lanes, np.int64)
    lane_of, first = np.full(len(lens), -1, np.int32), np.full(len(lens), -1, np.int64)
    for s, n_bytes in enumerate(lens):
        n = max(int(n_bytes) - 1, 0)
        if n == 0:
            continue
        lane = int(np.argmin(free))          # the first of the lowest
        lane_of[s], first[s] = lane, free[lane]
        free[lane] += -(-n // steps)
    return (int(free.max()) if len(lens) else 0), lane_of, first


def windows_ref(S, B, txts):
    """The windows the plan implies, in order.  Each: xi, ti [S, B] (-1 where a row holds no step), rows [B] (filled rows of
    each lane: they are rows 1 .. rows), stream [B] (-1: idle), fresh [B] (column 0 is zero: a text starts here, or the lane
    is idle), j0 [B] (the stream's step in row 1)."""
    L = S - 1
    lens = [len(t) for t in txts]
    n_win, lane_of, first = plan_ref(L, B, lens)
    out = []
    for w in range(n_win):
        win = dict(xi=np.full((S, B), -1, np.int32), ti=np.full((S, B), -1, np.int32), rows=np.zeros(B, np.int64),
                   stream=np.full(B, -1, np.int64), fresh=np.ones(B, bool), j0=np.zeros(B, np.int64))
        for s, t in enumerate(txts):
            n = max(lens[s] - 1, 0)
            if lane_of[s] < 0 or not first[s] <= w < first[s] + -(-n // L):
                continue
            lane, j0 = int(lane_of[s]), (w - int(first[s])) * L
            t = np.asarray(t, np.uint8)
            assert win["stream"][lane] < 0, "two streams on one lane in one window"
            win["stream"][lane], win["fresh"][lane], win["j0"][lane] = s, w == first[s], j0
            for row in range(S):
                j = j0 + row - 1
                if 0 <= j < n:
                    win["xi"][row, lane], win["ti"][row, lane] = t[j], t[j + 1]
            win["rows"][lane] = min(n - j0, L)
        out.append(win)
    return out


def window_ref(orc, N, P, win, carry_h, carry_c, mutant=False):
    """One window from the parameters P and the carry columns carry_h, carry_c [B, N] (column S - 1 of the window before;
    read for the lanes that continue a text).  Returns h, c, g, probs [S, B, .] (filled rows only; the rest NaN), mask
    [S, B], loss (bits, divided by B), grads (the flat block) and surprisal [S, B] (0 where there is no step)."""
    S, B = win["xi"].shape
    t = orc.np_t
    h0 = np.where(win["fresh"][:, None], 0.0, np.asarray(carry_h, np.float64)).astype(t)
    c0 = np.where(win["fresh"][:, None], 0.0, np.asarray(carry_c, np.float64)).astype(t)
    P = np.ascontiguousarray(P, dtype=t)
    out = dict(h=np.full((S, B, N), np.nan), c=np.full((S, B, N), np.nan), g=np.full((S, B, 4 * N), np.nan),
               probs=np.full((S, B, 256), np.nan), mask=np.zeros((S, B), bool), surprisal=np.zeros((S, B)),
               grads=np.zeros(P.size, np.float64), loss=0.0)
    if mutant:  # the whole window as the oracle takes it: dy = p on every row without a target
        fw = orc.forward(N, 256, S, B, P, win["xi"], win["ti"], h0, c0)
        out["grads"] = np.asarray(orc.backward(N, 256, S, B, P, win["xi"], win["ti"], fw), np.float64)
        out["loss"] = fw["loss_bits"]
        return out
    total = 0.0
    for lane in range(B):
        r = int(win["rows"][lane])
        if r == 0:
            continue
        xi, ti = win["xi"][:r + 1, lane:lane + 1].copy(), win["ti"][:r + 1, lane:lane + 1].copy()
        assert (xi[1:] >= 0).all() and (ti[1:] >= 0).all()   # the oracle never sees an empty target
        fw = orc.forward(N, 256, r + 1, 1, P, xi, ti, h0[lane:lane + 1], c0[lane:lane + 1])
        out["grads"] += np.asarray(orc.backward(N, 256, r + 1, 1, P, xi, ti, fw), np.float64)
        total += fw["loss_bits"]
        for name in ("h", "c", "g", "probs"):
            out[name][1:r + 1, lane] = fw[name][1:, 0]
        out["mask"][1:r + 1, lane] = True
        out["surprisal"][1:r + 1, lane] = -np.log2(fw["probs"][np.arange(1, r + 1), 0, ti[1:, 0]].astype(np.float64))
    out["loss"] = total / B
    return out


def adagrad_ref(orc, P, grads, mem, lr):
    """the oracle's Adagrad step from (P, mem): returns the stepped (P, mem) in the oracle's precision"""
    t = orc.np_t
    P, mem = np.array(P, dtype=t), np.array(mem, dtype=t)
    orc.adagrad(P, np.ascontiguousarray(grads, dtype=t), mem, lr)
    return P, mem
