"""The arithmetic of lstm_hip_train_text_windows on weighted texts (lstm_hip_set_train_texts_weighted; include/lstm_hip.h;
DESIGN.md section 3.20) restated with numpy, the unchanged oracle and tests/text_train_ref.py, for
tests/test_train_texts_weighted.py (-m gpu) and its device-free control, tests/test_train_texts_weighted_cpu.py.

The oracle takes no weights; the reference uses the backward pass's linearity in dy.  For a lane with r filled rows let G_m
be the truncated oracle's gradient at S' = m + 1, B = 1 (rows 1..m of the lane, the lane's column 0), G_0 = 0, and L_m its
loss.  G_m - G_{m-1} is what row m's own dy adds to the gradient, through every earlier state, so the weighted gradient is

    sum_{t=1..r} w_t (G_t - G_{t-1})  =  sum_{t=1..r} (w_t - w_{t+1}) G_t        (w_{r+1} = 0; summation by parts)

and the weighted loss the same sum over L.  The right-hand form is the one computed: it needs G_t only where the weight
changes behind row t, which is two oracle runs a lane for completion weights; and the lanes of a window that have the
same coefficient at the same t share one oracle run of that many columns, whose gradient is the plain sum of their one-lane
gradients (the truncation identity of tests/test_train_texts_cpu.py; held against B = 1 runs in the CPU control).  A row's
weight is the weight of its TARGET byte: row t of a lane that holds step j = j0 + t - 1 has the stream's entry j + 1.

The mutants (what the GPU test must be able to tell apart, tests/test_train_texts_weighted_cpu.py):
  "ignored"  the weights are not read: text_train_ref.window_ref;
  "cut"      a weight-0 row is taken for a text's end: xi = ti = -1 from that row on, so no gradient flows back through it."""
import numpy as np

import text_train_ref as tr

DRAW = (0.0, 0.0, 0.25, 1.0, 3.0)            # the values the per-byte weights are drawn from
KINDS = ("drawn", "completion")
SEP = 9                                       # the separator byte of the completion cases (a tab)
# every row of text_train_ref.CASES with 3B + 1 streams, and two rows with idle lanes
LOCK_STEP = [(c, "queue") for c in tr.CASES] + [(tr.CASES[1], "fewer"), (tr.CASES[3], "fewer")]


def lock_step_params():
    return [(c, k, wk) for wk in KINDS for c, k in LOCK_STEP]


def lock_step_id(p):
    return tr.case_id(p[0], p[1]) + "-" + p[2]


def completion_weights_ref(texts, sep):
    """lstm_hip.completion_weights in plain Python: 1.0 behind the first `sep` byte of a text, 0.0 up to and including it"""
    out = []
    for t in texts:
        t = bytes(t) if isinstance(t, (bytes, bytearray)) else np.asarray(t, np.uint8).tobytes()
        at = t.find(bytes([sep]))
        out.append(np.array([1.0 if at >= 0 and i > at else 0.0 for i in range(len(t))], np.float32))
    return out


def case_texts_and_weights(case, kind, wkind):
    """The texts of text_train_ref.case_texts and a float32 weight array per text.
    drawn: every byte's weight from DRAW, seeded.  completion: every byte of value SEP is moved off it, then one separator
    byte is written into each text at a seeded position inside the text's first window with a byte behind it (so that the
    window holds context rows AND the rows learned through them), and the weights are completion_weights_ref's.  In a case
    of eight texts or more the last three of at least two bytes get the edges instead: the separator as the first byte, as
    the last byte, and absent."""
    N, S, B, _ = case
    txts = [np.array(t, np.uint8) for t in tr.case_texts(case, kind)]
    rs = np.random.RandomState(1000 + 7 * N + 3 * S + B + tr.STREAMS.index(kind) + 13 * KINDS.index(wkind))
    if wkind == "drawn":
        return txts, [rs.choice(np.array(DRAW, np.float32), size=t.size).astype(np.float32) for t in txts]
    edges = dict(zip([i for i, t in enumerate(txts) if t.size >= 2][-3:], ("first", "last", "absent"))) if len(txts) >= 8 else {}
    for i, t in enumerate(txts):
        t[t == SEP] = SEP + 1
        place = edges.get(i, "seeded")
        if t.size == 0 or place == "absent":
            continue
        t[{"first": 0, "last": t.size - 1}.get(place, int(rs.randint(1, min(t.size - 2, S - 2) + 1)) if t.size >= 3 else 0)] = SEP
    return txts, completion_weights_ref(txts, SEP)


def fullest_window(wins, weights):
    """(window, wt) of the plan's fullest window; among equally full ones the one with the most context rows, that is rows of
    weight 0 in front of a weighted row of their lane"""
    def context_rows(win, wt):
        n = 0
        for lane in range(wt.shape[1]):
            w = wt[1:int(win["rows"][lane]) + 1, lane]
            nz = np.flatnonzero(w != 0)
            n += int((w[:nz[-1]] == 0).sum()) if nz.size else 0
        return n
    pairs = [(win, window_weights(win, weights)) for win in wins]
    return max(pairs, key=lambda p: (int(p[0]["rows"].sum()), context_rows(*p)))


def window_weights(win, weights):
    """wt [S, B] float32 for a window of text_train_ref.windows_ref: the weight of each filled row's target byte, 0.0 on every
    other row (row 0, rows past a text's end, idle lanes) -- what k_text_window writes beside ti"""
    S, B = win["xi"].shape
    wt = np.zeros((S, B), np.float32)
    for lane in range(B):
        s, r, j0 = int(win["stream"][lane]), int(win["rows"][lane]), int(win["j0"][lane])
        if s >= 0 and r > 0:
            wt[1:r + 1, lane] = np.asarray(weights[s], np.float32)[j0 + 1:j0 + r + 1]
    return wt


def window_ref(orc, N, P, win, wt, carry_h, carry_c, mutant=None, together=True):
    """text_train_ref.window_ref with the weights wt [S, B]: the same fields, with loss, grads and surprisal weighted (probs
    stay the plain p).  mutant: None, "ignored" or "cut".  together=False: every oracle run has B = 1."""
    if mutant == "ignored":
        return tr.window_ref(orc, N, P, win, carry_h, carry_c)
    S, B = win["xi"].shape
    t = orc.np_t
    h0 = np.where(win["fresh"][:, None], 0.0, np.asarray(carry_h, np.float64)).astype(t)
    c0 = np.where(win["fresh"][:, None], 0.0, np.asarray(carry_c, np.float64)).astype(t)
    P = np.ascontiguousarray(P, dtype=t)
    out = dict(h=np.full((S, B, N), np.nan), c=np.full((S, B, N), np.nan), g=np.full((S, B, 4 * N), np.nan),
               probs=np.full((S, B, 256), np.nan), mask=np.zeros((S, B), bool), surprisal=np.zeros((S, B)),
               grads=np.zeros(P.size, np.float64), loss=0.0)
    total = 0.0
    rows = np.array(win["rows"], np.int64)
    # w[t, lane] for t = 1 .. rows, 0 behind the lane's last row
    w = np.zeros((S + 1, B))
    for lane in range(B):
        w[1:rows[lane] + 1, lane] = wt[1:rows[lane] + 1, lane]
        if mutant == "cut":          # the text "ends" in front of the first weight-0 row
            zero = np.flatnonzero(w[1:rows[lane] + 1, lane] == 0.0)
            if zero.size:
                rows[lane] = int(zero[0])
                w[rows[lane] + 1:, lane] = 0.0

    def run(m, lanes, backward):
        xi, ti = win["xi"][:m + 1, lanes].copy(), win["ti"][:m + 1, lanes].copy()
        assert (xi[1:] >= 0).all() and (ti[1:] >= 0).all()   # the oracle never sees an empty target
        fw = orc.forward(N, 256, m + 1, len(lanes), P, xi, ti, h0[lanes], c0[lanes])
        return fw, (np.asarray(orc.backward(N, 256, m + 1, len(lanes), P, xi, ti, fw), np.float64) if backward else None), ti

    for m in range(1, S):
        a = np.where(rows >= m, w[m] - w[m + 1], 0.0)
        # lanes with one coefficient share an oracle run: its gradient is the plain sum of their one-lane gradients and its
        # loss their mean (the truncation identity of tests/test_train_texts_cpu.py); `together=False` runs them one by one
        groups = [np.flatnonzero(a == v) for v in np.unique(a[a != 0.0])]
        if not together:
            groups = [g[i:i + 1] for g in groups for i in range(g.size)]
        for lanes in groups:
            fw, grad, _ = run(m, lanes, True)
            out["grads"] += a[lanes[0]] * grad
            total += a[lanes[0]] * fw["loss_bits"] * len(lanes)
        ends = np.flatnonzero(rows == m)
        if mutant is None and ends.size:      # the whole lanes: their activations, whatever the weights
            fw, _, ti = run(m, ends, False)
            for k, lane in enumerate(ends):
                for name in ("h", "c", "g", "probs"):
                    out[name][1:m + 1, lane] = fw[name][1:, k]
                out["mask"][1:m + 1, lane] = True
                out["surprisal"][1:m + 1, lane] = w[1:m + 1, lane] * -np.log2(
                    fw["probs"][np.arange(1, m + 1), k, ti[1:, k]].astype(np.float64))
    out["loss"] = total / B
    return out
