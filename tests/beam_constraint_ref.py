"""Beam search under a constraint as lstm_hip_beam_search_constrained states it (include/lstm_hip.h),
on tests/beam_ref.py and tests/constraint_ref.py: select32 (the device's arithmetic from logits) and select64 (the rule in
float64 from probabilities) with a table, the slots' states, accepting states and the deadline, implemented literally; the
reachability table F; and a brute-force enumerator of all the strings a small table accepts, with their costs."""
import numpy as np

import beam_ref as br
import constraint_ref as cr

f32 = np.float32
INF = br.INF
FORBID = cr.FORBID


def trivial_table():
    """one state, every byte allowed"""
    return np.zeros((1, 256), np.uint16)


def chain_table(choices):
    """len(choices) + 1 states in a chain: position i allows the bytes choices[i] and leads to state i + 1; the last state
    loops on the bytes of the last position (never reached within len(choices) bytes, but no reachable state may be empty)"""
    n = len(choices)
    t = np.full((n + 1, 256), FORBID, np.uint16)
    for i, bs in enumerate(choices):
        for b in bs:
            t[i, b] = i + 1
    for b in choices[-1]:
        t[n, b] = n
    return t


def pattern_ab_newline():
    """(table, accept) of [ab]{1,3}\\n: states 0..3 = letters read so far, 4 = after the newline (accepting; it loops on the
    newline so that it is not empty)"""
    t = np.full((5, 256), FORBID, np.uint16)
    for q in range(3):
        t[q, ord("a")] = t[q, ord("b")] = q + 1
    for q in (1, 2, 3):
        t[q, 10] = 4
    t[4, 10] = 4
    acc = np.zeros(5, np.uint8)
    acc[4] = 1
    return t, acc


def f_table(table, accept, stop, count):
    """F [count + 1, states] bool: F[0][q] = acc(q); F[R][q] = OR over the allowed bytes b of q of acc(next) if b is the stop
    byte, F[R - 1][next] otherwise"""
    table = np.asarray(table)
    Q = table.shape[0]
    F = np.zeros((count + 1, Q), bool)
    F[0] = np.asarray(accept) != 0
    for R in range(1, count + 1):
        for q in range(Q):
            for b in range(256):
                nx = int(table[q, b])
                if nx == FORBID:
                    continue
                if F[0][nx] if b == stop else F[R - 1][nx]:
                    F[R][q] = True
                    break
    return F


def strings(table, q0, count, stop=-1, accept=None):
    """Brute force: every (bytes, end state) the search may return from state q0 -- a walk of the table that ends with its
    first stop byte or holds exactly `count` bytes, in an accepting state if there are any"""
    table = np.asarray(table)
    ok = (lambda q: True) if accept is None else (lambda q: bool(accept[q]))
    found = []

    def walk(pre, q):
        if len(pre) == count or (pre and pre[-1] == stop):
            if ok(q):
                found.append((bytes(pre), q))
            return
        for b in range(256):
            nx = int(table[q, b])
            if nx != FORBID:
                walk(pre + [b], nx)
    walk([], q0)
    return found


def cost32(logits_of, table, q0, text):
    """the device's cost of `text` from state q0: the double sum in text order of the masked float32 surprisals;
    logits_of(prefix tuple) -> z [256] float32"""
    q, total = q0, 0.0
    for i, b in enumerate(text):
        z = np.where(np.asarray(table[q]) != FORBID, np.asarray(logits_of(tuple(text[:i])), f32), f32(-np.inf)).astype(f32)
        total += float(br.surprisal32(z)[b])
        q = int(table[q][b])
    return total


def _select(terms, key, cost, length, fin, q, W, stop, table, accept, Frow):
    """beam_ref._select with states: a live slot j offers byte m iff next[q_j][m] is allowed and, with accept, acc(next) for
    the stop byte / Frow[next] (F[R - 1]) otherwise.  Returns beam_ref's tuple with the new states appended before margin:
    (parent, byte, cost, length, fin, x_next, state, margin)."""
    cand = []
    for j in range(W):
        if fin[j]:
            cand.append((cost[j], j, 0.0, 0))
            continue
        offered = len(cand)
        for m in range(256):
            nx = int(table[q[j]][m])
            if nx == FORBID:
                continue
            if accept is not None and not (accept[nx] if m == stop else Frow[nx]):
                continue
            v = cost[j] + float(terms[j][m])
            cand.append((INF if v != v else v, j, -float(key[j][m]), m))
        assert len(cand) > offered, (j, q[j])  # a live slot always offers a candidate
    assert len(cand) >= W, (len(cand), W)  # a live slot always has a candidate, a finished one exactly one
    cand.sort()
    sel = cand[:W]
    margin = cand[W][0] - cand[W - 1][0] if len(cand) > W and cand[W][0] < INF else INF
    par = [c[1] for c in sel]
    byt = [c[3] for c in sel]
    new_fin = [bool(fin[p]) or b == stop for p, b in zip(par, byt)]
    new_q = [q[p] if fin[p] else int(table[q[p]][b]) for p, b in zip(par, byt)]
    return (par, byt, [c[0] for c in sel], [length[p] + (0 if fin[p] else 1) for p in par], new_fin,
            [-1 if fin[p] else b for p, b in zip(par, byt)], new_q, margin)


def select32(z, cost, length, fin, q, W, stop, table, accept=None, Frow=None):
    """the device's selection from logits z [W, 256] float32: max, sum and surprisal on the masked logits"""
    z = np.asarray(z, f32)
    terms = [None if fin[j] else br.surprisal32(np.where(np.asarray(table[q[j]]) != FORBID, z[j], f32(-np.inf)).astype(f32))
             for j in range(W)]
    return _select(terms, z, cost, length, fin, q, W, stop, table, accept, Frow)


def select64(p, cost, length, fin, q, W, stop, table, accept=None, Frow=None):
    """the rule in float64 from the unconstrained probabilities p [W, 256]: renormalised over the allowed bytes"""
    p = np.asarray(p, np.float64)
    terms = []
    for j in range(W):
        ok = np.asarray(table[q[j]]) != FORBID
        pm = np.where(ok, p[j], 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            terms.append(-np.log2(pm / pm.sum()))
    return _select(terms, p, cost, length, fin, q, W, stop, table, accept, Frow)


def search(select, first, feed, W, count, table, q0=0, stop=-1, accept=None):
    """beam_ref.search under a constraint: slots 1..W-1 start finished (cost +inf, length 0, state q0).  Adds "state" [W] and
    "margins" (one per selection) to beam_ref's result."""
    F = None if accept is None else f_table(table, accept, stop, count)
    assert F is None or F[count][q0], "no accepted string"
    cost, length, fin, state = [0.0] + [INF] * (W - 1), [0] * W, [False] + [True] * (W - 1), [q0] * W
    x, tp, tb, xl, margins = first, [], [], [], []
    for i in range(count):
        par, byt, cost, length, fin, xs, state, mg = select(x, cost, length, fin, state, W, stop, table, accept,
                                                            None if F is None else F[count - i - 1])
        tp.append(par)
        tb.append(byt)
        xl.append(xs)
        margins.append(mg)
        if i + 1 < count:
            x = feed(par, xs)
    return dict(hyps=br.backtrack(tp, tb, length, W, count), bits=cost, length=length, fin=fin, parent=tp, byte=tb, x_next=xl,
                state=state, margin=min(margins) if margins else INF, margins=margins)


def beam32(logits, W, count, table, q0=0, stop=-1, accept=None):
    """beam_ref.beam32 under a constraint (logits(prefixes) -> z [W, 256] float32)"""
    pre = [()] * W

    def feed(par, xs):
        nonlocal pre
        pre = [pre[p] + ((x,) if x >= 0 else ()) for p, x in zip(par, xs)]
        return logits(pre)

    return search(select32, logits(pre), feed, W, count, table, q0, stop, accept)


def _oracle(orc, N, P, prompt, W):
    mdl = br._OracleModel(orc, N, P, W)
    for b in prompt:
        mdl.step(range(W), [int(b)] * W)
    return mdl


def beam64(orc64, N, P, prompt, W, count, table, q0=0, stop=-1, accept=None):
    """The rule in float64 for one stream from a zero state; prompt: at least one byte, walked through the table from q0."""
    assert len(prompt) >= 1 and orc64.kind == "f64"
    mdl = _oracle(orc64, N, P, prompt, W)

    def feed(par, xs):
        mdl.step(par, xs)
        return mdl.probs

    return search(select64, mdl.probs, feed, W, count, table, cr.walk(table, q0, bytes(prompt)), stop, accept)


def beam32_oracle(orc32, N, P, prompt, W, count, table, q0=0, stop=-1, accept=None):
    """The float32 restatement: the oracle's float32 recurrence, float32 logits and the device's selection arithmetic."""
    assert len(prompt) >= 1 and orc32.kind == "f32"
    mdl = _oracle(orc32, N, P, prompt, W)

    def feed(par, xs):
        mdl.step(par, xs)
        return mdl.logits32()

    return search(select32, mdl.logits32(), feed, W, count, table, cr.walk(table, q0, bytes(prompt)), stop, accept)


def well_formed_utf8(text, utf8_table):
    return cr.walk(utf8_table, 0, text) == 0


# ---- the oracle comparison (tests/test_beam_constraint.py) and its CPU control (tests/test_beam_constraint_cpu.py): the
# control case of tests/beam_ref.py with the output rows of bytes >= 0x80 scaled up until, by the float64 reference, the
# unconstrained search returns text that is not well-formed UTF-8 and the UTF-8 search without accepting states ends a
# hypothesis inside a character
HIGH_ROW_GAIN = 3.0
HIGH_ROW_SHIFT = 1.0
ORACLE_TABLES = ("utf8", "utf8_accept", "ascii_stop")
ASCII_ALLOW = "0x20-0x7e,10"


def control_params():
    from oracle_lib import split_params
    P = np.array(br.control_params(), f32, copy=True)
    N = br.CONTROL_N
    sp = split_params(P, N)  # views into P
    assert np.shares_memory(sp["Why"], P) and np.shares_memory(sp["by"], P)
    sp["Why"][0x80:] *= f32(HIGH_ROW_GAIN)
    sp["by"][0x80:] += f32(HIGH_ROW_SHIFT)
    return P


def oracle_table(name, utf8_table):
    """(table, accept or None, stop byte) of one of ORACLE_TABLES"""
    if name == "utf8":
        return utf8_table, None, -1
    if name == "utf8_accept":
        acc = np.zeros(utf8_table.shape[0], np.uint8)
        acc[0] = 1
        return utf8_table, acc, -1
    allow = np.zeros(256, np.uint8)
    allow[0x20:0x7f] = 1
    allow[10] = 1
    t = np.full((1, 256), FORBID, np.uint16)
    t[0, allow != 0] = 0
    return t, None, 10
