"""CPU: the logic of k_beam_head's CONSTRAIN instantiation (eigen-lstm_amd/csrc/heads/beam_head.inc) run on
the host -- the kernel's own text and the real lse_surprisal compiled with one thread per work-item
(tests/beam_head_constrained_emulation.cc), the files tests/test_beam_head_emulation_cpu.py compiles too --
against the constrained select32 of tests/beam_constraint_ref.py: tables, costs, lengths, finished flags, next inputs, new
states and the gather of h / c, bit for bit.  Logits are exact by construction (parameters and states are multiples of 1/16,
N = 16), 56 pairs of bytes have equal logits and slots often share a state, so costs tie inside a parent and across parents.

Three tables: `random` (six states, each allowing about 40 % of the bytes; the stop byte is one the free search selects
early), `narrow` (a chain with two bytes per state: fewer than W candidates exist, so absent slots are selected), and `accept`
(four states, state 3 accepting; the stop byte is allowed in states 0 and 1 but leads into the accepting state only from 0,
and only a few bytes of state 2 lead to state 3, so the deadline removes candidates in the last two selections)."""
import subprocess

import numpy as np
import pytest

import beam_constraint_ref as bcr
import beam_ref as br
import head_emulation

N = 16
f32 = np.float32
FORBID = bcr.FORBID
STOP = 100  # of the `accept` table


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    return head_emulation.build(tmp_path_factory.mktemp("beam_head_constrained"), "beam_head_constrained_emulation")


def _table(kind, rs):
    """(table, accept or None)"""
    if kind == "random":
        Q = 6
        t = np.where(rs.random_sample((Q, 256)) < 0.4, rs.randint(0, Q, size=(Q, 256)), FORBID).astype(np.uint16)
        t[:, 7] = 0  # (no state is empty)
        return t, None
    if kind == "narrow":
        return bcr.chain_table([(97, 210), (110, 98), (99, 211), (100, 212), (101, 213), (102, 214)]), None
    t = np.full((4, 256), FORBID, np.uint16)
    for b in range(256):
        t[0, b] = rs.randint(0, 2)
        t[1, b] = rs.randint(0, 3)
        if b % 3:
            t[2, b] = 0 if b % 2 else 2
    t[2, [30, 120, 220]] = 3
    t[3, [30, 31]] = 3
    t[0, STOP], t[1, STOP], t[2, STOP] = 3, 2, FORBID  # the stop byte: into the accepting state from 0 only
    acc = np.zeros(4, np.uint8)
    acc[3] = 1
    return t, acc


def _reference(Why, by, Hs, lengths, K, W, count, stop, table, q0, accept):
    """per stream: a list over steps of None (no selection) or the constrained select32's result on that step's states.
"""
    F = None if accept is None else bcr.f_table(table, accept, stop, count)
    res = []
    for s in range(K):
        cost, length, fin, q, rows = [0.0] + [br.INF] * (W - 1), [0] * W, [False] + [True] * (W - 1), [int(q0[s])] * W, []
        for t in range(Hs.shape[0]):
            if not lengths[s] <= t < lengths[s] + count:
                rows.append(None)
                continue
            i = t - lengths[s]
            z = (Hs[t, s * W:(s + 1) * W].astype(np.float64) @ Why.astype(np.float64) + by).astype(f32)  # exact
            sel = bcr.select32(z, cost, length, fin, q, W, stop, table, accept, None if F is None else F[count - i - 1])
            cost, length, fin, q = sel[2], sel[3], sel[4], sel[6]
            rows.append(sel)
        res.append(rows)
    return res


@pytest.mark.parametrize("kind", ["random", "narrow", "accept"])
@pytest.mark.parametrize("K,W,count,lengths,seed", [
    (3, 1, 6, [0, 2, 1], 1),
    (3, 4, 6, [1, 0, 3], 2),
    (2, 5, 5, [0, 1], 3),      # beams that are no power of two: the LDS stride is W, three registers idle
    (2, 32, 4, [1, 0], 4),
])
def test_emulated_constrained_head_matches_select32(emulator, tmp_path, kind, K, W, count, lengths, seed):
    rs = np.random.RandomState(seed)
    d = str(tmp_path)
    cols, steps = K * W, max(lengths) + count
    Why = (rs.randint(-32, 33, size=(N, 256)) / 16).astype(f32)  # [k][m]
    Why[:, 200:] = Why[:, 100:156]                               # 56 pairs of bytes with equal logits in every state
    by = (rs.randint(-16, 17, size=256) / 16).astype(f32)
    if kind == "accept":
        by[STOP] += f32(3)                                       # the stop byte is likely: slots finish
    by[200:] = by[100:156]
    Hs = (rs.randint(-16, 17, size=(steps, cols, N)) / 16).astype(f32)  # the state before each step: any will do
    for t in range(steps):                                       # slots that share a state: equal costs across parents
        for c in range(cols):
            if c % W and rs.random_sample() < 0.4:
                Hs[t, c] = Hs[t, c - 1]
    Cs = (rs.randint(-16, 17, size=(steps, cols, N)) / 16).astype(f32)
    prompts = [rs.randint(0, 256, size=n).astype(np.uint8) for n in lengths]
    off = np.zeros(K + 1, np.uint64)
    off[1:] = np.cumsum(lengths)
    table, accept = _table(kind, rs)
    Q = table.shape[0]
    # the state after each stream's prompt (`accept`: the stop byte cannot end a hypothesis at once from states 1 and 2)
    q0 = list(rs.randint(0, Q, size=K)) if kind == "random" else [(s + 1) % 3 for s in range(K)] if kind == "accept" else [0] * K
    if kind == "accept":
        stop = STOP
    else:  # one the unstopped search selects early in stream 0, so that slots finish while others live
        free = _reference(Why, by, Hs, lengths, K, W, count, -1, table, q0, None)
        stop = free[0][lengths[0] + 1][1][0]
    arrays = [("why", Why), ("by", by), ("hs", Hs), ("cs", Cs), ("off", off), ("table", table),
              ("q0", np.repeat(np.array(q0, np.int32), W)),
              ("prompts", np.concatenate(prompts) if off[-1] else np.zeros(1, np.uint8))]
    if accept is not None:
        F = bcr.f_table(table, accept, stop, count)
        assert all(F[count][q] for q in q0)
        rows = np.zeros((count, (Q + 31) // 32), np.uint32)
        for R in range(count):
            for q in range(Q):
                if F[R][q]:
                    rows[R, q >> 5] |= np.uint32(1 << (q & 31))
        arrays += [("accept", accept), ("frows", rows)]
    for name, arr in arrays:
        np.ascontiguousarray(arr).tofile(f"{d}/{name}.bin")
    subprocess.check_call([emulator, d, str(N), str(K), str(W), str(count), str(steps), str(stop), str(Q),
                           str(int(accept is not None))], timeout=600)
    tp = np.fromfile(f"{d}/tp.bin", np.uint8).reshape(count, cols)
    tb = np.fromfile(f"{d}/tb.bin", np.uint8).reshape(count, cols)
    xlog = np.fromfile(f"{d}/xlog.bin", np.int32).reshape(steps, cols)
    costlog = np.fromfile(f"{d}/costlog.bin", np.float64).reshape(steps, cols)
    lenlog = np.fromfile(f"{d}/lenlog.bin", np.int32).reshape(steps, cols)
    finlog = np.fromfile(f"{d}/finlog.bin", np.int32).reshape(steps, cols)
    qlog = np.fromfile(f"{d}/qlog.bin", np.int32).reshape(steps, cols)
    hr = np.fromfile(f"{d}/hr.bin", f32).reshape(steps, cols, N)
    cr = np.fromfile(f"{d}/cr.bin", f32).reshape(steps, cols, N)
    ref = _reference(Why, by, Hs, lengths, K, W, count, stop, table, q0, accept)
    stopped = absent = 0
    for s in range(K):
        sl = slice(s * W, (s + 1) * W)
        for t in range(steps):
            sel = ref[s][t]
            if sel is None:
                want_x = [int(prompts[s][t])] * W if t < lengths[s] else [-1] * W
                assert list(xlog[t, sl]) == want_x, (s, t)
                assert np.array_equal(hr[t, sl], Hs[t, sl]) and np.array_equal(cr[t, sl], Cs[t, sl]), (s, t)
                continue
            par, byt, cost, length, fin, xs, q, _ = sel
            i = t - lengths[s]
            assert list(tp[i, sl]) == par and list(tb[i, sl]) == byt, (s, i, list(tp[i, sl]), par, list(tb[i, sl]), byt)
            assert costlog[t, sl].tobytes() == np.array(cost, np.float64).tobytes(), (s, i)
            assert list(lenlog[t, sl]) == length and [bool(f) for f in finlog[t, sl]] == fin, (s, i)
            assert list(xlog[t, sl]) == xs, (s, i)
            assert list(qlog[t, sl]) == q, (s, i, list(qlog[t, sl]), q)
            assert np.array_equal(hr[t, sl], Hs[t, sl][par]) and np.array_equal(cr[t, sl], Cs[t, sl][par]), (s, i)
            absent += sum(c == br.INF and n == 0 for c, n in zip(cost, length))
            if i == count - 1:
                stopped += sum(f and n > 0 for f, n in zip(fin, length))
                if accept is not None:  # every hypothesis of finite bits stands in an accepting state
                    assert all(accept[qq] for qq, c in zip(q, cost) if c < br.INF), (s, q, cost)
    if W > 1 or kind == "accept":
        assert stopped >= 1  # (the stop byte was selected)
    if kind == "narrow" and W > 1:
        assert absent >= 1   # fewer than W strings exist: slots that stand for no hypothesis were selected
    if kind == "accept":
        # the last two selections read live slots, and the accepting states (stop byte) and the deadline removed candidates
        # the table alone allows
        for back in (1, 2):
            removed = 0
            for s in range(K):
                before = ref[s][lengths[s] + count - back - 1]  # the slots that selection count - back reads
                for q, fin in zip(before[6], before[4]):
                    if not fin:
                        nx = table[q]
                        ok = nx != FORBID
                        exists = [ok[m] and bool(accept[nx[m]] if m == stop else F[back - 1][nx[m]]) for m in range(256)]
                        assert any(exists), (s, back, q)  # a live slot always has a candidate
                        removed += int(ok.sum()) - sum(exists)
            assert removed >= 1, back
