"""CPU: the logic of k_gen_head's PROCESS instantiations (eigen-lstm_amd/csrc/heads/gen_head.inc) run on the
host -- the kernel's own text compiled with one thread per work-item (tests/gen_head_processed_emulation.cc) -- against the
float32 reference of tests/logit_processor_ref.py: bytes, kept counts, stop indices, end states, final states and the inputs
handed to the recurrence, bit for bit.  Logits are exact by construction (parameters, states and the bias are multiples of
1/16, N = 16), so they hold many ties, and expf is the C library's on both sides.  The given states cycle with period 1 or 2,
so a greedy stream wants the same byte again and the n-gram ban has something to remove."""
import subprocess

import numpy as np
import pytest

import constraint_ref as cr
import deadline_ref as dr
import head_emulation
import logit_processor_ref as lr

N = 16
f32 = np.float32


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    return head_emulation.build(tmp_path_factory.mktemp("gen_head_processed"), "gen_head_processed_emulation")


def _table(rs):
    """the seven states of test_deadline_head_emulation_cpu.py: 0 allows every byte, 1 exactly one, 2..5 some 3..120 of them,
    and 6 is a trap that only loops; states 0 and 4 accept"""
    Q = 7
    table = np.full((Q, 256), cr.FORBID, np.uint16)
    sizes = [256, 1, 3, 17, 64, 120]
    for q in range(6):
        allowed = rs.choice(256, sizes[q], replace=False)
        table[q, allowed] = rs.randint(0, Q, size=sizes[q])
    table[0, ::3] = 1  # (state 1 is reached often)
    table[1, table[1] != cr.FORBID] = 3
    table[6, 5:9] = 6
    accept = np.zeros(Q, np.uint8)
    accept[[0, 4]] = 1
    return table, accept


# (K, sb, count, prompt lengths, mode, tau, top_k, top_p, stop (None: chosen from the draws), table (0 none, 1 table, 2 with
#  accepting states), bias, min_p, n, history, seed)
CASES = {
    "bias_greedy": (9, 1, 10, [0, 1, 3, 0, 2, 5, 0, 0, 1], 2, 0.0, 0, 1.0, -1, 0, True, 0.0, 0, False, 1),
    "bias_tempered": (10, 4, 10, [0, 2, 0, 1, 0, 0, 3, 0, 1, 0], 1, 2.5, 0, 1.0, -1, 0, True, 0.0, 0, False, 2),
    "min_p": (10, 4, 10, [0, 2, 0, 1, 0, 0, 3, 0, 1, 0], 1, 3.0, 0, 1.0, -1, 0, False, 0.25, 0, False, 3),
    "min_p_top_k_nucleus": (20, 16, 8, [0, 1] * 10, 1, 4.0, 6, 0.9, -1, 0, False, 0.125, 0, False, 4),
    "min_p_temperature_1": (9, 1, 8, [0, 1, 3, 0, 2, 5, 0, 0, 1], 0, 1.0, 0, 1.0, -1, 0, False, 0.5, 0, False, 5),
    "n1_greedy": (9, 1, 12, [0, 1, 3, 0, 2, 5, 0, 0, 1], 2, 0.0, 0, 1.0, -1, 0, False, 0.0, 1, False, 6),
    "n3_greedy": (10, 4, 14, [0, 2, 0, 1, 0, 0, 3, 0, 1, 0], 2, 0.0, 0, 1.0, -1, 0, False, 0.0, 3, False, 7),
    "n3_greedy_history": (20, 16, 12, [1, 0, 2, 0] * 5, 2, 0.0, 0, 1.0, -1, 0, False, 0.0, 3, True, 8),
    "n3_tempered_stop": (10, 4, 14, [0, 2, 0, 1, 0, 0, 3, 0, 1, 0], 1, 0.5, 0, 1.0, None, 0, False, 0.0, 3, True, 9),
    "n2_table": (10, 4, 12, [0, 2, 0, 1, 0, 0, 3, 0, 1, 0], 2, 0.0, 0, 1.0, -1, 1, False, 0.0, 2, True, 10),
    "n2_table_tempered_all": (20, 16, 10, [0, 1] * 10, 1, 0.7, 40, 0.9, -1, 1, True, 0.25, 2, True, 11),
    "n2_deadline": (9, 1, 12, [0, 1, 3, 0, 2, 5, 0, 0, 1], 1, 0.8, 0, 1.0, -1, 2, False, 0.0, 2, False, 12),
    "n2_deadline_greedy_history": (10, 4, 10, [0, 2, 0, 1, 0, 0, 3, 0, 1, 0], 2, 0.0, 0, 1.0, -1, 2, False, 0.0, 2, True, 13),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_emulated_processed_head_matches_the_reference(emulator, tmp_path, name):
    K, sb, count, lengths, mode, tau, top_k, top_p, stop, tmode, biased, min_p, n, with_history, seed = CASES[name]
    rs = np.random.RandomState(seed)
    d = str(tmp_path)
    table, accept = _table(rs)
    if tmode == 0:
        table = None
    if tmode != 2:
        accept = None
    Why = (rs.randint(-32, 33, size=(N, 256)) / 16).astype(f32)  # [k][m]
    by = (rs.randint(-16, 17, size=256) / 16).astype(f32)
    bias = (rs.randint(-64, 65, size=256) / 16).astype(f32) if biased else None
    steps = max(lengths) + count
    period = rs.randint(1, 3, size=K)
    base = (rs.randint(-16, 17, size=(2, K, N)) / 16).astype(f32)
    Hs = np.empty((steps + 1, K, N), f32)  # the state before each step: two states per stream, taken in turn (or one)
    for t in range(steps + 1):
        for s in range(K):
            Hs[t, s] = base[t % period[s], s]
    u = rs.random_sample((count, K))
    u[rs.randint(0, count), rs.randint(0, K)] = 1.5  # past every edge
    assert len(set(lengths)) >= 2
    keep_k = top_k if 1 <= top_k <= 255 else 256
    filtered = keep_k < 256 or top_p < 1.0
    F = dr.f_table(table, accept, -1, count) if tmode == 2 else None

    # start states and prompts the table accepts (under accepting states: ending where an accepted end is within reach)
    q0 = np.zeros(K, np.int32)
    prompts = []
    if table is not None:
        q0 = rs.randint(0, 6, size=K).astype(np.int32)
        q0[:3] = (1, 0, 5)
        if F is not None:
            q0 = np.where(F[count][q0], q0, 0).astype(np.int32)
    for s, L in enumerate(lengths):
        p = []
        for _ in range(L):
            if table is None:
                b = int(rs.randint(0, 256))
            else:
                good = [b for b in np.nonzero(table[q0[s]] != cr.FORBID)[0] if F is None or F[count][table[q0[s], b]]]
                b = int(rs.choice(good))
                q0[s] = table[q0[s], b]
            p.append(b)
        prompts.append(np.array(p, np.uint8))
    # histories: under the table, every bigram (b, the one byte state 1 allows), so that the ban always empties state 1;
    # otherwise some random bytes per stream, of different lengths, none for stream 0
    histories = [np.zeros(0, np.uint8) for _ in range(K)]
    if with_history:
        if table is not None:
            only = int(np.nonzero(table[1] != cr.FORBID)[0][0])
            every = np.stack([np.arange(256), np.full(256, only)], axis=1).astype(np.uint8).ravel()
            histories = [every if s % 2 == 0 else every[:40] for s in range(K)]
        else:
            histories = [rs.randint(0, 256, size=(s * 7) % 23).astype(np.uint8) for s in range(K)]

    def reference(stop_byte):
        res, bit, drops = [], 0, 0
        for s in range(K):
            L, q, xs, ks, n_end = lengths[s], int(q0[s]), [], [], count
            T = bytes(histories[s]) + bytes(prompts[s])
            for i in range(count):
                V = lr.valid(table, q, accept, F, stop_byte, count - i)
                assert V.any()
                z = (Why.T.astype(np.float64) @ Hs[L + i, s].astype(np.float64) + by).astype(f32)  # exact
                x, k, b, dropped = lr.draw32(z, V, T, mode, tau, top_k, top_p, u[i, s], bias, min_p, n)
                assert V[x]
                bit += b
                drops += dropped
                xs.append(x)
                ks.append(k)
                T += bytes([x])
                if table is not None:
                    q = int(table[q, x])
                if x == stop_byte:
                    n_end = i + 1
                    break
            if accept is not None:
                assert accept[q], (s, q)  # the table always wins: every end state accepts
            res.append((xs, ks, n_end, q))
        return res, bit, drops

    if stop is None:  # a byte that some stream draws after its first draw, so that the stop index is exercised
        free, _, _ = reference(-1)
        late = [x for xs, _, _, _ in free for x in xs[1:]]
        stop = int(np.bincount(late, minlength=256).argmax())
    want, bit, drops = reference(stop)
    if n > 0:
        assert bit >= 1  # the ban removed a valid byte at least once
    if n > 0 and tmode == 1:
        assert drops >= 1  # state 1 has one allowed byte: the ban was dropped there
    if min_p > 0 and mode != 2:
        assert any(k < 256 for _, ks, _, _ in want for k in ks)  # min-p cut something
    off = np.zeros(K + 1, np.uint64)
    off[1:] = np.cumsum(lengths)
    texts = [np.concatenate([histories[s], prompts[s]]) for s in range(K)]
    ptoff = np.zeros(K + 1, np.uint64)
    ptoff[1:] = np.cumsum([t.size for t in texts])
    files = [("why", Why), ("by", by), ("hs", Hs), ("u", u), ("off", off),
             ("prompts", np.concatenate(prompts) if off[-1] else np.zeros(1, np.uint8)),
             ("ptext", np.concatenate(texts) if ptoff[-1] else np.zeros(1, np.uint8)), ("ptoff", ptoff)]
    if table is not None:
        files += [("tab", table), ("cnt", cr.counts(table).astype(np.uint16)), ("q", q0.astype(np.int32))]
    if accept is not None:
        files += [("acc", accept), ("frows", dr.pack_rows(F[:count]))]
    if bias is not None:
        files += [("bias", bias)]
    for fname, arr in files:
        np.ascontiguousarray(arr).tofile(f"{d}/{fname}.bin")
    subprocess.check_call([emulator, d, str(N), str(K), str(count), str(steps), str(sb), str(mode), repr(tau), str(keep_k),
                           str(int(top_p < 1.0)), repr(float(f32(top_p))), str(int(filtered)), str(stop), str(tmode),
                           str(int(biased)), repr(float(f32(min_p))), str(n)], timeout=300)
    out = np.fromfile(f"{d}/out.bin", np.uint8).reshape(count, K)
    kept = np.fromfile(f"{d}/kept.bin", np.uint16).reshape(count, K)
    end = np.fromfile(f"{d}/end.bin", np.int32)
    ho = np.fromfile(f"{d}/ho.bin", f32).reshape(K, N)
    xlog = np.fromfile(f"{d}/xlog.bin", np.int32).reshape(steps + 1, K)
    qend = np.fromfile(f"{d}/qend.bin", np.int32)
    stopped = 0
    for s in range(K):
        xs, ks, n_end, q = want[s]
        L = lengths[s]
        assert list(out[:n_end, s]) == xs and list(kept[:n_end, s]) == ks, (s, list(out[:, s]), xs, list(kept[:, s]), ks)
        assert not out[n_end:, s].any() and not kept[n_end:, s].any(), s
        assert end[s] == n_end, (s, end[s], n_end)
        if table is not None:
            assert qend[s] == q and cr.walk(table, int(q0[s]), out[:n_end, s]) == q, (s, qend[s], q)
        inputs = [int(b) for b in prompts[s]] + xs + [-1] * (steps + 1 - L - n_end)
        assert list(xlog[:, s]) == inputs, s
        assert np.array_equal(ho[s], Hs[L + n_end, s]), s
        stopped += n_end < count
    if stop >= 0:
        assert stopped >= 1
