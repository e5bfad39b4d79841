"""CPU: the logic of k_gen_head's DEADLINE instantiation (eigen-lstm_amd/csrc/heads/gen_head.inc) run on the
host -- the kernel's own text compiled with one thread per work-item (tests/gen_head_deadline_emulation.cc) -- against the
float32 reference of tests/deadline_ref.py: bytes, kept counts, stop indices, end states, final states and the inputs handed
to the recurrence, bit for bit.  Logits are exact by construction (parameters and states are multiples of 1/16, N = 16), so
they hold many ties, and expf is the C library's on both sides.  Streams have prompts of different lengths, so one launch
holds streams at different distances from their deadline."""
import subprocess

import numpy as np
import pytest

import constraint_ref as cr
import deadline_ref as dr
import head_emulation

N = 16
f32 = np.float32


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    return head_emulation.build(tmp_path_factory.mktemp("gen_head_deadline"), "gen_head_deadline_emulation")


def _table(rs):
    """seven states: 0 allows every byte, 1 exactly one, 2..5 some 3..120 of them, and 6 is a trap that only loops; states 0
    and 4 accept.  A byte into the trap is allowed by the table and never exists."""
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


@pytest.mark.parametrize("K,sb,count,lengths,mode,tau,top_k,top_p,stop,seed", [
    (9, 1, 12, [0, 1, 3, 0, 2, 5, 0, 0, 1], 1, 0.8, 0, 1.0, -1, 1),       # the deadline alone, tempered
    (10, 4, 10, [0, 2, 0, 1, 0, 0, 3, 0, 1, 0], 0, 1.0, 0, 1.0, -1, 2),   # alone, temperature 1, a partial last group
    (20, 16, 8, [0, 1] * 10, 0, 1.0, 3, 1.0, -1, 3),                      # with top-k, 16 streams a group (partial)
    (10, 4, 10, [0, 2, 0, 1, 0, 0, 3, 0, 1, 0], 1, 0.7, 40, 0.9, -1, 4),  # with both filters
    (20, 16, 8, [1, 0, 2, 0] * 5, 1, 1.5, 0, 0.8, None, 5),               # nucleus and a stop byte (chosen from the draws)
    (10, 4, 10, [0, 2, 0, 1, 0, 0, 3, 0, 1, 0], 2, 0.0, 40, 0.9, None, 6),  # greedy: masked argmax, a stop byte
    (6, 1, 8, [0, 0, 1, 0, 2, 0], 0, 1.0, 0, 1.0, None, 7),               # a stop byte under the deadline alone
])
def test_emulated_deadline_head_matches_the_reference(emulator, tmp_path, K, sb, count, lengths, mode, tau, top_k, top_p, stop, seed):
    rs = np.random.RandomState(seed)
    d = str(tmp_path)
    table, accept = _table(rs)
    Q = table.shape[0]
    Why = (rs.randint(-32, 33, size=(N, 256)) / 16).astype(f32)  # [k][m]
    by = (rs.randint(-16, 17, size=256) / 16).astype(f32)
    steps = max(lengths) + count
    Hs = (rs.randint(-16, 17, size=(steps + 1, K, N)) / 16).astype(f32)  # the state before each step: any will do
    u = rs.random_sample((count, K))
    u[rs.randint(0, count), rs.randint(0, K)] = 1.5  # past every edge
    assert len(set(lengths)) >= 2  # streams at different R in one launch
    keep_k = top_k if 1 <= top_k <= 255 else 256
    filtered = keep_k < 256 or top_p < 1.0

    def prompts_for(F):
        """prompts the table accepts, ending where an accepted end is within reach (the API refuses any other)"""
        start = rs.randint(0, 6, size=K).astype(np.int32)
        start[:3] = (1, 0, 5)
        start = np.where(F[count][start], start, 0).astype(np.int32)  # (a stop byte can shut a state off: state 0 never is)
        assert len(set(start)) >= 3
        prompts, q0 = [], start.copy()
        for s, n in enumerate(lengths):
            p = []
            for _ in range(n):
                good = [b for b in np.nonzero(table[q0[s]] != cr.FORBID)[0] if F[count][table[q0[s], b]]]
                b = int(rs.choice(good))
                p.append(b)
                q0[s] = table[q0[s], b]
            prompts.append(np.array(p, np.uint8))
        assert all(F[count][q] for q in q0), q0
        return prompts, q0

    def reference(stop_byte, F, q0):
        """per stream (bytes, kept, end index, end state); *cut: draws at which fewer bytes exist than the table allows"""
        res, cut = [], 0
        A = cr.counts(table)
        for s in range(K):
            L, q, xs, ks, n_end = lengths[s], int(q0[s]), [], [], count
            for i in range(count):
                R = count - i
                E = int(dr.exists(table, accept, F, stop_byte, q, R).sum())
                assert E >= 1
                cut += E < A[q]
                z = (Why.T.astype(np.float64) @ Hs[L + i, s].astype(np.float64) + by).astype(f32)  # exact
                x, k = dr.draw32(z, table, accept, F, stop_byte, q, R, mode, tau, top_k, top_p, u[i, s])
                assert dr.exists(table, accept, F, stop_byte, q, R)[x] and k <= E
                xs.append(x)
                ks.append(k)
                q = int(table[q, x])
                if x == stop_byte:
                    n_end = i + 1
                    break
            assert accept[q], (s, q)  # the point of the feature
            res.append((xs, ks, n_end, q))
        return res, cut

    state = rs.get_state()
    F = dr.f_table(table, accept, -1, count)
    prompts, q0 = prompts_for(F)
    if stop is None:  # a byte that some stream draws after its first draw, so that the stop index is exercised (asserted below)
        free, _ = reference(-1, F, q0)
        late = []  # bytes drawn after a first draw that led into an accepting state: as a stop byte they exist there
        for s, (xs, _, _, _) in enumerate(free):
            q = int(q0[s])
            for i, x in enumerate(xs):
                q = int(table[q, x])
                if i >= 1 and accept[q]:
                    late.append(x)
        stop = int(np.bincount(late, minlength=256).argmax())
        rs.set_state(state)
        F = dr.f_table(table, accept, stop, count)
        prompts, q0 = prompts_for(F)
    want, cut = reference(stop, F, q0)
    assert cut >= 1  # the deadline is seen: at some draw E < ccount[q]
    off = np.zeros(K + 1, np.uint64)
    off[1:] = np.cumsum(lengths)
    for name, arr in (("why", Why), ("by", by), ("hs", Hs), ("u", u), ("off", off), ("tab", table),
                      ("cnt", cr.counts(table).astype(np.uint16)), ("q", q0.astype(np.int32)), ("acc", accept),
                      ("frows", dr.pack_rows(F[:count])),
                      ("prompts", np.concatenate(prompts) if off[-1] else np.zeros(1, np.uint8))):
        np.ascontiguousarray(arr).tofile(f"{d}/{name}.bin")
    subprocess.check_call([emulator, d, str(N), str(K), str(count), str(steps), str(sb), str(mode), repr(tau), str(keep_k),
                           str(int(top_p < 1.0)), repr(float(f32(top_p))), str(int(filtered)), str(stop)], timeout=300)
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
        assert end[s] == n_end and qend[s] == q, (s, end[s], n_end, qend[s], q)
        assert cr.walk(table, int(q0[s]), out[:n_end, s]) == q and accept[q]
        inputs = [int(b) for b in prompts[s]] + xs + [-1] * (steps + 1 - L - n_end)
        assert list(xlog[:, s]) == inputs, s
        assert np.array_equal(ho[s], Hs[L + n_end, s]), s
        stopped += n_end < count
    if stop >= 0:
        assert stopped >= 1
