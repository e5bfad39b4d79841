"""CPU: the logic of k_gen_head's CONSTRAIN instantiation (eigen-lstm_amd/csrc/heads/gen_head.inc) run on
the host -- the kernel's own text compiled with one thread per work-item (tests/gen_head_constrained_emulation.cc) --
against the float32 reference of tests/constraint_ref.py: bytes, kept counts, stop indices, end states, final states and the
inputs handed to the recurrence, bit for bit.  Logits are exact by construction (parameters and states are multiples of
1/16, N = 16), so they hold many ties, and expf is the C library's on both sides."""
import subprocess

import numpy as np
import pytest

import constraint_ref as cr
import head_emulation

N = 16
f32 = np.float32


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    return head_emulation.build(tmp_path_factory.mktemp("gen_head_constrained"), "gen_head_constrained_emulation")


def _table(rs):
    """six states: 0 allows every byte, 1 exactly one, the others 3..120 of them; every allowed byte leads to some state"""
    Q = 6
    table = np.full((Q, 256), cr.FORBID, np.uint16)
    sizes = [256, 1, 3, 17, 64, 120]
    for q in range(Q):
        allowed = rs.choice(256, sizes[q], replace=False)
        table[q, allowed] = rs.randint(0, Q, size=sizes[q])
    table[0, ::3] = 1  # (state 1 is reached often)
    return table


@pytest.mark.parametrize("K,sb,count,lengths,mode,tau,top_k,top_p,stop,seed", [
    (9, 1, 12, [0, 1, 3, 0, 2, 5, 0, 0, 1], 1, 0.8, 0, 1.0, -1, 1),       # the constraint alone, tempered
    (10, 4, 10, [0, 2, 0, 1, 0, 0, 3, 0, 1, 0], 0, 1.0, 0, 1.0, -1, 2),   # alone, temperature 1, a partial last group
    (20, 16, 8, [0, 1] * 10, 0, 1.0, 3, 1.0, -1, 3),                      # with top-k, 16 streams a group (partial)
    (10, 4, 10, [0, 2, 0, 1, 0, 0, 3, 0, 1, 0], 1, 0.7, 40, 0.9, -1, 4),  # with both filters
    (20, 16, 8, [1, 0] * 10, 1, 1.5, 0, 0.8, None, 5),                    # nucleus and a stop byte (chosen from the draws)
    (10, 4, 10, [0, 2, 0, 1, 0, 0, 3, 0, 1, 0], 2, 0.0, 40, 0.9, None, 6),  # greedy: masked argmax, a stop byte
    (6, 1, 8, [0] * 6, 0, 1.0, 0, 1.0, None, 7),                          # a stop byte under the constraint alone
])
def test_emulated_constrained_head_matches_the_reference(emulator, tmp_path, K, sb, count, lengths, mode, tau, top_k, top_p, stop, seed):
    rs = np.random.RandomState(seed)
    d = str(tmp_path)
    table = _table(rs)
    Q = table.shape[0]
    Why = (rs.randint(-32, 33, size=(N, 256)) / 16).astype(f32)  # [k][m]
    by = (rs.randint(-16, 17, size=256) / 16).astype(f32)
    steps = max(lengths) + count
    Hs = (rs.randint(-16, 17, size=(steps + 1, K, N)) / 16).astype(f32)  # the state before each step: any will do
    u = rs.random_sample((count, K))
    u[rs.randint(0, count), rs.randint(0, K)] = 1.5  # past every edge
    start = rs.randint(0, Q, size=K).astype(np.int32)  # streams start in different states
    start[:3] = (1, 0, 5)
    assert len(set(start)) >= 3
    prompts, q0 = [], start.copy()
    for s, n in enumerate(lengths):  # prompts the table accepts (the head itself does not look: the API walks them)
        p = []
        for _ in range(n):
            b = int(rs.choice(np.nonzero(table[q0[s]] != cr.FORBID)[0]))
            p.append(b)
            q0[s] = table[q0[s], b]
        prompts.append(np.array(p, np.uint8))
    off = np.zeros(K + 1, np.uint64)
    off[1:] = np.cumsum(lengths)
    keep_k = top_k if 1 <= top_k <= 255 else 256
    filtered = keep_k < 256 or top_p < 1.0

    def reference(stop_byte):
        """per stream (bytes, kept, end index, end state)"""
        res = []
        for s in range(K):
            L, q, xs, ks, n_end = lengths[s], int(q0[s]), [], [], count
            for i in range(count):
                z = (Why.T.astype(np.float64) @ Hs[L + i, s].astype(np.float64) + by).astype(f32)  # exact
                x, k = cr.draw32(z, table, q, mode, tau, top_k, top_p, u[i, s])
                assert table[q, x] != cr.FORBID
                xs.append(x)
                ks.append(k)
                q = int(table[q, x])
                if x == stop_byte:
                    n_end = i + 1
                    break
            res.append((xs, ks, n_end, q))
        return res

    if stop is None:  # a byte that some stream draws after its first draw, so that the stop index is exercised
        free = reference(-1)
        late = [x for xs, _, _, _ in free for x in xs[1:]]
        stop = int(np.bincount(late, minlength=256).argmax())
    want = reference(stop)
    for name, arr in (("why", Why), ("by", by), ("hs", Hs), ("u", u), ("off", off), ("tab", table),
                      ("cnt", cr.counts(table).astype(np.uint16)), ("q", q0.astype(np.int32)),
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
    A = cr.counts(table)
    stopped, single, past_edge = 0, 0, 0
    for s in range(K):
        xs, ks, n_end, q = want[s]
        L = lengths[s]
        assert list(out[:n_end, s]) == xs and list(kept[:n_end, s]) == ks, s
        assert not out[n_end:, s].any() and not kept[n_end:, s].any(), s
        assert end[s] == n_end and qend[s] == q, (s, end[s], n_end, qend[s], q)
        assert cr.walk(table, int(q0[s]), out[:n_end, s]) == q  # the output is accepted by the table
        inputs = [int(b) for b in prompts[s]] + xs + [-1] * (steps + 1 - L - n_end)
        assert list(xlog[:, s]) == inputs, s
        assert np.array_equal(ho[s], Hs[L + n_end, s]), s
        stopped += n_end < count
        qq = int(q0[s])
        for i, x in enumerate(xs):
            assert ks[i] <= A[qq]
            single += A[qq] == 1
            past_edge += u[i, s] == 1.5
            qq = int(table[qq, x])
    assert single >= 1  # a draw in the state with one allowed byte
    if stop >= 0:
        assert stopped >= 1
    if seed in (1, 2, 3, 4):
        assert past_edge == 1  # the draw past every edge was made (no stop byte in these cases)
