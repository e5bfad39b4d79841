"""CPU: the logic of k_score_head (eigen-lstm_amd/csrc/heads/score_head.inc) run on the host -- the kernel's
own text compiled with one thread per work-item (tests/score_head_emulation.cc) -- against the float32 statement of the rule
in tests/score_ref.py: surprisal, entropy, rank, alternatives and their bits, the streams' bits, the inputs handed to the
recurrence and the final states, bit for bit.  Logits are exact by construction (parameters and states are multiples of 1/16,
N = 16), so they hold many ties, and expf and log2f are the C library's on both sides."""
import subprocess

import numpy as np
import pytest

import head_emulation
import score_ref as sc

N = 16
f32 = np.float32


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    return head_emulation.build(tmp_path_factory.mktemp("score_head"), "score_head_emulation")


def _table(rs):
    """six states: 0 allows every byte, 1 exactly one, the others 3..120 of them; every allowed byte leads to some state"""
    Q = 6
    table = np.full((Q, 256), sc.FORBID, np.uint16)
    sizes = [256, 1, 3, 17, 64, 120]
    for q in range(Q):
        allowed = rs.choice(256, sizes[q], replace=False)
        table[q, allowed] = rs.randint(0, Q, size=sizes[q])
    table[0, ::3] = 1  # (state 1, with its one byte, is reached often)
    return table


@pytest.mark.parametrize("K,sb,lengths,stable,first,top_n,detail,constrain,seed", [
    (5, 1, [0, 1, 7, 2, 4], 0, 0, 0, 0, 0, 1),                 # the plain instantiation
    (5, 1, [0, 1, 7, 2, 4], 1, 1, 8, 1, 1, 2),                 # everything on, one stream per group
    (10, 4, [3, 0, 1, 6, 2, 0, 5, 1, 4, 2], 0, 1, 1, 1, 0, 3),  # groups of 4, a partial last group
    (10, 4, [3, 0, 1, 6, 2, 0, 5, 1, 4, 2], 1, 0, 8, 1, 1, 4),
    (10, 4, [3, 0, 1, 6, 2, 0, 5, 1, 4, 2], 0, 0, 0, 1, 1, 5),  # rank alone, under a table
    (20, 16, [2, 0, 1, 5] * 5, 0, 1, 8, 1, 1, 6),               # groups of 16 (partial), unshifted, top_n above A_q
    (20, 16, [1, 3, 0, 4] * 5, 1, 1, 0, 0, 1, 7),               # the plain instantiation under a table
    (20, 16, [2, 0, 1, 5] * 5, 1, 0, 1, 1, 0, 8),
])
def test_emulated_score_head_matches_the_statement(emulator, tmp_path, K, sb, lengths, stable, first, top_n, detail, constrain, seed):
    rs = np.random.RandomState(seed)
    d = str(tmp_path)
    table = _table(rs)
    Q = table.shape[0]
    Why = (rs.randint(-32, 33, size=(N, 256)) / 16).astype(f32)  # [k][m]
    by = (rs.randint(-16, 17, size=256) / 16).astype(f32)
    steps = max(lengths)
    Hs = (rs.randint(-16, 17, size=(steps + 1, K, N)) / 16).astype(f32)  # the state before each step: any will do
    start = rs.randint(0, Q, size=K).astype(np.int32)
    start[:3] = (1, 0, 5)
    texts, qpos = [], []
    for s, n in enumerate(lengths):  # texts the table accepts (the head itself does not look: the API walks them)
        q, p = int(start[s]), []
        for _ in range(n):
            b = int(rs.choice(np.nonzero(table[q] != sc.FORBID)[0]))
            p.append(b)
            qpos.append(q)
            q = int(table[q, b])
        texts.append(np.array(p, np.uint8))
    off = np.zeros(K + 1, np.uint64)
    off[1:] = np.cumsum(lengths)
    total = int(off[-1])
    for name, arr in (("why", Why), ("by", by), ("hs", Hs), ("off", off), ("tab", table),
                      ("qpos", np.array(qpos + [0], np.uint16)), ("text", np.concatenate(texts + [np.zeros(1, np.uint8)]))):
        np.ascontiguousarray(arr).tofile(f"{d}/{name}.bin")
    subprocess.check_call([emulator, d, str(N), str(K), str(steps), str(sb), str(stable), str(detail), str(constrain), str(first),
                           str(top_n)], timeout=300)
    sur = np.fromfile(f"{d}/surprisal.bin", f32)
    ent = np.fromfile(f"{d}/entropy.bin", f32)
    rank = np.fromfile(f"{d}/rank.bin", np.uint8)
    tby = np.fromfile(f"{d}/top_byte.bin", np.uint8).reshape(total, top_n)
    tbi = np.fromfile(f"{d}/top_bits.bin", f32).reshape(total, top_n)
    bits = np.fromfile(f"{d}/bits.bin", np.float64)
    ho = np.fromfile(f"{d}/ho.bin", f32).reshape(K, N)
    xlog = np.fromfile(f"{d}/xlog.bin", np.int32).reshape(steps + 1, K)
    scored = past_allowed = one_byte = ties = 0
    for s in range(K):
        L = lengths[s]
        assert list(xlog[:, s]) == [int(b) for b in texts[s]] + [-1] * (steps + 1 - L), s
        assert np.array_equal(ho[s], Hs[L, s]), s
        want_bits = 0.0
        for j in range(L):
            pos = int(off[s]) + j
            if j == 0 and not first:
                assert sur[pos] == 0 and ent[pos] == 0 and rank[pos] == 0 and not tby[pos].any() and not tbi[pos].any(), (s, j)
                continue
            z = (Why.T.astype(np.float64) @ Hs[j, s].astype(np.float64) + by).astype(f32)  # exact
            ok = table[qpos[pos]] != sc.FORBID if constrain else None
            w_sur, w_ent, w_rank, w_tby, w_tbi = sc.statement32(z, texts[s][j], bool(stable), ok, top_n)
            assert np.isfinite(w_sur) and np.isfinite(w_ent)
            assert sur[pos].tobytes() == f32(w_sur).tobytes() and ent[pos].tobytes() == f32(w_ent).tobytes(), (s, j, sur[pos], w_sur, ent[pos], w_ent)
            want_bits += float(w_sur)
            scored += 1
            ties += np.unique(z).size < 256
            if detail:
                assert rank[pos] == w_rank, (s, j)
                assert np.array_equal(tby[pos], w_tby) and tbi[pos].tobytes() == w_tbi.astype(f32).tobytes(), (s, j, tby[pos], w_tby)
                if constrain:
                    A = int(ok.sum())
                    assert rank[pos] < A
                    assert np.isinf(tbi[pos][A:]).all() and np.isfinite(tbi[pos][:A]).all()
                    assert list(tby[pos][A:]) == list(np.nonzero(~ok)[0][:max(top_n - A, 0)])  # the forbidden bytes, in index order
                    past_allowed += top_n > A
                    one_byte += A == 1
            else:
                assert rank[pos] == 0
        assert bits[s] == want_bits, s
    assert scored >= 10 and ties == scored
    if detail and constrain and top_n == 8:
        assert past_allowed >= 1 and one_byte >= 1  # top_n passes the allowed count of the one-byte state
