"""CPU: the logic of k_beam_head (eigen-lstm_amd/csrc/heads/beam_head.inc) run on the host -- the kernel's own
text and the real lse_surprisal compiled with one thread per work-item (tests/beam_head_emulation.cc) -- against beam32's
selection (tests/beam_ref.py): tables, costs, lengths, finished flags, next inputs and the gather of the states, bit for
bit.  Logits are exact by construction (parameters and states are multiples of 1/16, N = 16) and slots often share a state,
so costs tie inside a parent and across parents; expf and log2f are the C library's on both sides."""
import subprocess

import numpy as np
import pytest

import beam_ref as br
import head_emulation

N = 16
f32 = np.float32


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    return head_emulation.build(tmp_path_factory.mktemp("beam_head"), "beam_head_emulation")


def _reference(Why, by, Hs, lengths, K, W, count, stop):
    """per stream: a list over steps of None (no selection) or select32's result on that step's states"""
    res = []
    for s in range(K):
        cost, length, fin, rows = [0.0] + [br.INF] * (W - 1), [0] * W, [False] * W, []
        for t in range(Hs.shape[0]):
            if not lengths[s] <= t < lengths[s] + count:
                rows.append(None)
                continue
            z = (Hs[t, s * W:(s + 1) * W].astype(np.float64) @ Why.astype(np.float64) + by).astype(f32)  # exact
            sel = br.select32(z, cost, length, fin, W, stop)
            cost, length, fin = sel[2], sel[3], sel[4]
            rows.append(sel)
        res.append(rows)
    return res


@pytest.mark.parametrize("K,W,count,lengths,seed", [
    (3, 1, 6, [0, 2, 1], 1),
    (3, 4, 6, [1, 0, 3], 2),
    (2, 5, 5, [0, 1], 3),      # beams that are no power of two: the LDS stride is W, three registers idle
    (2, 32, 4, [1, 0], 4),
])
def test_emulated_head_matches_beam32(emulator, tmp_path, K, W, count, lengths, seed):
    rs = np.random.RandomState(seed)
    d = str(tmp_path)
    cols, steps = K * W, max(lengths) + count
    Why = (rs.randint(-32, 33, size=(N, 256)) / 16).astype(f32)  # [k][m]
    Why[:, 200:] = Why[:, 100:156]                               # 56 pairs of bytes with equal logits in every state
    by = (rs.randint(-16, 17, size=256) / 16).astype(f32)
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
    # the stop byte: one the unstopped search selects early in stream 0, so that slots finish while others live
    free = _reference(Why, by, Hs, lengths, K, W, count, -1)
    stop = free[0][lengths[0] + 1][1][0]
    for name, arr in (("why", Why), ("by", by), ("hs", Hs), ("cs", Cs), ("off", off),
                      ("prompts", np.concatenate(prompts) if off[-1] else np.zeros(1, np.uint8))):
        np.ascontiguousarray(arr).tofile(f"{d}/{name}.bin")
    subprocess.check_call([emulator, d, str(N), str(K), str(W), str(count), str(steps), str(stop)], timeout=600)
    tp = np.fromfile(f"{d}/tp.bin", np.uint8).reshape(count, cols)
    tb = np.fromfile(f"{d}/tb.bin", np.uint8).reshape(count, cols)
    xlog = np.fromfile(f"{d}/xlog.bin", np.int32).reshape(steps, cols)
    costlog = np.fromfile(f"{d}/costlog.bin", np.float64).reshape(steps, cols)
    lenlog = np.fromfile(f"{d}/lenlog.bin", np.int32).reshape(steps, cols)
    finlog = np.fromfile(f"{d}/finlog.bin", np.int32).reshape(steps, cols)
    hr = np.fromfile(f"{d}/hr.bin", f32).reshape(steps, cols, N)
    cr = np.fromfile(f"{d}/cr.bin", f32).reshape(steps, cols, N)
    ref = _reference(Why, by, Hs, lengths, K, W, count, stop)
    finished = 0
    for s in range(K):
        sl = slice(s * W, (s + 1) * W)
        for t in range(steps):
            sel = ref[s][t]
            if sel is None:
                want_x = [int(prompts[s][t])] * W if t < lengths[s] else [-1] * W
                assert list(xlog[t, sl]) == want_x, (s, t)
                assert np.array_equal(hr[t, sl], Hs[t, sl]) and np.array_equal(cr[t, sl], Cs[t, sl]), (s, t)
                continue
            par, byt, cost, length, fin, xs, _ = sel
            i = t - lengths[s]
            assert list(tp[i, sl]) == par and list(tb[i, sl]) == byt, (s, i, list(tp[i, sl]), par, list(tb[i, sl]), byt)
            assert costlog[t, sl].tobytes() == np.array(cost, np.float64).tobytes(), (s, i)
            assert list(lenlog[t, sl]) == length and [bool(f) for f in finlog[t, sl]] == fin, (s, i)
            assert list(xlog[t, sl]) == xs, (s, i)
            assert np.array_equal(hr[t, sl], Hs[t, sl][par]) and np.array_equal(cr[t, sl], Cs[t, sl][par]), (s, i)
            finished += sum(fin)
    assert finished >= 1  # (the stop byte was selected)
