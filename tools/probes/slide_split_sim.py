"""The window slide split over workgroups that never wait for each other (csrc/kernels.hip, slide_body),
simulated on the CPU against the one-workgroup k_slide_window.

`reference` is k_slide_window statement by statement.  `split` runs the roles of the carried slide -- one owner and any number
of index workgroups -- in an arbitrary order, each reading only the state as it was BEFORE the launch where the kernel's
rule says so: the old cursors and head (double-buffered: the owner writes the other half) and the ring rows the owner does
not write.  To show that the rule is respected, the owner's writes go to the live ring arrays first or last (`owner_first`):
the result must not depend on it, and must equal the reference bit for bit.
"""
import numpy as np


def reference(text, pos, Xr, Tr, head, S, B, stride):
    pos, Xr, Tr = pos.copy(), Xr.copy(), Tr.copy()
    for b in range(B):
        p, hd = int(pos[b]), head
        for _ in range(stride):
            hd = (hd + 1) % S
            last, prev = (hd + S - 1) % S, (hd + S - 2) % S
            event = int(text[p])
            p += 1
            if p >= len(text):
                p = S
            Tr[last, b] = event
            Xr[last, b] = Tr[prev, b]
        pos[b] = p
    head = (head + stride) % S
    rows = (head + np.arange(S)) % S
    return pos, Xr, Tr, head, Xr[rows].copy(), Tr[rows].copy()


def _owner(text, pos, Xr, Tr, head, S, B, stride):
    """writes: pos_out, head_out, ring rows head .. head+stride-1"""
    pos_out = pos.copy()
    newest = (head + S - 1) % S
    for b in range(B):
        p, x = int(pos[b]), int(Tr[newest, b])
        for k in range(stride):
            last = (head + k) % S
            event = int(text[p])
            p += 1
            if p >= len(text):
                p = S
            Tr[last, b] = event
            Xr[last, b] = x
            x = event
        pos_out[b] = p
    return pos_out, (head + stride) % S


def _index(text, pos, Xr, Tr, head, S, B, stride, xi, ti, lo, hi):
    """flat entries [lo, hi) of the new window from the old cursors, the old head and the rows the owner leaves alone"""
    keep, newest = S - stride, (head + S - 1) % S
    for i in range(lo, hi):
        t, b = divmod(i, B)
        if t < keep:
            row = (head + stride + t) % S
            x, tg = Xr[row, b], Tr[row, b]
        else:
            p, x, tg = int(pos[b]), int(Tr[newest, b]), 0
            for k in range(t - keep + 1):
                if k > 0:
                    x = tg
                tg = int(text[p])
                p += 1
                if p >= len(text):
                    p = S
        xi[i], ti[i] = x, tg


def split(text, pos, Xr, Tr, head, S, B, stride, n_index, owner_first, order_seed=0):
    Xr, Tr = Xr.copy(), Tr.copy()
    xi, ti = np.empty(S * B, np.int64), np.empty(S * B, np.int64)
    chunks = np.array_split(np.arange(S * B), n_index)
    order = np.random.RandomState(order_seed).permutation(n_index)
    if owner_first:
        pos_out, head_out = _owner(text, pos, Xr, Tr, head, S, B, stride)
    for c in order:
        if chunks[c].size:
            _index(text, pos, Xr, Tr, head, S, B, stride, xi, ti, int(chunks[c][0]), int(chunks[c][-1]) + 1)
    if not owner_first:
        pos_out, head_out = _owner(text, pos, Xr, Tr, head, S, B, stride)
    return pos_out, Xr, Tr, head_out, xi.reshape(S, B), ti.reshape(S, B)


def run(S, B, stride, text_len, windows, n_index, seed=0):
    """`windows` slides in a row by both; returns the number compared (raises on the first difference)."""
    rs = np.random.RandomState(seed)
    text = rs.randint(0, 256, text_len)
    pos = S + rs.randint(0, text_len - S, B)
    state = [pos.astype(np.int64), np.full((S, B), -1, np.int64), np.full((S, B), -1, np.int64), int(rs.randint(S))]
    for w in range(windows):
        want = reference(text, *state, S, B, stride)
        for owner_first in (True, False):
            got = split(text, *state, S, B, stride, n_index, owner_first, order_seed=w)
            for name, a, b in zip(("pos", "Xr", "Tr", "head", "xi", "ti"), want, got):
                if not np.array_equal(a, b):
                    raise AssertionError(f"S={S} B={B} stride={stride} len={text_len} window {w} owner_first={owner_first}: {name}")
        state = list(want[:4])
    return windows


if __name__ == "__main__":
    n = 0
    for S, B, stride, L in ((100, 64, 1, 5000), (20, 12, 3, 400), (16, 20, 1, 21), (16, 20, 3, 20), (5, 3, 4, 9)):
        n += run(S, B, stride, L, 3 * S, n_index=7)
    print(f"{n} slides: the split slide equals k_slide_window")
