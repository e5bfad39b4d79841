"""CPU: the logic of k_gen_head's FILTER instantiation (eigen-lstm_amd/csrc/heads/gen_head.inc) run on the
host -- the kernel's own text compiled with one thread per work-item (tests/gen_head_emulation.cc) -- against the float32
reference of tests/sampling_ref.py: bytes, kept counts, stop indices, the tail behind a stop byte, final states and the
inputs handed to the recurrence, bit for bit.  Logits are exact by construction (parameters and states are multiples of
1/16, N = 16), so they hold many ties, and expf is the C library's on both sides."""
import ctypes
import subprocess

import numpy as np
import pytest

import head_emulation
import sampling_ref as sr

N = 16
f32 = np.float32


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    return head_emulation.build(tmp_path_factory.mktemp("gen_head"), "gen_head_emulation")


def _reference_draw(z, mode, tau, top_k, top_p, filtered, u):
    """(byte, kept) of one draw, in the head's arithmetic"""
    if mode == 2:
        return int(np.argmax(z)), 1
    libm = ctypes.CDLL("libm.so.6")
    libm.expf.restype, libm.expf.argtypes = ctypes.c_float, [ctypes.c_float]
    zmax = z.max()
    e = np.array([libm.expf(float(z[m])) if mode == 0 else libm.expf(float(f32(f32(z[m] - zmax) / f32(tau)))) for m in range(256)], f32)
    s = f32(0)
    for m in range(256):
        s = f32(s + e[m])
    p = (e / s).astype(f32)
    if filtered:
        x, keep, _ = sr.draw32(z, p, top_k, top_p, u)
        return x, keep
    cdf = f32(0)
    for m in range(256):
        cdf = f32(cdf + p[m])
        if f32(u) < cdf:
            return m, 256
    return 0, 256


@pytest.mark.parametrize("K,sb,count,lengths,mode,tau,top_k,top_p,stop,seed", [
    (9, 1, 12, [0, 1, 3, 0, 2, 5, 0, 0, 1], 1, 0.8, 40, 0.9, 65, 1),     # both filters, tempered
    (10, 4, 10, [0, 2, 0, 1, 0, 0, 3, 0, 1, 0], 0, 1.0, 0, 0.9, -1, 2),  # nucleus alone, temperature 1, a partial group
    (20, 16, 8, [0, 1] * 10, 0, 1.0, 3, 1.0, 200, 3),                    # top-k alone with a stop byte, 16 streams a group
    (10, 4, 10, [0, 2, 0, 1, 0, 0, 3, 0, 1, 0], 2, 0.0, 40, 0.9, 100, 4),  # greedy ignores the filter, not the stop byte
    (20, 16, 8, [1, 0] * 10, 1, 1.5, 0, 1.0, 77, 5),                     # a stop byte alone
    (6, 1, 8, [0] * 6, 1, 0.7, 1, 1.0, -1, 6),                           # top_k = 1
])
def test_emulated_head_matches_the_reference(emulator, tmp_path, K, sb, count, lengths, mode, tau, top_k, top_p, stop, seed):
    rs = np.random.RandomState(seed)
    d = str(tmp_path)
    Why = (rs.randint(-32, 33, size=(N, 256)) / 16).astype(f32)  # [k][m]
    by = (rs.randint(-16, 17, size=256) / 16).astype(f32)
    steps = max(lengths) + count
    Hs = (rs.randint(-16, 17, size=(steps + 1, K, N)) / 16).astype(f32)  # the state before each step: any will do
    u = rs.random_sample((count, K))
    u[rs.randint(0, count), rs.randint(0, K)] = 1.5  # past every edge
    prompts = [rs.randint(0, 256, size=n).astype(np.uint8) for n in lengths]
    off = np.zeros(K + 1, np.uint64)
    off[1:] = np.cumsum(lengths)
    for name, arr in (("why", Why), ("by", by), ("hs", Hs), ("u", u), ("off", off),
                      ("prompts", np.concatenate(prompts) if off[-1] else np.zeros(1, np.uint8))):
        np.ascontiguousarray(arr).tofile(f"{d}/{name}.bin")
    keep_k = top_k if 1 <= top_k <= 255 else 256
    filtered = keep_k < 256 or top_p < 1.0
    subprocess.check_call([emulator, d, str(N), str(K), str(count), str(steps), str(sb), str(mode), repr(tau), str(keep_k),
                           str(int(top_p < 1.0)), repr(float(f32(top_p))), str(int(filtered)), str(stop)], timeout=300)
    out = np.fromfile(f"{d}/out.bin", np.uint8).reshape(count, K)
    kept = np.fromfile(f"{d}/kept.bin", np.uint16).reshape(count, K)
    end = np.fromfile(f"{d}/end.bin", np.int32)
    ho = np.fromfile(f"{d}/ho.bin", f32).reshape(K, N)
    xlog = np.fromfile(f"{d}/xlog.bin", np.int32).reshape(steps + 1, K)
    stopped = 0
    for s in range(K):
        L, n_end = lengths[s], count
        for t in range(steps + 1):
            if t < L:
                want = int(prompts[s][t])
            elif t - L < n_end:
                i = t - L
                z = (Why.T.astype(np.float64) @ Hs[t, s].astype(np.float64) + by).astype(f32)  # exact
                want, k = _reference_draw(z, mode, tau, top_k, top_p, filtered and mode != 2, u[i, s])
                assert (int(out[i, s]), int(kept[i, s])) == (want, k), (s, i)
                if want == stop:
                    n_end = i + 1
                    stopped += 1
            else:
                want = -1
            assert xlog[t, s] == want, (s, t)
        assert end[s] == n_end, s
        assert not out[n_end:, s].any() and not kept[n_end:, s].any(), s
        assert np.array_equal(ho[s], Hs[L + n_end, s]), s
    if seed in (3, 4):
        assert stopped >= 1  # (these seeds draw their stop byte)
