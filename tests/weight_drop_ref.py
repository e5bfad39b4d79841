"""The weight-drop rule of include/lstm_hip.h (lstm_hip_set_weight_drop) transcribed into NumPy: Philox4x32-10 over the
element numbers of the logical 4N x N matrix U, the keep decision and the scale.  The tests compare the library's CPU entry
point and the device's masks against this file; nothing here calls the library."""
import functools
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """One call on Python integers: counter (c0, c1, c2, c3), key (k0, k1) -> four 32-bit output words."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0, c1, c2, c3


def _philox_quads(q, seed, t):
    """The same rounds, vectorised over quad numbers q (uint64 array) -> uint32 array [len(q), 4]."""
    q = np.asarray(q, np.uint64)
    m32 = np.uint64(MASK32)
    s32 = np.uint64(32)
    c0, c1 = q & m32, q >> s32
    c2 = np.full_like(q, t & MASK32)
    c3 = np.full_like(q, (t >> 32) & MASK32)
    k0, k1 = seed & MASK32, (seed >> 32) & MASK32
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2  # 32 x 32 bits: fits 64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def threshold(rate):
    return int(math.floor(rate * 4294967296.0))


def scale(rate):
    return np.float32(1.0 / (1.0 - rate))


@functools.lru_cache(maxsize=32)
def words(N, seed, t):
    """The random word of every element e = r + 4N k of the logical matrix, as uint32 [4N * N] (shared: read only)."""
    n = 4 * N * N
    quads = _philox_quads(np.arange((n + 3) // 4, dtype=np.uint64), seed, t)
    return quads.reshape(-1)[:n]


def mask(N, rate, seed=0, t=0):
    """keep as a bool array [4N, N]: keep[r, k] <=> word(r + 4N k) >= floor(rate * 2^32)."""
    return (words(N, seed, t) >= np.uint32(threshold(rate))).reshape(N, 4 * N).T


def flat_mask(N, rate, seed=0, t=0):
    """keep in the order of the U range of the flat parameter block (column-major): [4N * N]."""
    return words(N, seed, t) >= np.uint32(threshold(rate))


def apply(u, keep, rate):
    """where(keep, u * s, +0) on float32, as the device writes it."""
    u = np.asarray(u, np.float32)
    return np.where(keep, u * scale(rate), np.float32(0.0)).astype(np.float32)
