"""The frequency table of the model-driven coder (k_code_head, eigen-lstm_amd/csrc/heads/code_head.inc; DESIGN.md section
3.6) from the float32 logits on, stated twice.

table32 follows the device's arithmetic: max z, then e_m = expf(z_m - max z) with the C library's expf (the one the host
emulation of the head calls), s summed in index order, and p_m = e_m / s, v_m = p_m * 65024.0f, q_m = 1 + (uint32)v_m, each one
float32 operation.  A NaN anywhere gives q = 1 (every comparison with it is false).  The host emulation is held to it bit
for bit.

interval64 states the rule in float64, v64_m = 65024 exp(d_m) / sum_k exp(d_k) with d = z - max z, and gives the interval a
float32 evaluation of the rule may land in.  A device q_m is acceptable iff

    floor(v64_m (1 - DELTA)) <= q_m - 1 <= floor(v64_m (1 + DELTA)),     DELTA = (431 + 4 U) 2^-24.

Where DELTA comes from, with u = 2^-24 the unit roundoff of float32:
  * d_m = fl(z_m - max z) carries a relative error u, an absolute one of |d_m| u, which is a relative error |d_m| u of e_m.
    A term with d < -87 has v < 65024 e^-87 << 1 and contributes q = 1 whatever its error, and nothing visible to s, so
    |d| <= 87 where it matters: 87 u.
  * expf is within U ulp of the exact value: a relative 2 U u.
  * the sequential sum of 256 positive terms adds a relative 255 u to s.
  * the division and the product with 65024 add u each.
  * the numerator e_m carries 87 u + 2 U u, the denominator s the same (every term does) plus 255 u, and the errors of a
    quotient add: 2 (87 + 2 U) + 255 + 2 = 431 + 4 U units of u.
U is the largest ulp error of the device's expf.  The ROCm installation this was written against ships no documentation
that states one, so U = 2 is used: the fallback, not a documented figure.  At the largest possible entry (v ~ 65024) the
interval is about +-2 counts; at small entries it is exact or +-1."""
import ctypes

import numpy as np

M = 256
SCALE = 65024.0
U = 2
DELTA = (431 + 4 * U) * 2.0 ** -24
f32 = np.float32

_libm = ctypes.CDLL("libm.so.6")
_libm.expf.restype, _libm.expf.argtypes = ctypes.c_float, [ctypes.c_float]


def table32(z):
    """(q [256], cum [257], T) from the float32 logits, as the device computes them"""
    z = np.asarray(z, f32)
    assert z.shape == (M,)
    zmax = z[0]
    for v in z[1:]:
        if v > zmax:
            zmax = v
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d = (z - zmax).astype(f32)
        e = np.array([_libm.expf(float(x)) for x in d], f32)
        s = f32(0.0)
        for x in e:
            s = f32(s + x)
        p = (e / s).astype(f32)
        v = (p * f32(SCALE)).astype(f32)
        whole = np.where(v >= f32(1.0), v, f32(0.0))  # (a NaN compares false)
    q = (1 + whole.astype(np.uint32)).astype(np.uint32)
    cum = np.zeros(M + 1, np.uint32)
    cum[1:] = np.cumsum(q, dtype=np.uint32)
    return q, cum, int(cum[M])


FLAT = (np.ones(M, np.uint32), np.arange(M + 1, dtype=np.uint32), M)  # the table of a row with a NaN


def statement64(z):
    """v64 [256]: 65024 times the softmax of the (float32, finite) logits, in float64"""
    z = np.asarray(z, np.float64)
    assert np.isfinite(z).all()
    e = np.exp(z - z.max())
    return SCALE * e / e.sum()


def interval64(z):
    """(lo [256], hi [256]): q_m - 1 must lie in [lo_m, hi_m]"""
    v = statement64(z)
    return np.floor(v * (1.0 - DELTA)).astype(np.int64), np.floor(v * (1.0 + DELTA)).astype(np.int64)


def outside(q, z):
    """the indices m whose q_m lies outside the interval of the float64 statement"""
    lo, hi = interval64(z)
    w = np.asarray(q, np.int64) - 1
    return np.nonzero((w < lo) | (w > hi))[0]
