"""The constraint of lstm_hip_generate_constrained (include/lstm_hip.h) in numpy: a byte automaton
`table` ((states, 256) uint16: the state after byte b in state q, FORBID where b is forbidden) masks the logits of a draw,
and the sampling rules of tests/sampling_ref.py run on the masked logits with keep capped by the state's allowed count.

draw32 follows the device's arithmetic (float32, sequential sums, the C library's expf) from the logits on; filter64 states
the same rule in float64 for comparisons against the oracle."""
import ctypes

import numpy as np

import sampling_ref as sr

M = 256
FORBID = 0xFFFF
f32 = np.float32
# one-byte prompts that leave the UTF-8 automaton (lstm_hip_dfa_utf8) in states 0..7
UTF8_STATE_PROMPTS = (0x41, 0xC3, 0xE1, 0xE0, 0xED, 0xF1, 0xF0, 0xF4)

_libm = ctypes.CDLL("libm.so.6")
_libm.expf.restype, _libm.expf.argtypes = ctypes.c_float, [ctypes.c_float]


def counts(table):
    """A_q: allowed bytes per state"""
    return (np.asarray(table) != FORBID).sum(axis=1)


def walk(table, q, data):
    """the state after `data` from state q, or None where the table rejects a byte"""
    for b in bytes(data):
        q = int(table[q][b])
        if q == FORBID:
            return None
    return q


def capped_top_k(table, q, top_k):
    """min(keep_k, A_q) as a top_k argument of tests/sampling_ref.py (0: off, when it is 256)"""
    k = min(top_k if 1 <= top_k <= 255 else 256, int((table[q] != FORBID).sum()))
    return k if k <= 255 else 0


def draw32(z, table, q, mode, tau, top_k, top_p, u):
    """One constrained draw as the head computes it from the float32 logits z: returns (byte, kept).  mode 0: expf(z)
    unshifted, 1: expf((z - max) / tau), 2: greedy."""
    ok = np.asarray(table[q]) != FORBID
    zm = np.where(ok, z, f32(-np.inf)).astype(f32)
    if mode == 2:
        return int(np.argmax(zm)), 1
    zmax = zm.max()
    with np.errstate(invalid="ignore"):
        e = np.array([_libm.expf(float(zm[m])) if mode == 0 else _libm.expf(float(f32(f32(zm[m] - zmax) / f32(tau))))
                      for m in range(M)], f32)
    s = f32(0)
    for m in range(M):
        s = f32(s + e[m])
    p = (e / s).astype(f32)
    x, keep, _ = sr.draw32(zm, p, capped_top_k(table, q, top_k), top_p, u)
    return x, keep


def masked64(p1, table, q, tau):
    """(key, p) of one draw in float64 from the oracle's temperature-1 probabilities p1: the ranking key (forbidden bytes
    last) and the tempered distribution over the allowed bytes, renormalised"""
    ok = np.asarray(table[q]) != FORBID
    p1 = np.asarray(p1, np.float64)
    t = np.where(ok, p1, 0.0) ** (1.0 / tau)
    return np.where(ok, p1, -1.0), t / t.sum()


def filter64(p1, table, q, tau, top_k, top_p):
    """(keep, kept mask, renormalised p'', p before the filter) of a constrained tempered draw, in float64"""
    key, p = masked64(p1, table, q, tau)
    keep, mask, pp = sr.filter64(key, p, capped_top_k(table, q, top_k), top_p)
    return keep, mask, pp, p


def ambiguous(p, table, q, top_k, top_p):
    """sampling_ref.ambiguous under the capped keep (p: the masked, renormalised distribution)"""
    return sr.ambiguous(p, capped_top_k(table, q, top_k), top_p)


# ---- the case of the GPU oracle comparison (tests/test_constraint.py) and of its CPU control (tests/test_constraint_cpu.py):
# sampling_ref.oracle_case()'s parameters and draws with eight streams, one per state of the UTF-8 automaton
ORACLE_STREAMS = len(UTF8_STATE_PROMPTS)
ORACLE_SETTINGS = (  # (top_k, top_p, temperature)
    (0, 1.0, 1.0),
    (0, 1.0, 0.8),
    (40, 0.9, 1.0),
    (40, 0.9, 0.8),
)


def oracle_case():
    """(P, prompts, u): sampling_ref.oracle_case()'s parameters, the eight one-byte prompts, draws [count, 8]"""
    P, _, _ = sr.oracle_case()
    prompts = [np.array([b], np.uint8) for b in UTF8_STATE_PROMPTS]
    u = np.random.RandomState(43).random_sample((sr.ORACLE_COUNT, ORACLE_STREAMS))
    return P, prompts, u
