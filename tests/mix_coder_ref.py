"""The rule of lstm_hip_encode_mixed / lstm_hip_decode_mixed (include/lstm_hip.h) in numpy, from every
model's float32 logits on: the static coder on a log-linear mix whose weights each stream carries and, with rate > 0, learns.

Models 0..G are the main model and the G guides.  A stream holds v [1 + G] float32, at first the call's weights.  Byte j is
coded under z' = guided_ref.mix32(z^0, (z^1..z^G), v_0, (v_1..v_G)), the table is code_table_ref.table32(z'), the coder is
range_coder_ref's.  After byte x has been coded or decoded (the stream's last byte too), with rate > 0:

    d_m    = fl(fl((float)q_m / (float)T) - (m == x ? 1 : 0))
    grad_k = the sequential float32 sum over m = 0..255 of fl(d_m * z^k_m)
    v_k    = fl(v_k - fl((float)rate * grad_k))

update32 states that; grad64 states what it approximates, E_q[z^k] - z^k_x, in float64, and grad_bound the distance a float32
evaluation may have from it.

Where grad_bound comes from, with u = 2^-24 and a_m = q_m / T, d*_m = a_m - [m == x] exact:
  * fl(q_m / T) = a_m (1 + e), |e| <= u (q_m and T are integers below 2^24, so their conversions are exact): an error a_m u.
  * the subtraction is exact for m != x; for m == x it rounds once more: |d*_x| u.  So |d_m - d*_m| <= (a_m + |d*_m|) u.
  * the product fl(d_m z_m) adds |d_m z_m| u.
  * the sequential sum of 256 terms adds at most 255 u times the sum of the terms' magnitudes (first order).
  So |grad32 - grad64| <= u SUM_m |z_m| (a_m + 257 |d*_m|) to first order; the bound uses 258 for the terms of order u^2
  (256 u < 2^-16 of the first-order term) and adds 256 * 2^-149 for products that underflow.
The mutants (sign, order, early, mix_left) are for the control in tests/test_mix_coder_cpu.py."""
import numpy as np

import code_table_ref as ct
import guided_ref as gr
import range_coder_ref as rc

M = 256
f32 = np.float32


def mix32(zs, v, mix_left=False):
    """z' [256] float32 from the members' logits zs ([1 + G][256]) under the weights v ([1 + G]).
    mix_left: a mutant -- ((v_0 z^0 + v_1 z^1) + v_2 z^2) .. , the main model's term first"""
    if mix_left:
        with np.errstate(invalid="ignore", over="ignore"):
            acc = (f32(v[0]) * np.asarray(zs[0], f32)).astype(f32)
            for k in range(1, len(zs)):
                acc = (acc + (f32(v[k]) * np.asarray(zs[k], f32)).astype(f32)).astype(f32)
            return acc
    return gr.mix32(zs[0], list(zs[1:]), v[0], list(v[1:]))


def update32(v, q, T, zs, x, rate, sign=1, reverse=False):
    """the weights after byte x: v [1 + G] float32 from the table (q [256], T) the byte was coded under and the members' logits.
    sign = -1 and reverse (the sum from m = 255 down) are mutants"""
    v = np.array(v, f32)
    if f32(rate) == 0:
        return v
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        d = (np.asarray(q).astype(f32) / f32(T)).astype(f32)
        hot = np.zeros(M, f32)
        hot[int(x)] = 1
        d = (d - hot).astype(f32)
        for k in range(len(v)):
            terms = (d * np.asarray(zs[k], f32)).astype(f32)
            if reverse:
                terms = terms[::-1]
            grad = np.add.accumulate(terms, dtype=f32)[-1]  # (sequential in float32)
            step = f32(f32(rate) * grad)
            v[k] = f32(v[k] - step) if sign > 0 else f32(v[k] + step)
    return v


def grad64(q, T, zs, x):
    """E_q[z^k] - z^k_x for every member, in float64"""
    a = np.asarray(q, np.float64) / float(T)
    return np.array([float(np.dot(a, np.asarray(z, np.float64)) - float(z[int(x)])) for z in zs])


def grad32(q, T, zs, x):
    """the float32 gradient of update32, [1 + G]"""
    zero = np.zeros(len(zs), f32)
    return (zero - update32(zero, q, T, zs, x, 1.0)).astype(f32)  # (0 - (0 - 1 * grad) = grad, exactly)


def grad_bound(q, T, zs, x):
    a = np.asarray(q, np.float64) / float(T)
    d = a.copy()
    d[int(x)] -= 1.0
    return np.array([2.0 ** -24 * float(np.sum(np.abs(np.asarray(z, np.float64)) * (a + 258.0 * np.abs(d)))) + 256 * 2.0 ** -149
                     for z in zs])


def steps(text, zs_of, v0, rate, early=False, **mutant):
    """One stream coded byte by byte.  zs_of(j) gives the members' logits for byte j.  Yields nothing; returns
    (trace [n][3] uint32, w_trace [n][1 + G] float32, w_out [1 + G] float32, bits float, tables list of q).
    early: a mutant -- the update is taken before the byte is coded, so the byte is coded under weights that have seen it"""
    mix_left = mutant.pop("mix_left", False)
    v = np.array(v0, f32)
    trace, w_trace, tables, bits = [], [], [], 0.0
    for j, x in enumerate(text):
        zs = zs_of(j)
        if early:
            q0, _, T0 = ct.table32(mix32(zs, v, mix_left))
            v = update32(v, q0, T0, zs, x, rate, **mutant)
        w_trace.append(v.copy())
        q, cum, T = ct.table32(mix32(zs, v, mix_left))
        trace.append((int(cum[x]), int(q[x]), T))
        tables.append(q)
        bits += -np.log2(float(q[x]) / float(T))
        if not early:
            v = update32(v, q, T, zs, x, rate, **mutant)
    n = len(text)
    return (np.array(trace, np.uint32).reshape(n, 3), np.array(w_trace, f32).reshape(n, len(v)), v, bits, tables)


def encode(text, zs_of, v0, rate, **mutant):
    """(code bytes, trace, w_trace, w_out, bits)"""
    trace, w_trace, w_out, bits, _ = steps(text, zs_of, v0, rate, **mutant)
    return rc.encode(trace), trace, w_trace, w_out, bits


def decode(code, n, zs_of, v0, rate):
    """the decoder: it holds the weights of the bytes it has decoded and nothing else.  (text bytes, w_out)"""
    import bisect

    state = {"v": np.array(v0, f32)}

    def model(j):
        zs = zs_of(j)
        q, cum, T = ct.table32(mix32(zs, state["v"]))
        cl = [int(c) for c in cum]

        def find(val):
            m = bisect.bisect_right(cl, val) - 1
            m = min(m, M - 1)
            state["v"] = update32(state["v"], q, T, zs, m, rate)
            return m, cl[m], cl[m + 1] - cl[m]

        return T, find

    out = rc.decode(code, n, model)
    return bytes(out), state["v"]
