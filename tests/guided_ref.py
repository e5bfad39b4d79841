"""The rule of lstm_hip_generate_guided / lstm_hip_score_guided (include/lstm_hip.h) in numpy: a
log-linear mix of the logits of models fed the same bytes, z' = a * z + sum_k b_k * z^k.

mix32 follows the device's arithmetic from every model's float32 logits on: the weights narrowed to float32, g = b_1 * z^1, then
g = g + b_k * z^k in index order, then a * z + g, every multiply and every add rounded on its own.  draw32 / statement32 then
hand the mixed logits to tests/logit_processor_ref.py and tests/score_ref.py, which state everything behind the mix.  mix64 /
filter64 state the same in float64 on probabilities, p ~ p_main^a * prod_k p_k^b_k, for comparisons against the oracle."""
import numpy as np

import logit_processor_ref as lr
import score_ref as sc

M = 256
f32 = np.float32


def guide_sum32(zs, weights, reverse=False):
    """g [256] float32: b_1 * z^1, then + b_k * z^k for k = 2.. in index order (reverse: a mutant for the control -- the last
    guide first)"""
    order = range(len(zs))[::-1] if reverse else range(len(zs))
    g = None
    for k in order:
        t = (f32(weights[k]) * np.asarray(zs[k], f32)).astype(f32)
        g = t if g is None else (g + t).astype(f32)
    return g


def mix32(z, zs, a, weights, reverse=False):
    """z' [256] float32 from the main model's logits z, the guides' logits zs and the weights (a, weights)"""
    with np.errstate(invalid="ignore", over="ignore"):
        g = guide_sum32(zs, weights, reverse)
        return ((f32(a) * np.asarray(z, f32)).astype(f32) + g).astype(f32)


def draw32(z, zs, a, weights, V, T, mode, tau, top_k, top_p, u, bias=None, min_p=0.0, n=0, after_bias=False):
    """One guided draw: logit_processor_ref.draw32 on the mixed logits -- (byte, kept, banned a valid byte, dropped).
    after_bias: a mutant for the control -- the bias goes to the main model's logits ahead of the mix."""
    if after_bias and bias is not None:
        return lr.draw32(mix32((np.asarray(z, f32) + np.asarray(bias, f32)).astype(f32), zs, a, weights), V, T, mode, tau, top_k,
                         top_p, u, None, min_p, n)
    return lr.draw32(mix32(z, zs, a, weights), V, T, mode, tau, top_k, top_p, u, bias, min_p, n)


def statement32(z, zs, a, weights, x, stable=False, ok=None, top_n=0):
    """One scored byte under the mix: score_ref.statement32 on the mixed logits (the constraint mask behind the mix)"""
    return sc.statement32(mix32(z, zs, a, weights), x, stable, ok, top_n)


def mix64(p_main, ps, a, weights):
    """p ~ p_main^a * prod_k p_k^b_k, normalised: the temperature-1 distribution of the mixed logits, in float64"""
    lg = a * np.log(np.asarray(p_main, np.float64))
    for p, b in zip(ps, weights):
        lg = lg + b * np.log(np.asarray(p, np.float64))
    w = np.exp(lg - lg.max())
    return w / w.sum()


def filter64(p_main, ps, a, weights, S, tau, top_k, top_p, min_p=0.0, bias=None):
    """logit_processor_ref.filter64 on the mixed distribution: (keep, kept mask, renormalised p'', p before the filter)"""
    return lr.filter64(mix64(p_main, ps, a, weights), S, tau, top_k, top_p, min_p, bias)


# ---- the case of the GPU oracle comparison (tests/test_guided_generate.py) and of its CPU control (tests/test_guided_cpu.py):
# sampling_ref.oracle_case() for the main model, one guide at hidden 32
ORACLE_GUIDE_N, ORACLE_GUIDE_SEED = 32, 43
ORACLE_WEIGHTS = ((1.5, -0.5), (0.5, 0.5), (1.0, 1.0))  # (a, b_1)


def oracle_guide():
    import sampling_ref as sr
    return sr.peaked_params(ORACLE_GUIDE_N, seed=ORACLE_GUIDE_SEED)
