"""The sampling filter of lstm_hip_generate_ex (include/lstm_hip.h, rules 1-6) in numpy, and the case the oracle tests share.

filter64 states the rules in float64 for comparisons against the oracle; draw32 follows the device's arithmetic (float32,
every sum sequential) and also picks the byte.  Both take the stream's ranking key (the logits z, or anything monotone in
them such as the temperature-1 probabilities) and the normalised terms p the CDF walk would use without a filter."""
import numpy as np

import gpu_util as gu

M = 256


def ranks(key):
    """rank_m = #{i : key_i > key_m} + #{i < m : key_i == key_m}: key descending, index ascending"""
    key = np.asarray(key)
    order = np.lexsort((np.arange(key.size), -key.astype(np.float64)))  # last key first: -key, then the index
    r = np.empty(key.size, np.int64)
    r[order] = np.arange(key.size)
    return r


def tempered(p1, tau):
    """the distribution at temperature tau of temperature-1 probabilities p1 (float64)"""
    q = np.asarray(p1, np.float64) ** (1.0 / tau)
    return q / q.sum()


def filter64(key, p, top_k, top_p):
    """Rules 1-5 in float64: returns (keep, kept mask [256], renormalised p'' [256])."""
    p = np.asarray(p, np.float64)
    r = ranks(key)
    keep_k = top_k if 1 <= top_k <= 255 else 256
    keep_p = 256
    if top_p < 1.0:
        cum = np.cumsum(p[np.argsort(r)])
        hit = np.nonzero(cum >= top_p)[0]
        keep_p = int(hit[0]) + 1 if hit.size else 256
    keep = min(keep_k, keep_p)
    mask = r < keep
    q = np.where(mask, p, 0.0)
    return keep, mask, q / q.sum()


def draw32(key, p, top_k, top_p, u):
    """Rules 1-6 as the device computes them: float32, sequential sums.  Returns (byte, keep, p'' [256] float32)."""
    p = np.asarray(p, np.float32)
    r = ranks(key)
    keep_k = top_k if 1 <= top_k <= 255 else 256
    keep_p = 256
    if top_p < 1.0:
        by_rank = p[np.argsort(r)]
        s, edge = np.float32(0.0), np.float32(top_p)
        for i in range(M):
            s = np.float32(s + by_rank[i])
            if s >= edge:
                keep_p = i + 1
                break
    keep = min(keep_k, keep_p)
    mask = r < keep
    q = np.where(mask, p, np.float32(0.0)).astype(np.float32)
    s = np.float32(0.0)
    for m in range(M):
        s = np.float32(s + q[m])
    q = (q / s).astype(np.float32)
    x, cdf, uf = int(np.nonzero(mask)[0].max()), np.float32(0.0), np.float32(u)
    for m in range(M):
        cdf = np.float32(cdf + q[m])
        if uf < cdf:
            x = m
            break
    return x, keep, q


def ambiguous(p, top_k, top_p):
    """True where float32 and float64 may rightly disagree about the kept set: the k-th and (k+1)-th largest probabilities
    differ by less than 1e-6 relative (the argmax margin of test_temperature_and_greedy_against_the_oracle), or some prefix
    sum of the sorted probabilities lies within 1e-5 of top_p (that test's CDF slack)."""
    ps = np.sort(np.asarray(p, np.float64))[::-1]
    if 1 <= top_k <= 255 and ps[top_k - 1] - ps[top_k] < 1e-6 * ps[top_k - 1]:
        return True
    if top_p < 1.0 and np.abs(np.cumsum(ps) - top_p).min() < 1e-5:
        return True
    return False


# ---- the case of the oracle comparison (tests/test_sampling_controls.py) and of its CPU control
# (tests/test_sampling_controls_cpu.py): the tempered test's shape (N = 64, four streams of 150 draws after a one-byte
# prompt, recurrence parameters of scale 0.2) with the output layer (Why, by) scaled up by OUTPUT_GAIN, so that the
# distributions are peaked as a trained model's are and a filter has something to cut.
ORACLE_N, ORACLE_STREAMS, ORACLE_COUNT = 64, 4, 150
OUTPUT_GAIN = 9.0
ORACLE_SETTINGS = (  # (top_k, top_p, temperature)
    (40, 1.0, 1.0),
    (0, 0.9, 1.0),
    (40, 0.9, 0.8),
    (5, 1.0, 1.5),
)


def peaked_params(N, seed, scale=0.2, gain=OUTPUT_GAIN):
    P = gu.random_case(N, 2, 1, seed=seed, scale=scale)[0]
    out = 4 * N * M + 4 * N * N + 4 * N  # Why and by are the last M*N + M values
    P[out:] *= np.float32(gain)
    return P


def oracle_case():
    """(P, prompts, u): parameters, one prompt byte per stream, draws [count, streams]"""
    P = peaked_params(ORACLE_N, seed=41)
    rs = np.random.RandomState(42)
    prompts = [rs.randint(32, 127, size=1).astype(np.uint8) for _ in range(ORACLE_STREAMS)]
    u = np.random.RandomState(43).random_sample((ORACLE_COUNT, ORACLE_STREAMS))
    return P, prompts, u


def replay(orc, N, P, prompt, drawn):
    """temperature-1 probabilities [len(drawn), 256] (float64) each byte of `drawn` was drawn from, the stream having
    started from zero with the one-byte `prompt`: its inputs fed back through the oracle's forward pass"""
    C = len(drawn)
    xi = np.full((C + 1, 1), -1, np.int32)
    xi[1, 0] = prompt[0]
    xi[2:, 0] = drawn[:-1]
    fw = orc.forward(N, M, C + 1, 1, P, xi, np.full((C + 1, 1), -1, np.int32), np.zeros((1, N), np.float32),
                     np.zeros((1, N), np.float32))
    return np.asarray(fw["probs"][1:, 0, :], np.float64)
