"""Shared helpers for the -m gpu parity tests: build matching oracle / HIP inputs, compare tensors."""
import json
import os

import numpy as np

from oracle_lib import split_params


def random_case(N, S, B, seed, scale=0.08, M=256, empty=()):
    rs = np.random.RandomState(seed)
    n = 4 * N * M + 4 * N * N + 4 * N + M * N + M
    P = (rs.randn(n) * scale).astype(np.float32)
    xi = rs.randint(0, M, size=(S, B)).astype(np.int32)
    ti = rs.randint(0, M, size=(S, B)).astype(np.int32)
    for (t, b) in empty:
        xi[t, b] = -1
        ti[t, b] = -1
    h0 = (rs.randn(B, N) * 0.1).astype(np.float32)
    c0 = (rs.randn(B, N) * 0.1).astype(np.float32)
    return P, xi, ti, h0, c0


def max_rel(a, b):
    """max |a-b| relative to the tensor's own scale (max |b|)."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def grads_report(d_hip, d_ref, N, M=256):
    a, b = split_params(d_hip, N, M), split_params(d_ref, N, M)
    return {k: max_rel(a[k], b[k]) for k in a}


# ---- window bytes with the statistics of real inputs (tests/test_input_statistics*.py) ---------------------------------
# random_case draws every input byte uniformly, so a bucket of the per-byte gradient sums (dW[:, v] = the sum of the dg
# columns whose input byte is v) holds about T/256 columns.  The generators below give the skewed and degenerate buckets of
# real use.  Pure numpy, seeded; each returns xi, ti of shape [S, B] (row 0 unused, as everywhere else); an empty column is
# xi = ti = -1.
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DISTRIBUTIONS = ("uniform", "text", "one_byte", "edges", "empty_head", "all_empty", "group_collide8", "group_collide4",
                 "chunk_edges")
TARGETS = ("uniform", "one_byte", "same")
ONE_BYTE = 101
# chunk_edges: bucket size -> byte.  Size 0 is byte 1 (and every byte not named here); the rest of the window is REST_BYTE.
CHUNK_EDGE_SIZES = {1: 255, 31: 0, 32: 10, 33: 32, 64: 101, 65: 200}
CHUNK_EDGE_ABSENT, CHUNK_EDGE_REST = 1, 116
CHUNK_EDGE_MIN_T = sum(CHUNK_EDGE_SIZES) + 1


def byte_histogram():
    """Counts per byte value of the first 10^6 bytes of enwik8 (bench_data/enwik6_byte_hist.json)."""
    with open(os.path.join(ROOT, "bench_data", "enwik6_byte_hist.json")) as f:
        counts = np.array(json.load(f)["counts"], dtype=np.float64)
    assert counts.size == 256
    return counts


def text_bytes(n, seed):
    """n bytes with the order-0 statistics of real text (195 values in use, the top one 13.4 %)."""
    p = byte_histogram()
    return np.random.RandomState(seed).choice(256, size=n, p=p / p.sum()).astype(np.uint8)


def bucket_sizes(xi):
    """Columns per input byte over rows 1..S-1: [257], entry 256 the empty columns."""
    x = np.asarray(xi)[1:].ravel()
    return np.bincount(np.where(x < 0, 256, x), minlength=257)


def _chunk_edges(S, B):
    """Buckets of exactly 0, 1, 31, 32, 33, 64 and 65 columns (the DW_CHUNK = 32 edges of the sorted sums) and one bucket
    with the rest.  Column c = (t-1)*B + b.  Half of each bucket is a run of neighbouring columns (same step, same column
    group, same aligned quad of columns), the other half is spread over the whole window; the single column is the last."""
    T = (S - 1) * B
    assert T >= CHUNK_EDGE_MIN_T, f"chunk_edges needs at least {CHUNK_EDGE_MIN_T} columns, the window has {T}"
    flat = np.full(T, CHUNK_EDGE_REST, np.int32)
    free = np.ones(T, bool)
    flat[T - 1] = CHUNK_EDGE_SIZES[1]
    free[T - 1] = False
    start = 0
    for n, v in sorted(CHUNK_EDGE_SIZES.items()):
        if n == 1:
            continue
        run = n // 2
        assert free[start:start + run].all()
        flat[start:start + run] = v                 # next to each other
        free[start:start + run] = False
        start += run + 3                            # the runs start at different offsets inside a quad and a group
    for n, v in sorted(CHUNK_EDGE_SIZES.items()):
        if n == 1:
            continue
        spread = n - n // 2
        idx = np.nonzero(free)[0]
        pick = idx[np.linspace(0, idx.size - 1, spread).round().astype(int)]   # far apart, first and last free column included
        assert np.unique(pick).size == spread
        flat[pick] = v
        free[pick] = False
    xi = np.empty((S, B), np.int32)
    xi[1:] = flat.reshape(S - 1, B)
    xi[0] = xi[1]
    sizes = bucket_sizes(xi)
    for n, v in CHUNK_EDGE_SIZES.items():
        assert sizes[v] == n, (v, n, sizes[v])
        where = np.nonzero(flat == v)[0]
        if n > 1:
            assert (np.diff(where) == 1).any() and where[-1] - where[0] >= T // 2, (v, where)
            pairs = where[:-1][np.diff(where) == 1]
            assert (pairs // 4 == (pairs + 1) // 4).any(), v                       # two in one aligned quad of columns
            if B >= 2:                                                             # ... at one step in one column group
                assert ((pairs // B == (pairs + 1) // B) & ((pairs % B) // 8 == ((pairs + 1) % B) // 8)).any(), v
    assert sizes[CHUNK_EDGE_ABSENT] == 0 and sizes[256] == 0
    assert sizes[CHUNK_EDGE_REST] == T - sum(CHUNK_EDGE_SIZES) > 0
    assert np.count_nonzero(sizes) == len(CHUNK_EDGE_SIZES) + 1
    return xi


def window_bytes(kind, S, B, seed, target="uniform"):
    """xi, ti [S, B] int32 for one of DISTRIBUTIONS and one of TARGETS."""
    rs = np.random.RandomState(seed)
    if kind == "uniform":
        xi = rs.randint(0, 256, size=(S, B))
    elif kind == "text":
        xi = text_bytes(S * B, seed).reshape(S, B)
    elif kind == "one_byte":
        xi = np.full((S, B), ONE_BYTE)
    elif kind == "edges":
        xi = np.where(rs.random_sample((S, B)) < 0.001, 255, 0)
        if not (xi[1:] == 255).any():
            xi[1 + rs.randint(S - 1), rs.randint(B)] = 255
    elif kind == "empty_head":
        xi = text_bytes(S * B, seed).reshape(S, B).astype(np.int32)
        xi[:(S + 1) // 2] = -1
    elif kind == "all_empty":
        xi = np.full((S, B), -1)
    elif kind in ("group_collide8", "group_collide4"):
        k = int(kind[len("group_collide"):])
        xi = (rs.randint(0, 256, size=(S, 1)) + 37 * (np.arange(B)[None, :] // k)) % 256
    elif kind == "chunk_edges":
        xi = _chunk_edges(S, B)
    else:
        raise ValueError(kind)
    xi = np.ascontiguousarray(xi, dtype=np.int32)
    if target == "uniform":
        ti = rs.randint(0, 256, size=(S, B))
    elif target == "one_byte":
        ti = np.full((S, B), ONE_BYTE)
    elif target == "same":
        ti = xi.copy()
    else:
        raise ValueError(target)
    ti = np.where(xi < 0, -1, ti).astype(np.int32)
    return xi, ti


def dW_byte_report(d_hip, d_ref, N, xi, M=256):
    """dW column by column.  Returns (worst, byte, size, nonzero_absent): the largest max|dW[:, v] - ref[:, v]| / max|ref[:, v]|
    over the bytes v that occur in rows 1..S-1 of xi, the byte it belongs to and that byte's bucket size; and the bytes that do
    not occur but whose dW column is not bit-exactly 0.  A lost or misplaced column of a small bucket shows here where the
    per-tensor figure of grads_report, scaled by the largest bucket's sum, hides it."""
    a = split_params(np.asarray(d_hip), N, M)["W"].astype(np.float64)
    b = split_params(np.asarray(d_ref), N, M)["W"].astype(np.float64)
    sizes = bucket_sizes(xi)
    worst, at = 0.0, -1
    for v in np.nonzero(sizes[:M])[0]:
        e = float(np.abs(a[:, v] - b[:, v]).max() / max(np.abs(b[:, v]).max(), 1e-30))
        if at < 0 or e > worst:
            worst, at = e, int(v)
    absent = np.nonzero(sizes[:M] == 0)[0]
    nonzero_absent = [int(v) for v in absent if np.any(a[:, v] != 0.0)]
    return worst, at, (int(sizes[at]) if at >= 0 else 0), nonzero_absent


def db_minus_dW(d, N, M=256):
    """db - sum over the input bytes of dW, in float64: the empty columns' share of db (x is one-hot or empty)."""
    p = split_params(np.asarray(d), N, M)
    return p["b"][:, 0].astype(np.float64) - p["W"].astype(np.float64).sum(axis=1)


# ---- parameters and states with the statistics of a trained model (tests/test_param_statistics*.py) ---------------------
# random_case draws every parameter from one Gaussian of scale 0.02-0.08: every gate is about 0.5, tanh is linear and the
# softmax is flat.  The regimes below give saturated gates, cells near +-1 and peaked outputs.  Pure numpy, seeded.
PARAM_REGIMES = ("gauss", "saturated", "mild", "tiled_A", "tiled_B", "unit_scales")
STATE_REGIMES = ("small", "carried")
GOLDEN = os.path.join(ROOT, "tests", "golden")
# (W, U * sqrt(N), b, forget-row offset of b, Why * sqrt(N), by)
_SCALES = dict(saturated=(3.0, 2.0, 2.0, 3.0, 4.0, 3.0), mild=(1.5, 1.0, 1.0, 1.5, 2.0, 1.0))


def fixture(name):
    """tests/golden/fixture_{A,B}.npz: the reference's trained weights (hidden 32 / 16), its held-out text, its logged bits."""
    fx = np.load(os.path.join(GOLDEN, f"fixture_{name}.npz"))
    return dict(N=int(fx["N"]), params=fx["params"].astype(np.float32), text=fx["text"], bits=float(fx["expected_bits"]))


def join_params(W, U, b, Why, by):
    """Flat block from W [M, 4N], U [N, 4N], b [4N], Why [N, M], by [M]: each the C-order bytes of the column-major matrix."""
    return np.concatenate([np.asarray(a, np.float32).ravel() for a in (W, U, b, Why, by)])


def tile_params(P, n, k, M=256):
    """The hidden-n model P block-tiled to hidden k * n: the rows of W and b of each gate repeated k times, each gate block of
    U block-diagonal with k copies, Why repeated k times along its columns and divided by k, by unchanged.  Every block of n
    units then carries the small model's h (from a state tiled the same way) and the logits are the small model's."""
    p = split_params(np.asarray(P, np.float32), n, M)
    N = k * n
    W = np.tile(p["W"].T.reshape(M, 4, 1, n), (1, 1, k, 1)).reshape(M, 4 * N)
    b = np.tile(p["b"][:, 0].reshape(4, 1, n), (1, k, 1)).reshape(4 * N)
    Us = p["U"].T.reshape(n, 4, n)                       # [column, gate, row]
    U = np.zeros((k, n, 4, k, n), np.float32)
    for c in range(k):
        U[c, :, :, c, :] = Us
    Why = np.tile(p["Why"].T, (k, 1)) / np.float32(k)    # [N, M]
    return join_params(W, U.reshape(N, 4 * N), b, Why, p["by"][:, 0])


def regime_params(regime, N, seed, scale=0.08, M=256):
    """The flat parameter block of one of PARAM_REGIMES at hidden N (gate row order [i; o; f; u])."""
    rs = np.random.RandomState(seed)
    if regime == "gauss":
        return random_case(N, 2, 1, seed, scale=scale, M=M)[0]
    if regime in _SCALES:
        w, u, b_, f, why, by_ = _SCALES[regime]
        W = w * rs.randn(M, 4 * N)
        U = u / np.sqrt(N) * rs.randn(N, 4 * N)
        b = b_ * rs.randn(4 * N)
        b[2 * N:3 * N] += f
        return join_params(W, U, b, why / np.sqrt(N) * rs.randn(N, M), by_ * rs.randn(M))
    if regime in ("tiled_A", "tiled_B"):
        fx = fixture(regime[-1])
        assert N % fx["N"] == 0, (regime, N)
        return tile_params(fx["params"], fx["N"], N // fx["N"], M)
    if regime == "unit_scales":
        p = split_params(random_case(N, 2, 1, seed, scale=0.08, M=M)[0].copy(), N, M)      # views of the one block
        f = np.exp(rs.uniform(np.log(0.01), np.log(3.0), N)).astype(np.float32)             # one factor per hidden unit
        rows = np.tile(f, 4)
        W, U, b, Why = (p["W"] * rows[:, None]).T, (p["U"] * rows[:, None]).T, p["b"][:, 0] * rows, (p["Why"] * f[None, :]).T
        return join_params(W, U, b, Why, p["by"][:, 0])
    raise ValueError(regime)


def regime_state(kind, N, B, seed, tile=1):
    """h0, c0 [B, N] float32.  small: 0.1 N(0,1) as random_case; carried: c0 = tanh(2 N(0,1)), h0 = sigmoid(3 N(0,1)) c0, so
    that |c0| reaches 0.999 (cut at 0.9995).  tile = k draws the state of N / k units and repeats it k times (for tile_params' models)."""
    rs = np.random.RandomState(seed + 7919)
    n = N // tile
    if kind == "small":
        h0, c0 = rs.randn(B, n) * 0.1, rs.randn(B, n) * 0.1
    elif kind == "carried":
        c0 = np.clip(np.tanh(2.0 * rs.randn(B, n)), -0.9995, 0.9995)      # (a float32 cell is never 1.0, which tanh(9) rounds to)
        h0 = c0 / (1.0 + np.exp(-3.0 * rs.randn(B, n)))
    else:
        raise ValueError(kind)
    return np.tile(h0, (1, tile)).astype(np.float32), np.tile(c0, (1, tile)).astype(np.float32)


def text_windows(text, S, B):
    """xi, ti [S, B]: B overlapping windows of the text, their starts spread evenly over it, target = the next byte."""
    text = np.asarray(text, np.uint8)
    assert text.size > S
    start = np.linspace(0, text.size - S, B).round().astype(np.int64)
    at = start[None, :] + np.arange(S)[:, None]          # row t reads text[start + t - 1]; row 0 is unused
    xi = text[np.maximum(at - 1, 0)].astype(np.int32)
    ti = text[at].astype(np.int32)
    xi[0], ti[0] = xi[1], ti[1]
    return np.ascontiguousarray(xi), np.ascontiguousarray(ti)
