"""-m gpu: global-norm gradient clipping before every Adagrad step (lstm_hip_set_grad_clip, lstm_hip_get_grad_norms in
include/lstm_hip.h).

norm = sqrt(sum of d^2 over the flat block [dW|dU|db|dWhy|dby]) in double, in one fixed order; coef = max_norm / (norm + 1e-6)
narrowed to float; where coef < 1 the step uses d * coef.  +inf measures only.  Checked here: measure-only changes nothing on
any engine form, the recorded norm is the float64 norm of the block, the clipped step is the rule restated in numpy, the norm
is the same on every path (fold, summed block, 1-rank communicator, padded width), and the weight images the clipped Adagrad
launch refreshes match its parameters."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import gpu_util as gu
from oracle_lib import split_params
from test_pad_hidden import pad_params, same_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSTM = os.path.join(ROOT, "eigen-lstm_amd", "lstm")
M = 256


def _flags(names):
    import lstm_hip
    f = 0
    for n in names:
        f |= getattr(lstm_hip, n)
    return f


def _text(n=20000, seed=11):
    return np.random.RandomState(seed).randint(32, 127, size=n).astype(np.uint8)


def _loop(N, S, B, flags=0, clip=None, chunks=(1, 3, 4), lr=0.05, stride=1, P=None, comm=False, seed=3):
    """train_windows in the given chunks from init_params; returns (losses, norms or None, P, d, m)"""
    import lstm_hip
    text = _text()
    L = lstm_hip.Lstm(N, S, B, flags=flags)
    L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(seed), N) if P is None else P)
    L.set_text(text)
    L.set_cursors(lstm_hip.initial_cursors(len(text), S, B))
    if stride > 1:
        L.set_stride(stride, S // 2 - 1)
    if comm:
        L.comm_init(lstm_hip.comm_unique_id(), 1, 0)
        L.set_global_batch(B)
    if clip is not None:
        L.set_grad_clip(clip)
    losses, norms = [], []
    for k in chunks:
        losses.append(L.train_windows(k, lr))
        if clip is not None:
            norms.append(L.grad_norms(k))
            assert L.grad_norms().shape == (k,)
    out = (np.concatenate(losses), np.concatenate(norms) if norms else None, L.get_params(), L.get_grads(),
           L.get_params(lstm_hip.P_MEM))
    L.close()
    return out


FORMS = [  # (N, S, B, flags, stride): every engine form the plan picks
    (128, 25, 1, (), 1),                      # small one-stream forms
    (64, 10, 8, ("STEP_KERNELS",), 1),       # per-step engine
    (512, 100, 64, (), 1),                    # headline: two-half forward + scatter backward, fused, quad Adagrad
    (512, 20, 128, (), 1),                    # wide batch: several launches per recurrence
    (512, 20, 16, ("BF16_RECURRENCE",), 1),
    (1024, 20, 16, ("BF16_RECURRENCE",), 1),
    (256, 10, 16, ("NO_FUSED_GRADS",), 1),
    (128, 16, 8, (), 8),                      # segment variant: stride S/2
    (192, 6, 17, (), 1),                      # a width without a persistent recurrence: the plan's own per-step engine
]


@pytest.mark.parametrize("N,S,B,names,stride", FORMS)
def test_measure_only_changes_nothing(N, S, B, names, stride):
    flags = _flags(names)
    ref = _loop(N, S, B, flags, None, stride=stride)
    got = _loop(N, S, B, flags, math.inf, stride=stride)
    for a, b, what in zip(ref[:1] + ref[2:], got[:1] + got[2:], ("losses", "P", "d", "m")):
        assert same_bytes(a, b), what
    norms = got[1]
    assert norms.shape == (8,) and np.all(np.isfinite(norms)) and np.all(norms > 0), norms


@pytest.mark.parametrize("N,S,B,names", [
    (512, 100, 64, ()), (128, 25, 1, ()), (64, 10, 8, ("STEP_KERNELS",)), (512, 20, 16, ("BF16_RECURRENCE",)),
    (256, 10, 16, ("NO_FUSED_GRADS",)),
])
def test_recorded_norm_is_the_norm_of_the_gradient_block(N, S, B, names):
    import lstm_hip
    flags = _flags(names)
    text = _text()
    L = lstm_hip.Lstm(N, S, B, flags=flags)
    L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(5), N))
    L.set_text(text)
    L.set_cursors(lstm_hip.initial_cursors(len(text), S, B))
    L.set_grad_clip(0.5)  # active: later windows see clipped steps
    one = []
    for _ in range(6):
        L.train_windows(1, 0.1)
        rec = L.grad_norms(1)[0]
        want = np.sqrt(np.sum(L.get_grads().astype(np.float64) ** 2))
        assert abs(rec - want) <= 1e-9 * want, (rec, want)
        one.append(rec)
    L.close()
    chunked = _loop(N, S, B, flags, 0.5, chunks=(2, 4), lr=0.1, seed=5)[1]
    assert same_bytes(np.array(one), chunked)


def _step_case(N, S, B, flags, seed):
    """forward + backward of one random window; returns (handle, P, d, m)"""
    import lstm_hip
    P, xi, ti, h0, c0 = gu.random_case(N, S, B, seed=seed)
    m0 = np.random.RandomState(seed).uniform(0.01, 0.1, size=P.size).astype(np.float32)
    L = lstm_hip.Lstm(N, S, B, flags=flags)
    L.set_params(P)
    L.set_params(m0, lstm_hip.P_MEM)
    L.set_state(0, h0, c0)
    L.set_window(xi, ti)
    L.forward()
    L.backward()
    return L, L.get_params(), L.get_grads(), L.get_params(lstm_hip.P_MEM)


def _within_ulps(a, b, k, *operands):
    """|a - b| <= k ulp of the largest magnitude among a, b and the operands of the last operation"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    big = np.maximum(np.abs(a), np.abs(b))
    for o in operands:
        big = np.maximum(big, np.abs(o.astype(np.float64)))
    tol = k * np.spacing(big.astype(np.float32)).astype(np.float64)
    return np.all(np.abs(a - b) <= tol), np.max(np.abs(a - b) / np.maximum(tol, 1e-45))


@pytest.mark.parametrize("N,S,B,names", [(256, 10, 16, ()), (512, 100, 64, ()), (512, 10, 16, ("BF16_RECURRENCE",)),
                                         (64, 6, 4, ("STEP_KERNELS",))])
def test_clipped_step_follows_the_rule(N, S, B, names):
    import lstm_hip
    flags, lr = _flags(names), 0.1
    L, P0, d, m0 = _step_case(N, S, B, flags, seed=N + B)
    norm = np.sqrt(np.sum(d.astype(np.float64) ** 2))
    max_norm = norm / 2
    L.set_grad_clip(max_norm)
    L.adagrad(lr)
    rec = L.grad_norms()[0]
    assert abs(rec - norm) <= 1e-9 * norm, (rec, norm)
    coef = np.float32(max_norm / (rec + 1e-6))
    assert coef < 1
    dc = d * coef
    m1 = m0 + dc * dc
    den = np.sqrt((m1.astype(np.float64) + 1e-10).astype(np.float32))
    step = np.float32(lr) * (dc / den)
    p1 = P0 - step
    ok, worst = _within_ulps(L.get_params(lstm_hip.P_MEM), m1, 2)
    assert ok, ("m", worst)
    ok, worst = _within_ulps(L.get_params(), p1, 2, P0, step)
    assert ok, ("P", worst)
    assert same_bytes(L.get_grads(), d)  # the gradient block keeps the unclipped d
    L.close()
    # above the norm: the step is the unclipped one, bit for bit
    A, _, _, _ = _step_case(N, S, B, flags, seed=N + B)
    Z, _, _, _ = _step_case(N, S, B, flags, seed=N + B)
    A.set_grad_clip(2 * norm)
    A.adagrad(lr)
    Z.adagrad(lr)
    for which in (lstm_hip.P_PARAMS, lstm_hip.P_GRADS, lstm_hip.P_MEM):
        assert same_bytes(A.get_params(which), Z.get_params(which)), which
    A.close()
    Z.close()


@pytest.mark.parametrize("bad", [math.inf, math.nan])
@pytest.mark.parametrize("N,S,B,names", [(256, 10, 16, ()), (512, 100, 64, ()), (512, 10, 16, ("BF16_RECURRENCE",))])
def test_non_finite_norm_is_recorded_and_the_step_is_unscaled(N, S, B, names, bad):
    """an inf (or NaN) entry in the block makes the norm inf (NaN): it is recorded as is and the step is the unclipped one,
    byte for byte (inf and NaN bytes included) -- not a step scaled by max_norm / (inf + 1e-6) = 0"""
    import lstm_hip
    flags = _flags(names)
    A, _, d, _ = _step_case(N, S, B, flags, seed=N + B)
    Z, _, _, _ = _step_case(N, S, B, flags, seed=N + B)
    d = d.copy()
    d[d.size // 3] = bad
    for H in (A, Z):
        H.set_params(d, lstm_hip.P_GRADS)
    A.set_grad_clip(1.0)
    A.adagrad(0.1)
    Z.adagrad(0.1)
    rec = A.grad_norms()[0]
    assert (math.isinf(rec) and rec > 0) if math.isinf(bad) else math.isnan(rec), rec
    for which in (lstm_hip.P_PARAMS, lstm_hip.P_GRADS, lstm_hip.P_MEM):
        assert same_bytes(A.get_params(which), Z.get_params(which)), which
    assert np.sum(np.isfinite(A.get_params())) == d.size - 1  # only the bad entry left the finite range
    A.close()
    Z.close()


def test_clipped_headline_run_is_deterministic():
    runs = [_loop(512, 100, 64, 0, 0.5, chunks=(20, 30), lr=0.1) for _ in range(2)]
    assert np.sum(runs[0][1] > 0.5) > 0, runs[0][1]  # the clip is active
    for a, b in zip(runs[0], runs[1]):
        assert same_bytes(a, b)


@pytest.mark.parametrize("N,S,B", [(64, 8, 16), (256, 20, 32)])
def test_single_rank_communicator_gives_the_same_norms_and_trajectory(N, S, B):
    a = _loop(N, S, B, 0, 0.5, chunks=(3, 3), lr=0.1)
    b = _loop(N, S, B, 0, 0.5, chunks=(3, 3), lr=0.1, comm=True)
    assert np.sum(a[1] > 0.5) > 0, a[1]
    for x, y, what in zip(a, b, ("losses", "norms", "P", "d", "m")):
        assert same_bytes(x, y), what


@pytest.mark.parametrize("N,S,B", [(128, 25, 1), (256, 8, 8)])
def test_clipped_loop_is_the_same_in_any_chunking(N, S, B):
    """chunks > 1 carry the next window's slide in the clipped Adagrad launch (SLIDE with CLIP)"""
    a = _loop(N, S, B, 0, 0.5, chunks=(1,) * 6, lr=0.1)
    b = _loop(N, S, B, 0, 0.5, chunks=(6,), lr=0.1)
    assert np.sum(a[1] > 0.5) > 0, a[1]
    for x, y in zip(a, b):
        assert same_bytes(x, y)


def _unpad(Pp, N, Np):
    s = split_params(Pp, Np)
    W = np.concatenate([s["W"][k * Np:k * Np + N] for k in range(4)])
    U = np.concatenate([s["U"][k * Np:k * Np + N, :N] for k in range(4)])
    b = np.concatenate([s["b"][k * Np:k * Np + N] for k in range(4)])
    return np.concatenate([a.ravel(order="F") for a in (W, U, b, s["Why"][:, :N], s["by"])]).astype(np.float32)


def test_padded_handle_matches_an_explicit_wide_one():
    import lstm_hip
    N, Np, S, B = 500, 512, 20, 16
    P = lstm_hip.init_params(lstm_hip.MT19937Normal(7), N)
    a = _loop(N, S, B, lstm_hip.PAD_HIDDEN, 0.5, chunks=(2, 3), lr=0.1, P=P)
    b = _loop(Np, S, B, 0, 0.5, chunks=(2, 3), lr=0.1, P=pad_params(P, N, Np))
    assert np.sum(a[1] > 0.5) > 0, a[1]
    assert same_bytes(a[0], b[0]) and same_bytes(a[1], b[1])
    for x, y in zip(a[2:], b[2:]):
        assert same_bytes(x, _unpad(y, N, Np))


@pytest.mark.parametrize("N,S,B,names", [(512, 10, 16, ("BF16_RECURRENCE",)), (1024, 10, 16, ("BF16_RECURRENCE",)),
                                         (512, 100, 64, ())])
def test_images_refreshed_by_the_clipped_step_match_its_parameters(N, S, B, names):
    """the clipped Adagrad launch rewrites the weight images (bf16 U and Why images; the fp32 quad images at the headline
    shape); a second window on them must equal a fresh handle given the same parameters"""
    import lstm_hip
    flags = _flags(names)
    L, P0, d, m0 = _step_case(N, S, B, flags, seed=17)
    L.set_grad_clip(0.25 * np.sqrt(np.sum(d.astype(np.float64) ** 2)))
    L.adagrad(0.1)
    P1 = L.get_params()
    assert not same_bytes(P1, P0)
    _, xi, ti, h0, c0 = gu.random_case(N, S, B, seed=18)
    F = lstm_hip.Lstm(N, S, B, flags=flags)
    F.set_params(P1)
    out = []
    for H in (L, F):
        H.set_state(0, h0, c0)
        H.set_window(xi, ti)
        H.forward()
        loss = H.loss()
        H.backward()
        out.append((np.array([loss]), H.get_state(S - 1)[0], H.get_activations(S - 1)[1], H.get_grads()))
    for x, y in zip(*out):
        assert same_bytes(x, y)
    L.close()
    F.close()


def test_boundary_codes():
    import lstm_hip
    L = lstm_hip.Lstm(64, 6, 4)
    lib, h = L.lib, L._h
    lib.lstm_hip_set_grad_clip.argtypes = [C.c_void_p, C.c_double]
    lib.lstm_hip_get_grad_norms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int64]
    out = (C.c_double * 8)()
    assert lib.lstm_hip_set_grad_clip(h, -1.0) == lstm_hip.EINVAL
    assert lib.lstm_hip_set_grad_clip(h, float("nan")) == lstm_hip.EINVAL
    assert lib.lstm_hip_set_grad_clip(h, -math.inf) == lstm_hip.EINVAL
    assert lib.lstm_hip_get_grad_norms(h, out, 1) == lstm_hip.ESTATE  # no call yet
    text = _text(2000)
    L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(1), 64))
    L.set_text(text)
    L.set_cursors(lstm_hip.initial_cursors(len(text), 6, 4))
    L.train_windows(2, 0.1)
    assert lib.lstm_hip_get_grad_norms(h, out, 1) == lstm_hip.ESTATE  # clipping off for that call
    L.set_grad_clip(1.0)
    L.train_windows(3, 0.1)
    assert lib.lstm_hip_get_grad_norms(h, out, 3) == 0 and all(np.isfinite(out[:3]))
    assert lib.lstm_hip_get_grad_norms(h, out, 4) == lstm_hip.EINVAL
    assert lib.lstm_hip_get_grad_norms(h, out, -1) == lstm_hip.EINVAL
    L.set_grad_clip(0.0)
    L.train_windows(1, 0.1)
    assert lib.lstm_hip_get_grad_norms(h, out, 1) == lstm_hip.ESTATE
    L.close()


def test_profiling_shows_the_norm_launches_only_with_clipping():
    import lstm_hip
    text = _text()
    L = lstm_hip.Lstm(256, 10, 16)
    L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(1), 256))
    L.set_text(text)
    L.set_cursors(lstm_hip.initial_cursors(len(text), 10, 16))
    L.set_profiling(True)
    L.reset_kernel_stats()
    L.train_windows(3, 0.1)
    st = L.kernel_stats()
    assert st["grad_sumsq"][0] == 0 and st["grad_norm"][0] == 0 and st["adagrad"][0] == 3
    L.set_grad_clip(1.0)
    L.reset_kernel_stats()
    L.train_windows(3, 0.1)
    st = L.kernel_stats()
    assert st["grad_sumsq"][0] == 3 and st["grad_norm"][0] == 3 and st["adagrad"][0] == 3
    L.close()


def test_program_prints_the_norm_line(tmp_path):
    text = np.random.RandomState(11).randint(97, 110, size=3000).astype(np.uint8)
    f = tmp_path / "corpus.txt"
    text.tofile(f)
    base = [LSTM, str(f), "32", "8", "4", "0.1", "--epochs", "2", "--windows", "150", "--seed", "1", "--sample", "0"]
    out = subprocess.run(base + ["--clip-norm", "5"], capture_output=True, text=True, errors="replace", timeout=300)
    assert out.returncode == 0, out.stderr
    lines = re.findall(r"grad norm: mean (\S+), max (\S+), clipped (\d+) of (\d+) windows", out.stdout)
    assert len(lines) == 2, out.stdout
    for mean, mx, clipped, n in lines:
        assert np.isfinite(float(mean)) and float(mx) >= float(mean) > 0 and int(n) == 150 and int(clipped) <= 150
    losses = re.findall(r"avg loss = (\S+) bits/char", out.stdout)
    assert len(losses) == 2 and all(np.isfinite(float(v)) for v in losses), out.stdout
    plain = subprocess.run(base, capture_output=True, text=True, errors="replace", timeout=300)
    assert plain.returncode == 0 and "grad norm" not in plain.stdout, plain.stdout
