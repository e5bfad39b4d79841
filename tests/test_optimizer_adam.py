"""-m gpu: Adam / AdamW as the update rule of the fused update launch (lstm_hip_set_optimizer, lstm_hip_get_optimizer_steps,
lstm_hip_set_optimizer_steps in include/lstm_hip.h).

At step t (1-based, per handle), with d' = d * coef when clipping scales the step:
    p <- p * (1 - lr*wd)  (wd > 0);  m <- m + (1 - b1)(d' - m);  v <- b2 v + (1 - b2) d'^2
    p <- p - (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
with the per-step scalars computed in double and narrowed to float.  Checked here: the step is that rule within a few fp32
ulps of its operands on every engine form (fold path included), 20 windows replay torch.optim.AdamW, chunking, resuming
through the public calls, padding, clipping and a 1-rank communicator change no bit, the weight images the launch rewrites
match its parameters, the explicit Adagrad rule is the default one, and the training program saves and resumes Adam."""
import ctypes as C
import math
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import gpu_util as gu
from test_grad_clip import FORMS, _flags, _text, _unpad
from test_pad_hidden import pad_params, same_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSTM = os.path.join(ROOT, "eigen-lstm_amd", "lstm")
B1, B2, EPS = 0.9, 0.999, 1e-8
ULP = 2.0 ** -24
FLOOR = 8 * 2.0 ** -126  # (below the normal range the comparison does not depend on denormal handling)


def _scalars(lr, t, wd, b1=B1, b2=B2, eps=EPS):
    """the step's scalars as the library narrows them (include/lstm_hip.h)"""
    f = np.float32
    return dict(decay=f(1.0 - lr * wd) if wd > 0 else f(1.0), omb1=f(1.0 - b1), b2=f(b2), omb2=f(1.0 - b2),
                step=f(lr / (1.0 - b1 ** t)), bc2s=f(math.sqrt(1.0 - b2 ** t)), eps=f(eps))


def _check_rule(got, P0, d, m0, v0, s, k=8):
    """got = (p, m, v) from the device against the rule restated in float64 from the same fp32 inputs; each within k fp32
    ulps of the magnitudes of its operands"""
    P0, d, m0, v0 = (x.astype(np.float64) for x in (P0, d, m0, v0))
    g = {key: float(val) for key, val in s.items()}
    m = m0 + g["omb1"] * (d - m0)
    v = g["b2"] * v0 + g["omb2"] * d * d
    den = np.sqrt(v) / g["bc2s"] + g["eps"]
    q = g["step"] * m / den
    p = P0 * g["decay"] - q
    tol = {"m": k * ULP * (np.abs(m0) + np.abs(d)) + FLOOR,
           "v": k * ULP * v + FLOOR,
           "p": k * ULP * (np.abs(P0) + np.abs(q) + g["step"] * (np.abs(m0) + np.abs(d)) / den) + FLOOR}
    for name, want, have in (("p", p, got[0]), ("m", m, got[1]), ("v", v, got[2])):
        err = np.abs(have.astype(np.float64) - want)
        assert np.all(err <= tol[name]), (name, float(np.max(err / tol[name])))


def _adam(L, wd=0.0):
    import lstm_hip
    L.set_optimizer(lstm_hip.OPT_ADAM, B1, B2, EPS, wd)


def _state(L):
    import lstm_hip
    return L.get_params(), L.get_grads(), L.get_params(lstm_hip.P_MEM), L.get_params(lstm_hip.P_ADAM_V)


def _loop(N, S, B, flags=0, chunks=(1, 3, 4), lr=2e-3, wd=0.0, P=None, clip=None, comm=False, seed=3, stride=1, text=None):
    """Adam train_windows in the given chunks from init_params; returns (losses, norms or None, P, d, m, v, steps)"""
    import lstm_hip
    text = _text() if text is None else text
    L = lstm_hip.Lstm(N, S, B, flags=flags)
    _adam(L, wd)
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
    out = (np.concatenate(losses), np.concatenate(norms) if norms else None) + _state(L) + (np.array([L.optimizer_steps()]),)
    L.close()
    return out


def _case(N, S, B, flags, seed, t0, wd, loop):
    """an Adam handle with random p, m0, v0 >= 0 and step count t0 that has run one real forward and backward and the update:
    through train_windows(1) (loop: the fused engines' fold path) or forward / backward / adagrad.  Returns (handle, P0, d,
    m0, v0)."""
    import lstm_hip
    P, xi, ti, h0, c0 = gu.random_case(N, S, B, seed=seed)
    rs = np.random.RandomState(seed + 1)
    m0 = (rs.randn(P.size) * 1e-3).astype(np.float32)
    v0 = rs.uniform(0.0, 1e-5, size=P.size).astype(np.float32)
    L = lstm_hip.Lstm(N, S, B, flags=flags)
    _adam(L, wd)
    L.set_params(P)
    L.set_params(m0, lstm_hip.P_MEM)
    L.set_params(v0, lstm_hip.P_ADAM_V)
    L.set_optimizer_steps(t0)
    if loop:
        text = _text(seed=seed)
        L.set_text(text)
        L.set_cursors(lstm_hip.initial_cursors(len(text), S, B))
        L.train_windows(1, 2e-3)
    else:
        L.set_state(0, h0, c0)
        L.set_window(xi, ti)
        L.forward()
        L.backward()
        L.adagrad(2e-3)
    return L, P, L.get_grads(), m0, v0


RULE_SHAPES = [(512, 100, 64, ()), (256, 10, 16, ()), (512, 10, 16, ("BF16_RECURRENCE",)), (64, 6, 4, ("STEP_KERNELS",)),
               (256, 10, 16, ("NO_FUSED_GRADS",)), (128, 25, 1, ()),
               (192, 6, 17, ())]   # a width without a persistent recurrence: the plan's own per-step engine


@pytest.mark.parametrize("loop", [True, False], ids=["train_windows", "adagrad"])
@pytest.mark.parametrize("t0,wd", [(0, 0.0), (1000, 0.0), (0, 0.01), (1000, 0.1)])
@pytest.mark.parametrize("N,S,B,names", RULE_SHAPES)
def test_step_follows_the_rule(N, S, B, names, t0, wd, loop):
    import lstm_hip
    L, P0, d, m0, v0 = _case(N, S, B, _flags(names), N + B + t0, t0, wd, loop)
    assert np.any(d != 0) and np.all(np.isfinite(d))
    p, _, m, v = _state(L)
    _check_rule((p, m, v), P0, d, m0, v0, _scalars(2e-3, t0 + 1, wd))
    assert L.optimizer_steps() == t0 + 1
    assert np.all(v >= 0)
    L.close()


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("N,S,B,names", [(256, 20, 16, ()), (512, 100, 64, ()), (512, 20, 16, ("BF16_RECURRENCE",))])
def test_replay_against_torch_adamw(N, S, B, names, wd):
    """20 windows of train_windows(1); after each one the window's gradient goes through torch.optim.AdamW (single-tensor)
    on an fp32 copy of the start parameters on the CPU"""
    import torch
    import lstm_hip
    lr = 2e-3
    text = _text()
    P0 = lstm_hip.init_params(lstm_hip.MT19937Normal(9), N)
    L = lstm_hip.Lstm(N, S, B, flags=_flags(names))
    _adam(L, wd)
    L.set_params(P0)
    L.set_text(text)
    L.set_cursors(lstm_hip.initial_cursors(len(text), S, B))
    p = torch.nn.Parameter(torch.from_numpy(P0.copy()))
    opt = torch.optim.AdamW([p], lr=lr, betas=(B1, B2), eps=EPS, weight_decay=wd, foreach=False)
    for w in range(20):
        L.train_windows(1, lr)
        p.grad = torch.from_numpy(L.get_grads())
        opt.step()
        got, want = L.get_params(), p.detach().numpy()
        err = float(np.max(np.abs(got.astype(np.float64) - want)))
        assert err <= 1e-6 * max(1.0, float(np.max(np.abs(want)))), (w, err)
    assert L.optimizer_steps() == 20
    L.close()


@pytest.mark.parametrize("N,S,B,names,stride", FORMS)
def test_chunking_is_invisible(N, S, B, names, stride):
    """every engine form: chunks > 1 carry the next window's slide in the Adam launch (short windows); every window has its
    own t"""
    a = _loop(N, S, B, _flags(names), chunks=(1,) * 6, wd=0.01, stride=stride)
    b = _loop(N, S, B, _flags(names), chunks=(6,), wd=0.01, stride=stride)
    assert a[-1][0] == 6
    for x, y, what in zip(a[:1] + a[2:], b[:1] + b[2:], ("losses", "P", "d", "m", "v", "steps")):
        assert same_bytes(x, y), what


@pytest.mark.parametrize("N,S,B,names", [(512, 10, 16, ("BF16_RECURRENCE",)), (1024, 10, 16, ("BF16_RECURRENCE",)),
                                         (512, 100, 64, ()), (512, 20, 128, ())])
def test_images_refreshed_by_the_adam_step_match_its_parameters(N, S, B, names):
    """the Adam launch rewrites the weight images (bf16 U and Why images; the fp32 quad images at the headline shape); a
    second window on them must equal a fresh handle given the same parameters"""
    import lstm_hip
    flags = _flags(names)
    text = _text()
    L = lstm_hip.Lstm(N, S, B, flags=flags)
    _adam(L, 0.01)
    P0 = lstm_hip.init_params(lstm_hip.MT19937Normal(4), N)
    L.set_params(P0)
    L.set_text(text)
    L.set_cursors(lstm_hip.initial_cursors(len(text), S, B))
    L.train_windows(3, 2e-3)
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


def test_padded_handle_matches_an_explicit_wide_one():
    import lstm_hip
    N, Np, S, B = 500, 512, 20, 16
    P = lstm_hip.init_params(lstm_hip.MT19937Normal(7), N)
    a = _loop(N, S, B, lstm_hip.PAD_HIDDEN, chunks=(2, 3), wd=0.01, P=P)
    b = _loop(Np, S, B, 0, chunks=(2, 3), wd=0.01, P=pad_params(P, N, Np))
    assert same_bytes(a[0], b[0]) and same_bytes(a[-1], b[-1])
    for x, y in zip(a[2:6], b[2:6]):  # P, d, m, v
        assert same_bytes(x, _unpad(y, N, Np))
    for y in b[4:6]:  # m and v of the padding rows and columns stay exactly 0
        assert same_bytes(pad_params(_unpad(y, N, Np), N, Np), y)


@pytest.mark.parametrize("N,S,B,names", [(256, 10, 16, ()), (512, 100, 64, ()), (512, 10, 16, ("BF16_RECURRENCE",))])
def test_clipped_adam_step(N, S, B, names):
    import lstm_hip
    flags = _flags(names)
    L, P0, d, m0, v0 = _case(N, S, B, flags, 21, 5, 0.01, loop=False)
    norm = np.sqrt(np.sum(d.astype(np.float64) ** 2))
    # the same step again with clipping at half the norm, from the state the first one started from (d is still in place)
    L.set_params(P0)
    L.set_params(m0, lstm_hip.P_MEM)
    L.set_params(v0, lstm_hip.P_ADAM_V)
    L.set_optimizer_steps(5)
    L.set_grad_clip(norm / 2)
    L.adagrad(2e-3)
    rec = L.grad_norms()[0]
    assert abs(rec - norm) <= 1e-9 * norm, (rec, norm)  # the norm of the unclipped gradient
    coef = np.float32(norm / 2 / (rec + 1e-6))
    assert coef < 1
    p, dg, m, v = _state(L)
    assert same_bytes(dg, d)  # the gradient block keeps the unclipped d
    _check_rule((p, m, v), P0, d * coef, m0, v0, _scalars(2e-3, 6, 0.01))
    L.close()


@pytest.mark.parametrize("N,S,B", [(64, 8, 16), (256, 20, 32)])
def test_single_rank_communicator_gives_the_same_bits(N, S, B):
    """clipped Adam with and without a 1-rank communicator.  In a fresh process: RCCL is loaded on first use and must not
    meet a GPU runtime state that earlier tests of this process left (an in-process torch.cuda initialisation, for one)."""
    code = textwrap.dedent(f"""
        import sys
        sys.path[:0] = [{os.path.dirname(os.path.abspath(__file__))!r}, {os.path.join(ROOT, 'eigen-lstm_amd')!r}]
        import numpy as np
        from test_optimizer_adam import _loop
        from test_pad_hidden import same_bytes
        a = _loop({N}, {S}, {B}, 0, chunks=(3, 3), clip=0.5, wd=0.01)
        b = _loop({N}, {S}, {B}, 0, chunks=(3, 3), clip=0.5, wd=0.01, comm=True)
        assert np.sum(a[1] > 0.5) > 0, a[1]
        for x, y, what in zip(a, b, ("losses", "norms", "P", "d", "m", "v", "steps")):
            assert same_bytes(x, y), what
        print("OK")
    """)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout + out.stderr


def _adagrad_loop(N, S, B, explicit, windows=(2, 3)):
    import lstm_hip
    text = _text()
    L = lstm_hip.Lstm(N, S, B)
    if explicit:
        L.set_optimizer(lstm_hip.OPT_ADAGRAD)
    L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(3), N))
    L.set_text(text)
    L.set_cursors(lstm_hip.initial_cursors(len(text), S, B))
    losses = np.concatenate([L.train_windows(k, 0.1) for k in windows])
    out = (losses, L.get_params(), L.get_grads(), L.get_params(lstm_hip.P_MEM))
    L.close()
    return out


@pytest.mark.parametrize("N,S,B", [(256, 10, 16), (512, 100, 64)])
def test_explicit_adagrad_is_the_default(N, S, B):
    for x, y in zip(_adagrad_loop(N, S, B, False), _adagrad_loop(N, S, B, True)):
        assert same_bytes(x, y)


def test_switching_the_kind_zeroes_the_state():
    import lstm_hip
    N, S, B = 128, 10, 8
    text = _text()
    L = lstm_hip.Lstm(N, S, B)
    L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(3), N))
    L.set_text(text)
    L.set_cursors(lstm_hip.initial_cursors(len(text), S, B))
    _adam(L)
    L.train_windows(4, 2e-3)
    assert L.optimizer_steps() == 4
    m, v = L.get_params(lstm_hip.P_MEM), L.get_params(lstm_hip.P_ADAM_V)
    assert np.any(m != 0) and np.any(v != 0)
    _adam(L, 0.05)  # the same kind again: state and count are kept, the new decay applies from the next step
    assert L.optimizer_steps() == 4 and same_bytes(L.get_params(lstm_hip.P_MEM), m)
    assert same_bytes(L.get_params(lstm_hip.P_ADAM_V), v)
    L.set_optimizer(lstm_hip.OPT_ADAGRAD)
    assert L.optimizer_steps() == 0 and not np.any(L.get_params(lstm_hip.P_MEM))
    with pytest.raises(lstm_hip.LstmHipError):
        L.get_params(lstm_hip.P_ADAM_V)
    L.train_windows(3, 0.1)
    assert L.optimizer_steps() == 3 and np.any(L.get_params(lstm_hip.P_MEM) != 0)
    _adam(L)
    assert L.optimizer_steps() == 0
    assert not np.any(L.get_params(lstm_hip.P_MEM)) and not np.any(L.get_params(lstm_hip.P_ADAM_V))
    L.close()


@pytest.mark.parametrize("N,S,B,names", [(256, 10, 16, ()), (512, 100, 64, ()), (512, 10, 16, ("BF16_RECURRENCE",))])
def test_resume_through_the_public_calls(N, S, B, names):
    import lstm_hip
    flags, lr, wd = _flags(names), 2e-3, 0.01
    text = _text()
    P0 = lstm_hip.init_params(lstm_hip.MT19937Normal(12), N)

    def start(H):
        _adam(H, wd)
        H.set_text(text)

    A = lstm_hip.Lstm(N, S, B, flags=flags)
    start(A)
    A.set_params(P0)
    A.set_cursors(lstm_hip.initial_cursors(len(text), S, B))
    la = np.concatenate([A.train_windows(10, lr), A.train_windows(10, lr)])
    want = (la,) + _state(A) + (np.array([A.optimizer_steps()]),)
    A.close()

    X = lstm_hip.Lstm(N, S, B, flags=flags)
    start(X)
    X.set_params(P0)
    X.set_cursors(lstm_hip.initial_cursors(len(text), S, B))
    l1 = X.train_windows(10, lr)
    R = lstm_hip.Lstm(N, S, B, flags=flags)
    start(R)
    for which in (lstm_hip.P_PARAMS, lstm_hip.P_MEM, lstm_hip.P_ADAM_V):
        R.set_params(X.get_params(which), which)
    R.set_optimizer_steps(X.optimizer_steps())
    R.set_cursors(X.get_cursors())
    R.set_window(*X.get_window())
    R.set_state(1, *X.get_state(1))  # the carry column of the next slide
    X.close()
    l2 = R.train_windows(10, lr)
    got = (np.concatenate([l1, l2]),) + _state(R) + (np.array([R.optimizer_steps()]),)
    R.close()
    for x, y, what in zip(want, got, ("losses", "P", "d", "m", "v", "steps")):
        assert same_bytes(x, y), what


def test_headline_run_is_deterministic_and_trains():
    runs = [_loop(512, 100, 64, 0, chunks=(50,) * 4, wd=0.01, seed=5) for _ in range(2)]
    assert np.all(np.isfinite(runs[0][0])) and runs[0][-1][0] == 200
    for a, b in zip(runs[0], runs[1]):
        assert a is None and b is None or same_bytes(a, b)
    # a learnable text; the first S - 1 windows score fewer steps (the window fills one column per window), so the
    # comparison starts at window S
    text = np.frombuffer(b"the quick brown fox jumps over the lazy dog; " * 400, np.uint8)
    S = 25
    small = _loop(128, S, 8, 0, chunks=(100,) * 3, seed=6, text=text)[0]
    early, late = small[S:S + 50].mean(), small[-50:].mean()
    assert np.all(np.isfinite(small)) and late < 0.9 * early, (early, late)


def test_boundary_codes():
    import lstm_hip
    L = lstm_hip.Lstm(64, 6, 4)
    lib, h = L.lib, L._h
    lib.lstm_hip_set_optimizer.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double]
    lib.lstm_hip_set_optimizer_steps.argtypes = [C.c_void_p, C.c_int64]
    lib.lstm_hip_get_optimizer_steps.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    buf = np.zeros(L.np, np.float32)
    bp = buf.ctypes.data_as(C.POINTER(C.c_float))
    OPT_ADAM, OPT_ADAGRAD, EINVAL, ESTATE = lstm_hip.OPT_ADAM, lstm_hip.OPT_ADAGRAD, lstm_hip.EINVAL, lstm_hip.ESTATE
    assert lib.lstm_hip_get_params(h, 3, bp) == ESTATE  # Adagrad handle: no second moment
    nan, inf = math.nan, math.inf
    for args in [(OPT_ADAGRAD, 0.9, 0, 0, 0), (OPT_ADAGRAD, 0, 0, 1e-8, 0), (OPT_ADAGRAD, 0, 0, 0, 0.01), (OPT_ADAGRAD, 0, 0.9, 0, 0),
                 (OPT_ADAM, 1.0, 0.999, 1e-8, 0), (OPT_ADAM, -0.1, 0.999, 1e-8, 0), (OPT_ADAM, nan, 0.999, 1e-8, 0),
                 (OPT_ADAM, 0.9, 1.0, 1e-8, 0), (OPT_ADAM, 0.9, -1e-3, 1e-8, 0), (OPT_ADAM, 0.9, inf, 1e-8, 0),
                 (OPT_ADAM, 0.9, 0.999, 0.0, 0), (OPT_ADAM, 0.9, 0.999, -1e-8, 0), (OPT_ADAM, 0.9, 0.999, inf, 0),
                 (OPT_ADAM, 0.9, 0.999, 1e-8, -0.01), (OPT_ADAM, 0.9, 0.999, 1e-8, nan), (OPT_ADAM, 0.9, 0.999, 1e-8, inf),
                 (2, 0, 0, 0, 0), (-1, 0, 0, 0, 0)]:
        assert lib.lstm_hip_set_optimizer(h, *args) == EINVAL, args
    assert lib.lstm_hip_get_params(h, 3, bp) == ESTATE  # (nothing was accepted)
    assert lib.lstm_hip_set_optimizer_steps(h, -1) == EINVAL
    assert lib.lstm_hip_get_optimizer_steps(h, None) == EINVAL
    assert lib.lstm_hip_set_optimizer(h, OPT_ADAM, 0.0, 0.0, 1e-8, 0.0) == 0  # the edges of the ranges are accepted
    assert lib.lstm_hip_get_params(h, 3, bp) == 0 and not np.any(buf)
    assert lib.lstm_hip_get_params(h, 4, bp) == EINVAL
    L.close()


def test_profiling_shows_adam_launches_only_with_adam():
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
    assert st["adam"][0] == 0 and st["adagrad"][0] == 3
    _adam(L)
    L.reset_kernel_stats()
    L.train_windows(3, 2e-3)
    st = L.kernel_stats()
    assert st["adam"][0] == 3 and st["adagrad"][0] == 0
    L.close()


def _read(path):
    return np.loadtxt(path, ndmin=2)


def test_program_saves_and_resumes_adam(tmp_path):
    text = np.random.RandomState(11).randint(97, 110, size=3000).astype(np.uint8)
    f = tmp_path / "corpus.txt"
    text.tofile(f)
    base = [LSTM, str(f), "32", "8", "4", "0.002", "--epochs", "1", "--seed", "1", "--sample", "0", "--quiet"]
    adam = ["--optimizer", "adam", "--adam-betas", "0.9,0.99", "--adam-eps", "1e-7", "--weight-decay", "0.01"]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    out = subprocess.run(base + adam + ["--windows", "50", "--save", a], capture_output=True, text=True, errors="replace",
                         timeout=300)
    assert out.returncode == 0, out.stderr
    names = sorted(p.name for p in tmp_path.iterdir() if p.name.startswith("a_"))
    blocks = ("W", "U", "Why", "b", "by")
    want = sorted([f"a_{k}.txt" for k in blocks] + [f"a_adam_{w}_{k}.txt" for w in "mv" for k in blocks] +
                  ["a_adam_steps.txt", "a_cursors.txt"])
    assert names == want, names  # (no _mem_* files)
    assert open(a + "_adam_steps.txt").read().split() == ["50"]
    for k in blocks:
        assert np.all(_read(f"{a}_adam_v_{k}.txt") >= 0)
    assert np.any(_read(a + "_adam_m_U.txt") < 0)  # m is signed: it must never be loaded as Adagrad memory
    out = subprocess.run(base + adam + ["--windows", "10", "--load", a, "--save", b], capture_output=True, text=True,
                         errors="replace", timeout=300)
    assert out.returncode == 0, out.stderr
    assert "Loaded Adam state (t = 50)" in out.stdout, out.stdout
    assert open(b + "_adam_steps.txt").read().split() == ["60"]
    losses = re.findall(r"avg loss = (\S+) bits/char", out.stdout)
    assert len(losses) == 1 and np.isfinite(float(losses[0])), out.stdout
    plain = subprocess.run(base + ["--windows", "10", "--load", a], capture_output=True, text=True, errors="replace", timeout=300)
    assert plain.returncode == 0, plain.stderr
    assert "Loaded parameters" in plain.stdout and "Loaded Adagrad memory" not in plain.stdout and "Adam" not in plain.stdout
