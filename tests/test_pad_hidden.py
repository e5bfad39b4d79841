"""-m gpu: LSTM_HIP_PAD_HIDDEN -- any hidden size, run at an internal padded width Np (include/lstm_hip.h).

A padded unit (all-zero rows and columns of W, U, b, Why) keeps c = h = 0 and gets zero gradients, so a handle created as
(N, PAD_HIDDEN) must compute exactly what a handle created as (Np) computes from the zero-padded parameters: bit for bit, in
the losses, in every block it returns and in the evaluator and sampler.  Against the oracle at logical N the usual parity
tolerances of test_hip_parity.py hold."""
import os
import re
import subprocess

import numpy as np
import pytest

import gpu_util as gu
from oracle_lib import split_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 256
ACT_TOL, LOSS_TOL, GRAD_TOL = 2e-5, 2e-5, 2e-4


def padded_width(N, flags):
    """the rule of include/lstm_hip.h"""
    import lstm_hip
    up = lambda n, k: -(-n // k) * k
    if flags & lstm_hip.STEP_KERNELS:
        return up(N, 16)
    if flags & lstm_hip.BF16_RECURRENCE:
        return up(N, 128)
    if N <= 64 or N > 1024:
        return up(N, 16)
    if N % 64 == 0:
        return N
    return next(w for w in (128, 256, 512, 1024) if N <= w)


def pad_params(P, N, Np):
    s = split_params(P, N)
    W = np.zeros((4 * Np, M), np.float32, order="F")
    U = np.zeros((4 * Np, Np), np.float32, order="F")
    b = np.zeros((4 * Np, 1), np.float32, order="F")
    for k in range(4):
        W[k * Np:k * Np + N] = s["W"][k * N:(k + 1) * N]
        U[k * Np:k * Np + N, :N] = s["U"][k * N:(k + 1) * N]
        b[k * Np:k * Np + N] = s["b"][k * N:(k + 1) * N]
    Why = np.zeros((M, Np), np.float32, order="F")
    Why[:, :N] = s["Why"]
    return np.concatenate([a.ravel(order="F") for a in (W, U, b, Why, s["by"])]).astype(np.float32)


def unpad_params(Pp, N, Np):
    s = split_params(Pp, Np)
    gates = lambda a: np.concatenate([a[k * Np:k * Np + N] for k in range(4)])
    parts = (gates(s["W"]), gates(s["U"])[:, :N], gates(s["b"]), s["Why"][:, :N], s["by"])
    return np.concatenate([a.ravel(order="F") for a in parts]).astype(np.float32)


def pad_cols(a, N, Np, blocks=1):
    """[B, blocks*N] (column-major blocks*N x B) -> [B, blocks*Np], zero rows"""
    a = np.asarray(a, np.float32).reshape(a.shape[0], blocks, N)
    out = np.zeros((a.shape[0], blocks, Np), np.float32)
    out[:, :, :N] = a
    return out.reshape(a.shape[0], blocks * Np)


def real_rows(a, N, Np, blocks=1):
    a = np.asarray(a).reshape(a.shape[0], blocks, Np)
    return np.ascontiguousarray(a[:, :, :N]).reshape(a.shape[0], blocks * N), a[:, :, N:]


def same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _text(n, seed=3):
    rs = np.random.RandomState(seed)
    return rs.choice(np.arange(32, 127), size=n).astype(np.uint8)


def _start(L, text, S, B, P, h1, c1):
    import lstm_hip
    L.set_params(P)
    L.set_text(text)
    L.set_cursors(lstm_hip.initial_cursors(len(text), S, B))
    L.reset_window()
    L.set_state(1, h1, c1)


def _twins(N, S, B, flags, windows, lr=0.1, seed=5, full=True):
    """handle A = (N, flags | PAD_HIDDEN), handle B = (Np, flags) from the zero-padded parameters; same text, cursors,
    carry and `windows` windows of train_windows.  Checks everything A returns against the real part of B's."""
    import lstm_hip
    Np = padded_width(N, flags)
    assert Np % 16 == 0 and Np >= N
    g = lstm_hip.MT19937Normal(seed)
    P = lstm_hip.init_params(g, N, forget_bias=1.0)
    h1, c1 = g.randn(N, B, 0.0, 0.1), g.randn(N, B, 0.0, 0.1)
    text = _text(S * 40 + 7, seed=seed)
    A = lstm_hip.Lstm(N, S, B, flags=flags | lstm_hip.PAD_HIDDEN)
    Bh = lstm_hip.Lstm(Np, S, B, flags=flags)
    _start(A, text, S, B, P, h1, c1)
    _start(Bh, text, S, B, pad_params(P, N, Np), pad_cols(h1, N, Np), pad_cols(c1, N, Np))
    la = A.train_windows(windows, lr)
    lb = Bh.train_windows(windows, lr)
    assert np.all(np.isfinite(la)), la
    assert same_bytes(la, lb), (la, lb)
    assert np.array_equal(A.get_cursors(), Bh.get_cursors())
    for which in (lstm_hip.P_PARAMS, lstm_hip.P_GRADS, lstm_hip.P_MEM):
        pa, pb = A.get_params(which), Bh.get_params(which)
        assert pa.size == lstm_hip.param_count(N)
        assert same_bytes(pa, unpad_params(pb, N, Np)), which
        assert np.array_equal(pad_params(unpad_params(pb, N, Np), N, Np), pb), which   # B's padding entries are 0
    if full:
        for t in range(S):
            for a, b in zip(A.get_state(t), Bh.get_state(t)):
                real, pad = real_rows(b, N, Np)
                assert a.shape == (B, N) and same_bytes(a, real) and not pad.any(), t
        for t in range(1, S):
            (ga, pa), (gb, pb) = A.get_activations(t), Bh.get_activations(t)
            real, pad = real_rows(gb, N, Np, blocks=4)
            assert ga.shape == (B, 4 * N) and same_bytes(ga, real) and same_bytes(pa, pb), t
        ev = _text(700, seed=seed + 1)
        ea, eb = A.eval_bits(ev), Bh.eval_bits(ev)
        assert np.isfinite(ea) and same_bytes(np.float64(ea), np.float64(eb)), (ea, eb)
        rs = np.random.RandomState(seed)
        h0, c0 = (rs.randn(N) * 0.1).astype(np.float32), (rs.randn(N) * 0.1).astype(np.float32)
        u = rs.random_sample(40)
        oa, ha, ca = A.sample(h0, c0, u)
        ob, hb, cb = Bh.sample(pad_cols(h0[None], N, Np)[0], pad_cols(c0[None], N, Np)[0], u)
        assert same_bytes(oa, ob)
        for a, b in ((ha, hb), (ca, cb)):
            assert a.shape == (N,) and same_bytes(a, b[:N]) and not b[N:].any()
    A.close()
    Bh.close()
    return la


@pytest.mark.parametrize("N,S,B,flag_names", [
    (500, 7, 64, ()),
    (400, 10, 32, ()),
    (200, 6, 9, ()),
    (50, 5, 3, ()),
    (1000, 4, 16, ()),
    (200, 6, 9, ("FAST_MATH",)),
    (500, 6, 16, ("BF16_RECURRENCE",)),
])
def test_bit_identical_to_an_explicit_padded_model(N, S, B, flag_names):
    import lstm_hip
    flags = 0
    for f in flag_names:
        flags |= getattr(lstm_hip, f)
    _twins(N, S, B, flags, windows=3)


@pytest.mark.parametrize("N,S,B", [(512, 5, 16), (48, 5, 3)])
def test_flag_is_inert_where_no_padding_is_needed(N, S, B):
    """N = 512 / 48 are their own padded widths: the flag changes nothing (handle B is the same shape without it)."""
    _twins(N, S, B, 0, windows=3)


@pytest.mark.parametrize("N,S,B", [(500, 7, 24), (400, 6, 16), (50, 5, 3)])
def test_one_window_matches_oracle_at_logical_N(N, S, B, oracle32):
    import lstm_hip
    P, xi, ti, h0, c0 = gu.random_case(N, S, B, seed=N + S + B)
    fw = oracle32.forward(N, M, S, B, P, xi, ti, h0, c0)
    dref = oracle32.backward(N, M, S, B, P, xi, ti, fw)
    lr = 0.1
    Pref, mref = P.copy(), np.zeros_like(P)
    oracle32.adagrad(Pref, dref, mref, lr)

    L = lstm_hip.Lstm(N, S, B, flags=lstm_hip.PAD_HIDDEN)
    L.set_params(P)
    L.set_state(0, h0, c0)
    L.set_window(xi, ti)
    L.forward()
    loss = L.loss()
    for t in range(1, S):
        h, c = L.get_state(t)
        g, p = L.get_activations(t)
        for name, got in (("h", h), ("c", c), ("g", g), ("probs", p)):
            err = gu.max_rel(got, fw[name][t])
            assert err <= ACT_TOL, (name, t, err)
    assert abs(loss - fw["loss_bits"]) <= LOSS_TOL * (S - 1), (loss, fw["loss_bits"])
    L.backward()
    rep = gu.grads_report(L.get_grads(), dref, N)
    assert max(rep.values()) <= GRAD_TOL, rep
    L.adagrad(lr)
    mask = np.abs(dref) > 1e-3 * np.abs(dref).max()
    assert np.abs(L.get_params()[mask] - Pref[mask]).max() <= 2e-4 * lr + 1e-6
    mem = L.get_params(lstm_hip.P_MEM)
    np.testing.assert_allclose(mem, mref, rtol=1e-3, atol=1e-3 * float(mref.max()))
    L.close()


def test_device_loop_follows_the_oracle_trainer_at_N500(oracle32):
    """train_windows at N = 500 in lock step with the oracle's trainer (re-synchronised before every window, as
    test_hip_parity.py's device-loop test does): loss and carry within tolerance, window and cursors bit-exact."""
    import lstm_hip
    N, S, B, windows, lr = 500, 6, 8, 4, 0.1
    text = _text(S + 24)
    tr = oracle32.trainer(text, N, S, B, lr=lr, seed=1)
    tr.epoch_reset()
    L = lstm_hip.Lstm(N, S, B, flags=lstm_hip.PAD_HIDDEN)
    L.set_text(text)
    L.set_cursors(lstm_hip.initial_cursors(len(text), S, B))
    L.reset_window()
    for w in range(windows):
        L.set_params(tr.params.copy())
        L.set_params(tr.mem.copy(), lstm_hip.P_MEM)
        L.set_state(1, tr.h[1], tr.c[1])
        got = L.train_windows(1, lr)[0]
        want = tr.window()
        assert abs(got - want) <= LOSS_TOL * (S - 1), (w, got, want)
        xi, ti = L.get_window()
        assert np.array_equal(xi, tr.xi) and np.array_equal(ti, tr.ti), w
        h1, c1 = L.get_state(1)
        assert gu.max_rel(h1, tr.h[1]) <= ACT_TOL and gu.max_rel(c1, tr.c[1]) <= ACT_TOL, w
        d = tr.grads
        mask = np.abs(d) > 1e-3 * np.abs(d).max()
        assert np.abs(L.get_params()[mask] - tr.params[mask]).max() <= 2e-4 * lr + 1e-6, w
    want_pos = []
    for p in lstm_hip.initial_cursors(len(text), S, B):
        p = int(p)
        for _ in range(windows):  # pos++, wrapping to S (OV/lstm_eigen_opt/lstm.cc:190-213)
            p = S if p + 1 >= len(text) else p + 1
        want_pos.append(p)
    assert np.array_equal(L.get_cursors().astype(np.int64), want_pos)
    L.close()


def test_reference_best_model_shape():
    """N = 500, S = 7, B = 1024 (the reference's best published model): 20 windows, finite, and equal to the Np = 512 handle."""
    losses = _twins(500, 7, 1024, 0, windows=20, lr=0.01, full=False)
    assert np.all(np.isfinite(losses))


def test_host_program_at_hidden_500(tmp_path, oracle32):
    """The host program takes the reference's any hidden size: checkpoints in logical N, and the evaluator's number from a
    reloaded checkpoint matches the oracle's."""
    N, S, B = 500, 7, 16
    lstm = os.path.join(ROOT, "eigen-lstm_amd", "lstm")
    text = _text(3000, seed=11)
    f = tmp_path / "corpus.txt"
    text.tofile(f)
    # (lr 0.01: at 0.1 this shape overflows the reference's unshifted softmax within ten windows, the oracle's as well)
    out = subprocess.run([lstm, str(f), str(N), str(S), str(B), "0.01", "--epochs", "1", "--windows", "30", "--seed", "1",
                          "--sample", "50", "--save", str(tmp_path / "ck")],
                         capture_output=True, text=True, errors="replace", timeout=300)
    assert out.returncode == 0, out.stderr
    assert re.search(r"avg loss = ([\d.]+) bits/char", out.stdout), out.stdout
    shapes = {k: np.loadtxt(tmp_path / f"ck_{k}.txt", ndmin=2).shape for k in ("W", "U", "b", "Why", "by")}
    assert shapes == {"W": (4 * N, 256), "U": (4 * N, N), "b": (4 * N, 1), "Why": (256, N), "by": (256, 1)}, shapes
    out2 = subprocess.run([lstm, str(f), str(N), str(S), str(B), "0.0", "--epochs", "1", "--windows", "1", "--load",
                           str(tmp_path / "ck"), "--eval-file", str(f), "--sample", "0"],
                          capture_output=True, text=True, errors="replace", timeout=300)
    assert out2.returncode == 0, out2.stderr
    m2 = re.search(r"Test error: ([\d.]+) bits/char", out2.stdout)
    assert m2, out2.stdout
    P = np.concatenate([np.loadtxt(tmp_path / f"ck_{k}.txt", ndmin=2).astype(np.float32).flatten(order="F")
                        for k in ("W", "U", "b", "Why", "by")])
    assert abs(float(m2.group(1)) - oracle32.eval_bits(N, 256, P, text)) <= 1e-3
