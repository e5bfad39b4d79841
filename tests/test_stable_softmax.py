"""-m gpu: LSTM_HIP_STABLE_SOFTMAX -- the max-shifted output layer (include/lstm_hip.h).

Per column (one stream at one step), with z = Why*h + by and zmax = max_m z_m: p = expf(z - zmax) / sum, and the surprisal
log2(sum) + (zmax - z_target) log2(e).  At ordinary logits a stable handle computes what a default one does (the recurrence
bit for bit, the output layer within rounding); where the logits leave expf's range it stays finite and right, checked
against float64 restatements made here (the oracle stays the reference's unshifted softmax)."""
import os
import re
import subprocess

import numpy as np
import pytest

import gpu_util as gu
from oracle_lib import split_params
from test_pad_hidden import pad_cols, pad_params, same_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 256
LOG2E = 1.0 / np.log(2.0)


def _flags(names):
    import lstm_hip
    f = 0
    for n in names:
        f |= getattr(lstm_hip, n)
    return f


def _window(N, S, B, flags, P, xi, ti, h0, c0):
    """one forward, loss and backward; returns (handle, loss)"""
    import lstm_hip
    L = lstm_hip.Lstm(N, S, B, flags=flags)
    L.set_params(P)
    L.set_state(0, h0, c0)
    L.set_window(xi, ti)
    L.forward()
    loss = L.loss()
    L.backward()
    return L, loss


@pytest.mark.parametrize("N,S,B,names", [
    (512, 100, 64, ()),
    (128, 25, 1, ()),
    (256, 20, 32, ()),
    (128, 10, 8, ("STEP_KERNELS",)),
    (256, 10, 16, ("NO_FUSED_GRADS",)),
    (256, 10, 16, ("BF16_RECURRENCE",)),
    (500, 7, 16, ("PAD_HIDDEN",)),
])
def test_only_the_softmax_changes_at_ordinary_logits(N, S, B, names):
    import lstm_hip
    flags = _flags(names)
    P, xi, ti, h0, c0 = gu.random_case(N, S, B, seed=N + S + B, empty=((2, 0),))
    A, la = _window(N, S, B, flags, P, xi, ti, h0, c0)
    Z, lz = _window(N, S, B, flags | lstm_hip.STABLE_SOFTMAX, P, xi, ti, h0, c0)
    assert np.isfinite(la) and abs(lz - la) <= 2e-6 * abs(la), (lz, la)
    for t in range(S):
        for a, z in zip(A.get_state(t), Z.get_state(t)):
            assert same_bytes(a, z), t
    for t in range(1, S):
        (ga, pa), (gz, pz) = A.get_activations(t), Z.get_activations(t)
        assert same_bytes(ga, gz), t
        assert gu.max_rel(pz, pa) <= 2e-6, t
    rep = gu.grads_report(Z.get_grads(), A.get_grads(), N)
    assert max(rep.values()) <= 2e-5, rep
    A.close()
    Z.close()


# ---- large logits ---------------------------------------------------------------------------------------------------

def _large_params(N, seed, close_top=False):
    """random parameters whose logits reach |z| ~ 1e3 .. 1e4: by = 1000 - 37 * (a permutation of 0..255), Why * h of a few
    units.  Every column then has one logit ahead of the rest by > 20, so float32 rounding of z (ulp 1e-3 at 1e4) moves p by
    far less than 1e-6.  close_top: the three largest by within 1.5 of each other (CDF edges away from 0 and 1)."""
    P = gu.random_case(N, 2, 1, seed=seed)[0]
    s = split_params(P, N)
    rs = np.random.RandomState(seed + 1)
    s["Why"][:] = (rs.randn(M, N) * (1.5 / np.sqrt(N))).astype(np.float32)
    by = 1000.0 - 37.0 * rs.permutation(M)
    if close_top:
        top = np.argsort(-by)[:3]
        by[top] = [1000.0, 999.2, 998.5]
    s["by"][:, 0] = by.astype(np.float32)
    return P, int(np.argmax(by))


def _z64(P, N, h):
    s = split_params(P, N)
    return h.astype(np.float64) @ s["Why"].astype(np.float64).T + s["by"][:, 0].astype(np.float64)  # [B, M]


def _logsoftmax64(z):
    zm = z.max(axis=-1, keepdims=True)
    return z - zm - np.log(np.exp(z - zm).sum(axis=-1, keepdims=True))


def _large_case(N, S, B, seed, empty=((3, 1),)):
    P, top = _large_params(N, seed)
    _, xi, ti, h0, c0 = gu.random_case(N, S, B, seed=seed + 2, empty=empty)
    ti[1::2, 0] = top          # some targets are the column's likely byte, most underflow in fp32
    return P, xi, ti, h0, c0


def test_large_logits_stable_handle_matches_float64_default_does_not():
    import lstm_hip
    N, S, B = 64, 9, 8
    P, xi, ti, h0, c0 = _large_case(N, S, B, seed=7)
    A, la = _window(N, S, B, 0, P, xi, ti, h0, c0)
    assert not np.isfinite(la), la                                   # the unshifted softmax overflows
    A.close()
    Z, lz = _window(N, S, B, lstm_hip.STABLE_SOFTMAX, P, xi, ti, h0, c0)
    sd = split_params(Z.get_grads(), N)
    dby = np.zeros(M)
    dWhy = np.zeros((M, N))
    surpr = np.zeros((S, B))
    zmax_seen = 0.0
    for t in range(1, S):
        h, _ = Z.get_state(t)
        z = _z64(P, N, h)
        zmax_seen = max(zmax_seen, np.abs(z).max())
        lp = _logsoftmax64(z)
        p = np.exp(lp)
        _, pz = Z.get_activations(t)
        assert np.abs(pz - p).max() <= 1e-6, t
        dy = p.copy()
        for b in range(B):
            if ti[t, b] >= 0:
                surpr[t, b] = -lp[b, ti[t, b]] * LOG2E
                dy[b, ti[t, b]] -= 1.0
        dby += dy.sum(axis=0)
        dWhy += dy.T @ h.astype(np.float64)
    assert zmax_seen > 1e3, zmax_seen
    assert np.isfinite(surpr).all() and surpr.max() > 1e3
    want = {lstm_hip.LOSS_ALL_STEPS_BITS: surpr[1:].sum() / B,
            lstm_hip.LOSS_LAST_STEP_BITS: surpr[S - 1].sum() / B,
            lstm_hip.LOSS_LAST_STEP_NATS: surpr[S - 1].sum() / B * np.log(2.0)}
    assert abs(lz - want[0]) <= 1e-5 * abs(want[0]), (lz, want[0])
    for mode, w in want.items():
        Z.set_loss_mode(mode)
        got = Z.loss()
        assert np.isfinite(got) and abs(got - w) <= 1e-5 * abs(w), (mode, got, w)
    assert gu.max_rel(sd["by"][:, 0], dby) <= 1e-5
    assert gu.max_rel(sd["Why"], dWhy) <= 1e-5
    assert all(np.isfinite(v).all() for v in sd.values())
    Z.close()


def test_whole_window_gradients_against_float64_autograd():
    import torch
    import lstm_hip
    N, S, B = 32, 6, 3
    P, xi, ti, h0, c0 = _large_case(N, S, B, seed=21, empty=())      # (no empty column: the loss below is a sum of CE)
    Z, _ = _window(N, S, B, lstm_hip.STABLE_SOFTMAX, P, xi, ti, h0, c0)
    got = Z.get_grads()
    Z.close()
    s = split_params(P, N)
    T = {k: torch.tensor(np.ascontiguousarray(v), dtype=torch.float64, requires_grad=True) for k, v in s.items()}
    h = torch.tensor(h0, dtype=torch.float64)
    c = torch.tensor(c0, dtype=torch.float64)
    loss = torch.zeros((), dtype=torch.float64)
    for t in range(1, S):
        x = torch.tensor(xi[t], dtype=torch.long)
        g = T["W"][:, x].T + h @ T["U"].T + T["b"][:, 0]              # [B, 4N], gate rows [i; o; f; u]
        i, o, f = (torch.sigmoid(g[:, k * N:(k + 1) * N]) for k in range(3))
        u = torch.tanh(g[:, 3 * N:])
        c = torch.tanh(i * u + f * c)                                 # the stored cell is already squashed
        h = o * c
        z = h @ T["Why"].T + T["by"][:, 0]
        lp = torch.log_softmax(z, dim=1)
        loss = loss - lp[torch.arange(B), torch.tensor(ti[t], dtype=torch.long)].sum()
    loss.backward()
    want = np.concatenate([T[k].grad.numpy().ravel(order="F") for k in ("W", "U", "b", "Why", "by")])
    rep = gu.grads_report(got, want, N)
    assert max(rep.values()) <= 1e-4, rep


def test_reference_learning_rate_trains_finite():
    """lr = 0.1 (R/lstm.cc:59) at the headline shape from the start of
    test_hip_parity.py::test_reference_learning_rate_overflows_the_unshifted_softmax_on_both_sides."""
    import lstm_hip
    from oracle_lib import Oracle
    from bench import synthetic_text
    N, S, B, lr, windows = 512, 100, 64, 0.1, 300
    text = synthetic_text(1_000_000, seed=0)
    tr = Oracle("f32_omp").trainer(text, N, S, B, lr=lr, seed=1)
    tr.epoch_reset()

    def run(flags):
        L = lstm_hip.Lstm(N, S, B, flags=flags)
        L.set_params(tr.params.copy())
        L.set_state(1, tr.h[1], tr.c[1])
        L.set_text(text)
        L.set_cursors(lstm_hip.initial_cursors(len(text), S, B))
        L.reset_window()
        losses = L.train_windows(windows, lr)
        P, mem = L.get_params(), L.get_params(lstm_hip.P_MEM)
        L.close()
        return losses, P, mem

    ls, P, mem = run(lstm_hip.STABLE_SOFTMAX)
    assert np.isfinite(ls).all(), np.nonzero(~np.isfinite(ls))[0][:5]
    assert np.isfinite(P).all() and np.isfinite(mem).all()
    ld, _, _ = run(0)
    bad = np.nonzero(~np.isfinite(ld))[0]
    assert bad.size > 0, "the default handle stayed finite at lr = 0.1"
    first = int(bad[0])
    assert first > 5
    # bits/char per window.  The shift changes only the rounding of p, but at lr = 0.1 such differences grow from window
    # to window (trajectories decorrelate), so the windows are held tightly only at the start.
    diff = np.abs(ls[:first] - ld[:first]) / (S - 1)
    print(f"stable lr=0.1: window 100 loss {ls[99]:.4f}, window 300 loss {ls[299]:.4f} (bits/char {ls[99] / (S - 1):.4f}, "
          f"{ls[299] / (S - 1):.4f}); default non-finite from window {first}; |dloss|/(S-1) per window: "
          + " ".join(f"{d:.2g}" for d in diff))
    assert diff[:5].max() <= 1e-3, diff[:5]


def _eval64(P, N, text):
    """float64 restatement of the evaluator (h = c = 0, bits of text[1:]) in log-softmax form"""
    s = {k: v.astype(np.float64) for k, v in split_params(P, N).items()}
    h, c = np.zeros(N), np.zeros(N)
    bits = 0.0
    for j in range(len(text) - 1):
        g = s["W"][:, text[j]] + s["U"] @ h + s["b"][:, 0]
        sg = 1.0 / (1.0 + np.exp(-g[:3 * N]))
        c = np.tanh(sg[:N] * np.tanh(g[3 * N:]) + sg[2 * N:3 * N] * c)
        h = sg[N:2 * N] * c
        z = s["Why"] @ h + s["by"][:, 0]
        bits += -_logsoftmax64(z)[text[j + 1]] * LOG2E
    return bits / (len(text) - 1)


@pytest.mark.parametrize("names", [(), ("STEP_KERNELS",)])
def test_evaluator_at_large_logits(names):
    """the persistent handle's evaluator runs through its internal B = 1 handle, a STEP_KERNELS handle through k_eval_bits"""
    import lstm_hip
    N = 64
    P, _ = _large_params(N, seed=31)
    text = np.random.RandomState(5).randint(32, 127, size=300).astype(np.uint8)
    want = _eval64(P, N, text)
    for flags, finite in ((_flags(names) | lstm_hip.STABLE_SOFTMAX, True), (_flags(names), False)):
        L = lstm_hip.Lstm(N, 8, 4, flags=flags)
        L.set_params(P)
        got = L.eval_bits(text)
        L.close()
        if finite:
            assert np.isfinite(got) and abs(got - want) <= 1e-5 * abs(want), (names, got, want)
        else:
            assert not np.isfinite(got), (names, got)


def _step64(s, N, h, c, x):
    g = s["W"][:, x] + s["U"] @ h + s["b"][:, 0]
    sg = 1.0 / (1.0 + np.exp(-g[:3 * N]))
    c = np.tanh(sg[:N] * np.tanh(g[3 * N:]) + sg[2 * N:3 * N] * c)
    return sg[N:2 * N] * c, c


def _cdf_walk(s, N, prompt, u, out):
    """float64 CDF walk (first m with u < cdf[m]) along the device's own path from h = c = 0 after `prompt`, for the draws
    at least 1e-4 away from every CDF edge; returns how many were checked"""
    h, c = np.zeros(N), np.zeros(N)
    for x in prompt:
        h, c = _step64(s, N, h, c, x)
    checked = 0
    for i in range(len(u)):
        cdf = np.cumsum(np.exp(_logsoftmax64(s["Why"] @ h + s["by"][:, 0])))
        if np.abs(cdf - u[i]).min() >= 1e-4:
            want = int(np.searchsorted(cdf, u[i], side="right"))
            assert out[i] == want, (i, out[i], want)
            checked += 1
        h, c = _step64(s, N, h, c, out[i])
    return checked


def test_generator_and_sampler_at_large_logits():
    import lstm_hip
    N, C, K = 64, 40, 6
    P, _ = _large_params(N, seed=41, close_top=True)
    s = {k: v.astype(np.float64) for k, v in split_params(P, N).items()}
    rs = np.random.RandomState(3)
    prompts = [rs.randint(32, 127, size=n).astype(np.uint8) for n in (30, 2, 17, 0, 45, 9)]
    u = rs.random_sample((C, K))
    L = lstm_hip.Lstm(N, 8, 4, flags=lstm_hip.STABLE_SOFTMAX)
    L.set_params(P)
    out, bits, _, _ = L.generate(prompts, count=C, u=u, temperature=1.0, score=True)
    assert np.isfinite(bits).all()
    for k, p in enumerate(prompts):
        if len(p) >= 2:
            ev = L.eval_bits(p)
            assert abs(bits[k] / (len(p) - 1) - ev) <= 1e-5 * ev, (k, bits[k] / (len(p) - 1), ev)
            assert abs(bits[k] / (len(p) - 1) - _eval64(P, N, p)) <= 1e-5 * ev
    # temperature 1: the float64 CDF walk along the device's own path, for draws >= 1e-4 away from every edge
    checked = sum(_cdf_walk(s, N, p, u[:, k], out[:, k]) for k, p in enumerate(prompts))
    assert checked >= 0.9 * C * K, checked
    assert len(set(out.ravel().tolist())) >= 2                         # the close top logits are all drawn
    # the single-stream sampler (lstm_hip_sample) is the generator's one-stream case
    so, _, _ = L.sample(np.zeros(N, np.float32), np.zeros(N, np.float32), u[:, 3])
    assert np.array_equal(so, out[:, 3])
    # greedy is unchanged by the flag
    D = lstm_hip.Lstm(N, 8, 4)
    D.set_params(P)
    gz = L.generate(prompts, count=C, temperature=0.0)[0]
    gd = D.generate(prompts, count=C, temperature=0.0)[0]
    assert np.array_equal(gz, gd)
    db = D.generate(prompts, count=C, u=u, temperature=1.0, score=True)[1]
    assert not np.isfinite(db[[0, 2, 4, 5]]).any()                   # the unshifted softmax at these logits
    D.close()
    L.close()


def test_step_kernels_sampler_at_large_logits():
    """a STEP_KERNELS handle samples with k_sample"""
    import lstm_hip
    N, C = 64, 60
    P, _ = _large_params(N, seed=41, close_top=True)
    s = {k: v.astype(np.float64) for k, v in split_params(P, N).items()}
    u = np.random.RandomState(4).random_sample(C)
    L = lstm_hip.Lstm(N, 8, 4, flags=lstm_hip.STABLE_SOFTMAX | lstm_hip.STEP_KERNELS)
    L.set_params(P)
    out = L.sample(np.zeros(N, np.float32), np.zeros(N, np.float32), u)[0]
    L.close()
    assert _cdf_walk(s, N, [], u, out) >= 0.9 * C
    assert len(set(out.tolist())) >= 2


def test_batch_size_independence_with_the_flag():
    import lstm_hip
    N, C, K = 64, 24, 512
    P, _ = _large_params(N, seed=51, close_top=True)
    rs = np.random.RandomState(K)
    lengths = rs.randint(0, 20, size=K)
    prompts = [rs.randint(32, 127, size=n).astype(np.uint8) for n in lengths]
    h0 = (rs.randn(K, N) * 0.1).astype(np.float32)
    c0 = (rs.randn(K, N) * 0.1).astype(np.float32)
    u = rs.random_sample((C, K))
    L = lstm_hip.Lstm(N, 2, 1, flags=lstm_hip.STABLE_SOFTMAX)
    L.set_params(P)
    wide = L.generate(prompts, count=C, u=u, temperature=1.0, h0=h0, c0=c0, score=True)
    assert np.isfinite(wide[1]).all()
    for i in (0, 1, 15, 16, 255, 300, K - 1):
        one = L.generate([prompts[i]], count=C, u=u[:, i:i + 1], temperature=1.0, h0=h0[i:i + 1], c0=c0[i:i + 1], score=True)
        assert np.array_equal(wide[0][:, i], one[0][:, 0]), i
        assert same_bytes(wide[1][i:i + 1], one[1]), i
        assert same_bytes(wide[2][i], one[2][0]) and same_bytes(wide[3][i], one[3][0]), i
    L.close()


def test_padding_composes_with_the_flag():
    """(N = 500, PAD_HIDDEN | STABLE_SOFTMAX) against (512, STABLE_SOFTMAX) from the zero-padded parameters, at large logits"""
    import lstm_hip
    N, Np, S, B, lr = 500, 512, 7, 16, 0.1
    P, _ = _large_params(N, seed=61)
    g = lstm_hip.MT19937Normal(5)
    h1, c1 = g.randn(N, B, 0.0, 0.1), g.randn(N, B, 0.0, 0.1)
    text = np.random.RandomState(6).randint(32, 127, size=S * 40 + 7).astype(np.uint8)
    hs = []
    for n, flags, PP, h, c in ((N, lstm_hip.PAD_HIDDEN | lstm_hip.STABLE_SOFTMAX, P, h1, c1),
                               (Np, lstm_hip.STABLE_SOFTMAX, pad_params(P, N, Np), pad_cols(h1, N, Np), pad_cols(c1, N, Np))):
        L = lstm_hip.Lstm(n, S, B, flags=flags)
        L.set_params(PP)
        L.set_text(text)
        L.set_cursors(lstm_hip.initial_cursors(len(text), S, B))
        L.reset_window()
        L.set_state(1, h, c)
        hs.append(L)
    A, Bh = hs
    la, lb = A.train_windows(3, lr), Bh.train_windows(3, lr)
    assert np.isfinite(la).all() and la.max() > 100.0, la
    assert same_bytes(la, lb), (la, lb)
    for which in (lstm_hip.P_PARAMS, lstm_hip.P_GRADS, lstm_hip.P_MEM):
        assert same_bytes(pad_params(A.get_params(which), N, Np), Bh.get_params(which)), which
    A.close()
    Bh.close()


LSTM = os.path.join(ROOT, "eigen-lstm_amd", "lstm")
GEN = os.path.join(ROOT, "eigen-lstm_amd", "lstm_generate")


def test_program_trains_with_the_flag(tmp_path):
    import lstm_hip
    N, S, B, lr, windows = 32, 8, 4, 0.1, 60
    rs = np.random.RandomState(11)
    text = rs.randint(97, 110, size=3000).astype(np.uint8)
    f = tmp_path / "corpus.txt"
    text.tofile(f)
    out = subprocess.run([LSTM, str(f), str(N), str(S), str(B), str(lr), "--epochs", "1", "--windows", str(windows),
                          "--seed", "1", "--sample", "0", "--stable-softmax", "--save", str(tmp_path / "ck")],
                         capture_output=True, text=True, errors="replace", timeout=300)
    assert out.returncode == 0, out.stderr
    m = re.search(r"avg loss = ([\d.]+) bits/char", out.stdout)
    assert m, out.stdout
    # the same run in-process, from the start the program makes (the oracle trainer's, as test_host_driver.py checks)
    from oracle_lib import Oracle
    tr = Oracle("f32").trainer(text, N, S, B, lr=lr, seed=1)
    tr.epoch_reset()
    L = lstm_hip.Lstm(N, S, B, flags=lstm_hip.STABLE_SOFTMAX | lstm_hip.PAD_HIDDEN)
    L.set_params(tr.params.copy())
    L.set_state(1, tr.h[1], tr.c[1])
    L.set_text(text)
    L.set_cursors(lstm_hip.initial_cursors(len(text), S, B))
    L.reset_window()
    losses = L.train_windows(windows, lr)
    L.close()
    want = losses.sum() / (S * (windows + S))
    assert abs(float(m.group(1)) - want) <= 2e-3, (m.group(1), want)


def test_generate_program_scores_a_large_logit_checkpoint(tmp_path):
    rs = np.random.RandomState(81)
    text = rs.randint(97, 110, size=3000).astype(np.uint8)
    corpus = tmp_path / "corpus.txt"
    text.tofile(corpus)
    tr = subprocess.run([LSTM, str(corpus), "32", "8", "4", "0.1", "--epochs", "1", "--windows", "30", "--sample", "0",
                         "--save", str(tmp_path / "ck"), "--quiet"], capture_output=True, text=True, errors="replace", timeout=300)
    assert tr.returncode == 0, tr.stderr
    Why = np.loadtxt(tmp_path / "ck_Why.txt", ndmin=2) * 1000.0
    np.savetxt(tmp_path / "ck_Why.txt", Why, fmt="%.9g")
    score = tmp_path / "t.txt"
    rs.randint(97, 110, size=400).astype(np.uint8).tofile(score)
    run = lambda *extra: subprocess.run([GEN, "--load", str(tmp_path / "ck"), "--score", str(score), *extra],
                                        capture_output=True, text=True, errors="replace", timeout=300)
    a, b = run("--stable-softmax"), run()
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    ma = re.search(re.escape(str(score)) + r": (\S+) bits/char", a.stdout)
    mb = re.search(re.escape(str(score)) + r": (\S+) bits/char", b.stdout)
    assert ma and mb, (a.stdout, b.stdout)
    assert np.isfinite(float(ma.group(1))), a.stdout
    assert not np.isfinite(float(mb.group(1))), b.stdout
