"""-m gpu: the tail of a window inside the device-resident loop.

Inside lstm_hip_train_windows (single GPU, fused gradient sums, no clipping) the loss sum and the dby fold of a window and
the slide to the next window have no launch of their own: they ride in extra workgroups of the window's update launch, and
only the last window of a call stores the probabilities and the folded gradient.  Nothing of that may change a bit: every
comparison here is bitwise, between
  A  one train_windows(K) call,
  B  K train_windows(1) calls (standalone slide launch; every window is a last window), and
  C  the step-by-step calls: the slide done on the host (set_window, the carry through get_state / set_state), then
     forward, loss, backward, adagrad -- the separate loss / dby launch, the separate folds, every store."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _host_slide(xi, ti, pos, text, S, stride):
    """OV/lstm_eigen_opt/lstm.cc:190-213 on indices, `stride` times; in place."""
    for _ in range(stride):
        ev = text[pos.astype(np.int64)].astype(np.int32)
        pos += 1
        pos[pos >= len(text)] = S
        xi[:-1] = xi[1:].copy()
        ti[:-1] = ti[1:].copy()
        ti[S - 1] = ev
        xi[S - 1] = ti[S - 2]


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _blocks(lstm_hip, adam):
    return (lstm_hip.P_PARAMS, lstm_hip.P_MEM) + ((lstm_hip.P_ADAM_V,) if adam else ())


# N, S, B, flag names, stride, carry column, text length, windows, Adam, fused sums expected
CASES = [
    pytest.param(512, 100, 64, (), 1, 1, 200_000, 5, False, True, id="headline"),
    pytest.param(256, 32, 63, (), 1, 1, 50_000, 6, False, None, id="columns-2016-ragged-batch"),
    pytest.param(256, 33, 63, (), 1, 1, 50_000, 6, False, None, id="columns-2079-ragged-batch"),
    pytest.param(128, 20, 12, (), 3, 2, 50_000, 7, False, None, id="stride3-carry2"),
    pytest.param(256, 50, 32, (), 7, 6, 50_000, 5, False, None, id="stride7-carry6"),
    pytest.param(128, 16, 20, (), 1, 1, 16 + 5, 14, False, None, id="text-wraps-every-5"),
    pytest.param(128, 16, 20, (), 3, 2, 16 + 4, 9, False, None, id="text-wraps-stride3"),
    pytest.param(100, 24, 16, ("PAD_HIDDEN",), 1, 1, 50_000, 5, False, None, id="pad-hidden"),
    pytest.param(500, 30, 64, ("PAD_HIDDEN",), 1, 1, 50_000, 4, False, None, id="pad-hidden-500"),
    pytest.param(256, 50, 32, ("STABLE_SOFTMAX",), 1, 1, 50_000, 5, False, None, id="stable-softmax"),
    pytest.param(512, 100, 64, (), 1, 1, 200_000, 4, True, True, id="headline-adam"),
    pytest.param(128, 20, 12, (), 3, 2, 50_000, 6, True, None, id="stride3-adam"),
]


@pytest.mark.parametrize("N,S,B,flag_names,stride,carry,text_len,K,adam,fused", CASES)
def test_loop_equals_single_windows_and_step_by_step(N, S, B, flag_names, stride, carry, text_len, K, adam, fused):
    import lstm_hip
    from bench import synthetic_text
    flags = 0
    for f in flag_names:
        flags |= getattr(lstm_hip, f)
    lr = 0.01
    text = synthetic_text(text_len, seed=3)
    pos = np.array([S + (3 * b) % (text_len - S) for b in range(B)], np.uint64) if text_len < 1000 \
        else lstm_hip.initial_cursors(text_len, S, B)
    xi, ti = np.full((S, B), -1, np.int32), np.full((S, B), -1, np.int32)
    _host_slide(xi, ti, pos, text, S, S)  # a full first window
    rs = np.random.RandomState(7)
    h0, c0 = (rs.randn(B, N) * 0.1).astype(np.float32), (rs.randn(B, N) * 0.1).astype(np.float32)
    P0 = lstm_hip.init_params(lstm_hip.MT19937Normal(2), N)
    P0[-256:] = (rs.randn(256) * 0.01).astype(np.float32)  # by: its update is the carried workgroups' own

    Ls = []
    for _ in range(3):
        L = lstm_hip.Lstm(N, S, B, flags=flags)
        L.set_params(P0)
        if adam:
            L.set_optimizer(lstm_hip.OPT_ADAM, weight_decay=0.01)
        L.set_text(text)
        L.set_cursors(pos)
        L.set_stride(stride, carry)
        L.set_window(xi, ti)
        L.set_state(carry, h0, c0)  # becomes column 0 of the first trained window
        Ls.append(L)
    A, Bh, Cs = Ls
    try:
        if fused is not None:
            assert ("fused1" in A.plan_identity()) == fused, A.plan_identity()
        la = A.train_windows(K, lr)
        lb = np.array([Bh.train_windows(1, lr)[0] for _ in range(K)])
        lc = []
        for _ in range(K):
            _host_slide(xi, ti, pos, text, S, stride)
            Cs.set_window(xi, ti)
            Cs.set_state(0, *Cs.get_state(carry))
            Cs.forward()
            lc.append(Cs.loss())
            Cs.backward()
            Cs.adagrad(lr)
        lc = np.array(lc)
        assert np.all(np.isfinite(la))
        assert _same(la, lb), (la, lb)
        assert _same(la, lc), (la, lc)
        for which in _blocks(lstm_hip, adam):
            pa = A.get_params(which)
            assert _same(pa, Bh.get_params(which)), which
            assert _same(pa, Cs.get_params(which)), which
        assert not _same(A.get_params()[-256:], P0[-256:])  # by moved
        for L in (A, Bh):
            assert np.array_equal(L.get_cursors(), pos)
            wx, wt = L.get_window()
            assert np.array_equal(wx, xi) and np.array_equal(wt, ti)
        # what only the last window of a call stores: the folded gradient and the probabilities, against the standalone
        # backward / forward of the same window
        ga = A.get_grads()
        assert _same(ga, Bh.get_grads()) and _same(ga, Cs.get_grads())
        for t in (1, S // 2, S - 1):
            (g_a, p_a), (g_b, p_b), (g_c, p_c) = A.get_activations(t), Bh.get_activations(t), Cs.get_activations(t)
            assert _same(p_a, p_b) and _same(p_a, p_c), t
            assert _same(g_a, g_b) and _same(g_a, g_c), t
            assert abs(float(p_a.sum()) - B) < 1e-3 * B
        for t in (0, 1, S - 1):
            for x, y, z in zip(A.get_state(t), Bh.get_state(t), Cs.get_state(t)):
                assert _same(x, y) and _same(x, z), t
        # the loop goes on from where it stopped (cursor and head copies flipped an odd / even number of times)
        la2 = A.train_windows(3, lr)
        lb2 = np.array([Bh.train_windows(1, lr)[0] for _ in range(3)])
        assert _same(la2, lb2)
        assert np.array_equal(A.get_cursors(), Bh.get_cursors())
        assert _same(A.get_params(), Bh.get_params())
    finally:
        for L in Ls:
            L.close()


def test_set_cursors_between_calls_is_honoured():
    """The live cursor copy is whichever half the last carried slide wrote: set_cursors / get_cursors must reach it."""
    import lstm_hip
    from bench import synthetic_text
    N, S, B = 128, 20, 12
    text = synthetic_text(30_000, seed=4)
    out = []
    for counts in ((2, 3), (2, 1, 1, 1)):
        L = lstm_hip.Lstm(N, S, B)
        L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(2), N))
        L.set_text(text)
        L.set_cursors(lstm_hip.initial_cursors(len(text), S, B))
        L.reset_window()
        L.train_windows(counts[0], 0.01)
        L.set_cursors(np.arange(B, dtype=np.uint64) * 100 + S)
        assert np.array_equal(L.get_cursors(), np.arange(B, dtype=np.uint64) * 100 + S)
        losses = np.concatenate([L.train_windows(c, 0.01) for c in counts[1:]])
        out.append((losses, L.get_cursors(), L.get_params()))
        L.close()
    for a, b in zip(*out):
        assert _same(a, b)
    assert np.array_equal(out[0][1], np.arange(B, dtype=np.uint64) * 100 + S + 3)


def test_two_handles_in_lock_step_at_the_headline_shape():
    import lstm_hip
    from bench import synthetic_text
    N, S, B = 512, 100, 64
    text = synthetic_text(200_000, seed=0)
    Ls = []
    for _ in range(2):
        L = lstm_hip.Lstm(N, S, B)
        L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(1), N))
        L.set_text(text)
        L.set_cursors(lstm_hip.initial_cursors(len(text), S, B))
        Ls.append(L)
    try:
        for chunk in (1, 2, 997, 1000, 1000):  # 3 000 windows; odd and even numbers of carried slides per call
            la, lb = (L.train_windows(chunk, 0.005) for L in Ls)
            assert np.all(np.isfinite(la))
            assert _same(la, lb), f"first differing window: {int(np.argmax(la != lb))}"
        for which in (lstm_hip.P_PARAMS, lstm_hip.P_MEM, lstm_hip.P_GRADS):
            assert _same(Ls[0].get_params(which), Ls[1].get_params(which)), which
        assert np.array_equal(Ls[0].get_cursors(), Ls[1].get_cursors())
        for a, b in zip(Ls[0].get_window(), Ls[1].get_window()):
            assert np.array_equal(a, b)
    finally:
        for L in Ls:
            L.close()
