"""-m gpu: gradient accumulation (lstm_hip_set_grad_accumulation), bitwise throughout.

The construction is tests/test_window_tail.py's: same init, text, cursors and carried state.
  A  has accumulation on and runs train_windows;
  C  has it off and runs the step-by-step calls with the slide on the host: forward, loss, backward, get_grads per window, the
     float32 running sum kept in NumPy in window order, and on every K-th window set_params(total, P_GRADS) and adagrad(lr).
After every window A's accumulator, pending count, gradient block and loss are held against C's (A one window per call), and
at the end every block, the step count, the cursors, the window and the states.  Every case is also run with every = 1, C
updating at each window: the control that the loop and the steps agree at that shape without the feature.

One comparison is not bitwise: at 128x20x12 the accumulator is also held against the float32 oracle, window by window from
A's own parameters and state, at grad_accum_ref's tolerance: per tensor GRAD_TOL * sum_w max|g_w| / max|sum_w g_w| + n 2^-24
with tests/test_hip_parity.py's GRAD_TOL = 2e-4, i.e. 2e-4 for one window and at most a few times that for a cycle (the
figure of every cycle is printed)."""
import numpy as np
import pytest

import grad_accum_ref as ref

pytestmark = pytest.mark.gpu
LR = 0.01


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class Case:
    def __init__(self, N, S, B, every, windows, flags=(), stride=1, carry=1, mean=False, adam=False, clip=False, drop=0.0,
                 plan=(), more=0):
        self.N, self.S, self.B, self.every, self.windows, self.flags = N, S, B, every, windows, flags
        self.stride, self.carry, self.mean, self.adam, self.clip, self.drop, self.plan, self.more = \
            stride, carry, mean, adam, clip, drop, plan, more


# `plan`: what plan_identity() must say, so that the path is asserted and not believed
CASES = [
    pytest.param(Case(128, 20, 12, 3, 7, stride=3, carry=2, more=2), id="stride3-carry2-ends-pending1"),
    pytest.param(Case(256, 32, 63, 2, 6, adam=True, clip=True), id="adamw-clipped"),
    pytest.param(Case(512, 100, 64, 4, 8, mean=True, plan=("fused1",)), id="fused-groups-slabs-mean"),
    pytest.param(Case(100, 24, 16, 3, 7, flags=("PAD_HIDDEN",)), id="pad-hidden"),
    pytest.param(Case(80, 12, 8, 2, 5, plan=("fused0",)), id="per-step-engine"),
    pytest.param(Case(256, 20, 16, 2, 5, flags=("NO_FUSED_GRADS",), plan=("fused0",)), id="no-fused-grads"),
    pytest.param(Case(128, 16, 8, 2, 5, flags=("BF16_RECURRENCE",), plan=("fused0",)), id="bf16"),
    pytest.param(Case(128, 20, 12, 3, 7, drop=0.5), id="weight-drop"),
]


class Run:
    """the inputs of a case and handles made from them"""

    def __init__(self, lstm_hip, case, text_len=50_000):
        from bench import synthetic_text
        self.m, self.c = lstm_hip, case
        N, S, B = case.N, case.S, case.B
        self.flags = 0
        for f in case.flags:
            self.flags |= getattr(lstm_hip, f)
        self.text = synthetic_text(text_len, seed=3)
        self.pos0 = lstm_hip.initial_cursors(text_len, S, B)
        self.xi0, self.ti0 = np.full((S, B), -1, np.int32), np.full((S, B), -1, np.int32)
        ref.host_slide(self.xi0, self.ti0, self.pos0, self.text, S, S)  # a full first window
        rs = np.random.RandomState(7)
        self.h0, self.c0 = (rs.randn(B, N) * 0.1).astype(np.float32), (rs.randn(B, N) * 0.1).astype(np.float32)
        self.P0 = lstm_hip.init_params(lstm_hip.MT19937Normal(2), N)
        self.P0[-256:] = (rs.randn(256) * 0.01).astype(np.float32)
        self.handles = []

    def handle(self, every, mean=False, max_norm=0.0):
        m, c = self.m, self.c
        L = m.Lstm(c.N, c.S, c.B, flags=self.flags)
        self.handles.append(L)
        L.set_params(self.P0)
        if c.adam:
            L.set_optimizer(m.OPT_ADAM, weight_decay=0.01)
        if max_norm:
            L.set_grad_clip(max_norm)
        if c.drop:
            L.set_weight_drop(c.drop, seed=5, t=3)
        L.set_text(self.text)
        L.set_cursors(self.pos0)
        L.set_stride(c.stride, c.carry)
        L.set_window(self.xi0, self.ti0)
        L.set_state(c.carry, self.h0, self.c0)  # becomes column 0 of the first trained window
        if every is not None:
            L.set_grad_accumulation(every, mean)
        words = L.plan_identity().split()
        for word in c.plan:
            assert word in words, words
        if "fused1" in c.plan:  # more than one column group to fold, and dU in split-K slabs
            num = {w.rstrip("0123456789"): int(w[len(w.rstrip("0123456789")):]) for w in words}
            assert 0 < num["gp"] < c.B and num["su"] > 1, words
        return L

    def close(self):
        for L in self.handles:
            L.close()


def _blocks(m, L, adam):
    out = {"params": L.get_params(m.P_PARAMS), "mem": L.get_params(m.P_MEM), "grads": L.get_grads(), "steps": L.optimizer_steps()}
    if adam:
        out["v"] = L.get_params(m.P_ADAM_V)
    return out


def _end_state(m, L, case):
    out = _blocks(m, L, case.adam)
    out["cursors"] = L.get_cursors()
    out["xi"], out["ti"] = L.get_window()
    for t in (0, 1, case.S - 1):
        out[f"h{t}"], out[f"c{t}"] = L.get_state(t)
    if case.drop:
        out["drop"] = np.array(L.weight_drop()[2], np.uint64)
    return out


def _assert_same(a, b, what):
    assert a.keys() == b.keys(), (what, a.keys(), b.keys())
    for k in a:
        assert _same(np.asarray(a[k]), np.asarray(b[k])), (what, k)


def _steps(run, L, windows, every, mean, state=None):
    """C: `windows` step-by-step windows on handle L with the host's running sum.  Returns per window (loss, accumulator after
    it or zeros, pending, gradient block after it), the norms of the updates, and the host state to go on from."""
    m, c = run.m, run.c
    if state is None:
        state = dict(xi=run.xi0.copy(), ti=run.ti0.copy(), pos=run.pos0.copy(), total=None, pending=0)
    rec, norms = [], []
    for _ in range(windows):
        ref.host_slide(state["xi"], state["ti"], state["pos"], run.text, c.S, c.stride)
        L.set_window(state["xi"], state["ti"])
        L.set_state(0, *L.get_state(c.carry))
        L.forward()
        loss = L.loss()
        L.backward()
        g = L.get_grads()
        assert g.dtype == np.float32
        state["total"] = g if state["pending"] == 0 else state["total"] + g
        state["pending"] += 1
        d = g
        if state["pending"] == every:
            if every > 1:
                d = state["total"] * np.float32(1.0 / every) if mean else state["total"]
                L.set_params(d, m.P_GRADS)
            L.adagrad(LR)
            if c.clip:
                norms.append(L.grad_norms()[0])
            state["pending"] = 0
        rec.append((loss, np.zeros_like(g) if state["pending"] == 0 else state["total"].copy(), state["pending"], d.copy()))
    return rec, np.array(norms), state


def _host_end_state(m, L, case, state):
    out = _end_state(m, L, case)
    out["cursors"], out["xi"], out["ti"] = state["pos"], state["xi"], state["ti"]  # (the handle has no cursors: the host slid)
    return out


def _compare(run, every, mean, max_norm=0.0):
    """A in one call and A one window per call against C; returns A's norms"""
    m, c = run.m, run.c
    A, A1, C = run.handle(every, mean, max_norm), run.handle(every, mean, max_norm), run.handle(None, False, max_norm)
    rec, norms_c, state = _steps(run, C, c.windows, every, mean)
    la = A.train_windows(c.windows, LR)
    norms_a = A.grad_norms() if c.clip else np.zeros(0)
    assert np.all(np.isfinite(la))
    assert _same(la, np.array([r[0] for r in rec])), (la, [r[0] for r in rec])
    for w, (loss, acc, pending, d) in enumerate(rec):
        assert A1.train_windows(1, LR)[0] == loss, w
        assert _same(A1.get_grads(), d), w
        if every > 1:
            assert A1.grad_accumulation() == (every, mean, pending), w
            assert _same(A1.grad_accumulator(), acc), w
            if c.flags == ("PAD_HIDDEN",):
                assert acc.size == m.param_count(c.N)  # the logical block
    assert every == 1 or A.grad_accumulation() == (every, mean, c.windows % every)
    assert A.optimizer_steps() == c.windows // every
    want = _host_end_state(m, C, c, state)
    _assert_same(_end_state(m, A, c), want, "one call")
    _assert_same(_end_state(m, A1, c), want, "one window per call")
    if every > 1:
        assert _same(A.grad_accumulator(), A1.grad_accumulator())
    if c.clip:
        assert len(norms_a) == c.windows // every and _same(norms_a, norms_c), (norms_a, norms_c)
    if c.more and every > 1:  # go on from a half-full accumulator
        rec2, _, state = _steps(run, C, c.more, every, mean, state)
        la2 = A.train_windows(c.more, LR)
        assert _same(la2, np.array([r[0] for r in rec2]))
        _assert_same(_end_state(m, A, c), _host_end_state(m, C, c, state), "continued")
        assert A.grad_accumulation() == (every, mean, rec2[-1][2]) and _same(A.grad_accumulator(), rec2[-1][1])
    return norms_a


@pytest.mark.parametrize("case", CASES)
def test_control_loop_equals_steps_without_accumulation(case):
    import lstm_hip
    run = Run(lstm_hip, case)
    try:
        max_norm = float("inf") if case.clip else 0.0
        _compare(run, 1, False, max_norm)
    finally:
        run.close()


@pytest.mark.parametrize("case", CASES)
def test_accumulating_loop_equals_steps_with_the_sum_on_the_host(case):
    import lstm_hip
    run = Run(lstm_hip, case)
    try:
        max_norm = 0.0
        if case.clip:  # the bound from a measure-only run of the same case: the median of its norms
            measured = _compare(run, case.every, case.mean, float("inf"))
            assert len(measured) == 3
            max_norm = float(np.median(measured))
        norms = _compare(run, case.every, case.mean, max_norm)
        if case.clip:
            scaled = max_norm / (norms + 1e-6) < 1.0
            print("norms", norms, "max_norm", max_norm)
            assert scaled.any() and not scaled.all(), (norms, max_norm)
    finally:
        run.close()


@pytest.mark.parametrize("case", CASES)
def test_chunking_shows_nowhere(case):
    import lstm_hip
    run = Run(lstm_hip, case)
    try:
        ends = []
        for chunks in ((8,), (3, 5), (1,) * 8):
            L = run.handle(case.every, case.mean, 1.0 if case.clip else 0.0)
            losses = np.concatenate([L.train_windows(n, LR) for n in chunks])
            end = _end_state(lstm_hip, L, case)
            end["losses"], end["acc"], end["pending"] = losses, L.grad_accumulator(), np.array(L.grad_accumulation()[2])
            ends.append(end)
        assert int(ends[0]["pending"]) == 8 % case.every
        _assert_same(ends[0], ends[1], "3 + 5")
        _assert_same(ends[0], ends[2], "8 x 1")
    finally:
        run.close()


def test_off_is_off_and_the_launch_counts():
    import lstm_hip
    case = Case(128, 20, 12, 4, 8)
    run = Run(lstm_hip, case)
    try:
        plain, off = run.handle(None), run.handle(1)
        lp, lo = plain.train_windows(5, LR), off.train_windows(5, LR)
        assert _same(lp, lo)
        _assert_same(_end_state(lstm_hip, plain, case), _end_state(lstm_hip, off, case), "every = 1")
        for L in (plain, off):  # (launches are counted in a profiling pass)
            L.set_profiling(True)
            L.reset_kernel_stats()
            L.train_windows(5, LR)
        sp, so = plain.kernel_stats(), off.kernel_stats()
        assert {k: v[0] for k, v in sp.items()} == {k: v[0] for k, v in so.items()}
        assert sp["grad_accumulate"][0] == 0 and sp["adagrad"][0] == 5
        with pytest.raises(lstm_hip.LstmHipError):
            off.grad_accumulator()
        on = run.handle(4)
        on.set_averaging(lstm_hip.AVG_EMA, 0.9)
        on.set_profiling(True)
        on.reset_kernel_stats()
        on.train_windows(8, LR)
        st = on.kernel_stats()
        assert st["adagrad"][0] == 2 and st["grad_accumulate"][0] == 8, st
        assert on.optimizer_steps() == 2 and on.averaging_counts() == (2, 2)
        assert on.grad_accumulation() == (4, False, 0)
    finally:
        run.close()


def test_setting_again_keeps_and_a_new_pair_discards():
    import lstm_hip
    case = Case(128, 20, 12, 3, 2)
    run = Run(lstm_hip, case)
    try:
        L = run.handle(3)
        L.train_windows(2, LR)
        acc = L.grad_accumulator()
        assert L.grad_accumulation() == (3, False, 2) and np.any(acc != 0)
        L.set_grad_accumulation(3, False)
        assert L.grad_accumulation() == (3, False, 2) and _same(L.grad_accumulator(), acc)
        L.set_grad_accumulation(3, True)
        assert L.grad_accumulation() == (3, True, 0) and not np.any(L.grad_accumulator())
        L.train_windows(1, LR)
        L.set_grad_accumulation(1)
        assert L.grad_accumulation() == (1, False, 0)
        L.set_grad_accumulation(3, True)
        assert L.grad_accumulation() == (3, True, 0)
    finally:
        run.close()


def test_resume_from_a_saved_accumulator():
    import lstm_hip
    m = lstm_hip
    case = Case(128, 20, 12, 3, 5, stride=3, carry=2, adam=True)
    run = Run(lstm_hip, case)
    try:
        A = run.handle(3, True)
        A.train_windows(5, LR)
        every, mean, pending = A.grad_accumulation()
        assert (every, mean, pending) == (3, True, 2)
        F = m.Lstm(case.N, case.S, case.B)
        run.handles.append(F)
        F.set_optimizer(m.OPT_ADAM, weight_decay=0.01)
        for which in (m.P_PARAMS, m.P_MEM, m.P_ADAM_V):
            F.set_params(A.get_params(which), which)
        F.set_optimizer_steps(A.optimizer_steps())
        F.set_grad_accumulation(every, mean)
        F.set_grad_accumulator(A.grad_accumulator(), pending)
        F.set_text(run.text)
        F.set_cursors(A.get_cursors())
        F.set_stride(case.stride, case.carry)
        F.set_window(*A.get_window())
        F.set_state(case.carry, *A.get_state(case.carry))
        assert F.grad_accumulation() == (3, True, 2) and _same(F.grad_accumulator(), A.grad_accumulator())
        la, lf = A.train_windows(4, LR), F.train_windows(4, LR)
        assert _same(la, lf), (la, lf)
        ea, ef = _end_state(m, A, case), _end_state(m, F, case)
        _assert_same(ea, ef, "resumed")
        assert A.grad_accumulation() == F.grad_accumulation() == (3, True, 0) and A.optimizer_steps() == 3
    finally:
        run.close()


def test_text_windows_accumulate_and_cut_anywhere():
    """The step-by-step calls do not exist for the text windows: the accumulator is held against the float32 running sum of
    each window's own get_grads(), and each update against a twin handle loaded with A's blocks from before it."""
    import lstm_hip
    m = lstm_hip
    N, S, B, every = 128, 12, 8, 2
    rs = np.random.RandomState(5)
    lengths = [5, 40, 3, 17, 29, 2, 11, 33, 8, 23, 14, 6]
    texts = [rs.randint(32, 127, size=n).astype(np.uint8) for n in lengths]
    weights = [rs.rand(n).astype(np.float32) if s % 2 == 0 else 1.0 for s, n in enumerate(lengths)]
    P0 = m.init_params(m.MT19937Normal(2), N)
    made = []

    def handle(acc):
        L = m.Lstm(N, S, B)
        made.append(L)
        L.set_params(P0)
        L.set_optimizer(m.OPT_ADAM, weight_decay=0.01)
        if acc:
            L.set_grad_accumulation(every)
        return L

    try:
        A, W, T = handle(True), handle(True), handle(False)
        windows = A.set_train_texts(texts, weights)
        assert W.set_train_texts(texts, weights) == windows and windows >= 4
        lw = W.train_text_windows(windows, LR)
        la, total, pending = [], None, 0
        for w in range(windows):
            before = [A.get_params(which) for which in (m.P_PARAMS, m.P_MEM, m.P_ADAM_V)], A.optimizer_steps()
            la.append(A.train_text_windows(1, LR)[0])
            g = A.get_grads()
            if pending + 1 < every:
                total = g if pending == 0 else total + g
                pending += 1
                assert A.grad_accumulation() == (every, False, pending) and _same(A.grad_accumulator(), total), w
                for which, blk in zip((m.P_PARAMS, m.P_MEM, m.P_ADAM_V), before[0]):
                    assert _same(A.get_params(which), blk), (w, which)
                assert A.optimizer_steps() == before[1]
            else:  # an update window: get_grads() is the cycle's block, and the twin makes the same update from it
                pending = 0
                assert A.grad_accumulation() == (every, False, 0) and not np.any(A.grad_accumulator()), w
                for which, blk in zip((m.P_PARAMS, m.P_MEM, m.P_ADAM_V), before[0]):
                    T.set_params(blk, which)
                T.set_optimizer_steps(before[1])
                T.set_params(g, m.P_GRADS)
                T.adagrad(LR)
                for which in (m.P_PARAMS, m.P_MEM, m.P_ADAM_V):
                    assert _same(A.get_params(which), T.get_params(which)), (w, which)
                assert not _same(A.get_params(), before[0][0])
        assert np.all(np.isfinite(la))
        assert _same(np.array(la), lw)
        for which in (m.P_PARAMS, m.P_MEM, m.P_ADAM_V, m.P_GRADS):
            assert _same(A.get_params(which), W.get_params(which)), which
        assert A.grad_accumulation() == W.grad_accumulation() and _same(A.grad_accumulator(), W.grad_accumulator())
        assert A.optimizer_steps() == W.optimizer_steps() == windows // every
        assert _same(A.train_texts_bits(), W.train_texts_bits())
    finally:
        for L in made:
            L.close()


def test_text_windows_update_block_is_the_sum_of_its_windows():
    """... and that block itself: with every = 2 the block of an update window is the float32 sum of the two windows' own
    gradients, the second taken from a handle that ran the same windows and stopped accumulating one window earlier."""
    import lstm_hip
    m = lstm_hip
    N, S, B = 128, 12, 8
    rs = np.random.RandomState(5)
    lengths = [5, 40, 3, 17, 29, 2, 11, 33, 8, 23, 14, 6]
    texts = [rs.randint(32, 127, size=n).astype(np.uint8) for n in lengths]
    P0 = m.init_params(m.MT19937Normal(2), N)
    made = []
    try:
        A, G = m.Lstm(N, S, B), m.Lstm(N, S, B)
        made += [A, G]
        for L in (A, G):
            L.set_params(P0)
            L.set_train_texts(texts)
        A.set_grad_accumulation(2)
        G.set_grad_accumulation(3)  # never reaches an update in two windows: the same windows at the same parameters
        A.train_text_windows(1, LR)
        G.train_text_windows(1, LR)
        g0 = G.get_grads()
        assert _same(A.get_grads(), g0) and _same(A.grad_accumulator(), g0)
        A.train_text_windows(1, LR)
        G.train_text_windows(1, LR)
        g1 = G.get_grads()
        assert _same(A.get_grads(), g0 + g1) and _same(G.grad_accumulator(), g0 + g1)
        assert A.optimizer_steps() == 1 and G.optimizer_steps() == 0 and _same(G.get_params(), P0)
    finally:
        for L in made:
            L.close()


def test_accumulator_against_the_oracle(oracle32):
    """128x20x12, K = 3, 7 windows: each window's reference gradient from the float32 oracle at A's own parameters, window
    and carried state; A's records against their sums at grad_accum_ref's tolerance (the module docstring)."""
    import lstm_hip
    case = Case(128, 20, 12, 3, 7, stride=3, carry=2)
    run = Run(lstm_hip, case)
    N, S, B = case.N, case.S, case.B
    try:
        A = run.handle(3)
        got, want, total, pending = [], [], None, 0
        for w in range(case.windows):
            P = A.get_params()
            A.train_windows(1, LR)
            xi, ti = A.get_window()
            h0, c0 = A.get_state(0)
            fw = oracle32.forward(N, 256, S, B, P, xi, ti, h0, c0)
            g = oracle32.backward(N, 256, S, B, P, xi, ti, fw)
            total = g if pending == 0 else total + g
            pending = (pending + 1) % 3
            want.append((np.zeros_like(g) if pending == 0 else total.copy(), pending, g, total.copy() if pending == 0 else g))
            got.append((A.grad_accumulator(), A.grad_accumulation()[2], None, A.get_grads()))
            if pending != 1:
                print("window", w, "tolerance of the cycle so far:", ref.accum_tolerance([r[2] for r in want[-(pending or 3):]], N))
        ok, worst = ref.accumulators_agree(got, want, N)
        print("worst error / tolerance:", worst)
        assert ok, worst
    finally:
        run.close()


def test_program_accumulates_saves_and_resumes(tmp_path):
    """lstm --accumulate K [--accumulate-mean]: --save writes what is pending and its state, --load with the same setting
    resumes it and with another ignores it; the epoch line is as without it."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lstm = os.path.join(root, "eigen-lstm_amd", "lstm")
    corpus = tmp_path / "corpus.txt"
    np.random.RandomState(81).randint(97, 110, size=3000).astype(np.uint8).tofile(corpus)

    def run(*args):
        out = subprocess.run([lstm, str(corpus), "64", "8", "4", "0.1", "--epochs", "1", "--sample", "0", "--quiet"] + list(args),
                             capture_output=True, text=True, errors="replace", timeout=300)
        assert out.returncode == 0, out.stderr
        return out.stdout

    ck, ck2 = str(tmp_path / "ck"), str(tmp_path / "ck2")
    first = run("--windows", "10", "--save", ck, "--accumulate", "3", "--accumulate-mean", "--clip-norm", "5")
    assert open(ck + "_accum_state.txt").read() == "every 3\nmean 1\npending 1\n"
    assert "of 3 windows (--clip-norm 5)" in first  # one norm per update: three updates in ten windows
    acc = np.loadtxt(ck + "_accum_b.txt", ndmin=2)
    assert acc.size == 4 * 64 and np.any(acc != 0)
    again = run("--windows", "5", "--load", ck, "--save", ck2, "--accumulate", "3", "--accumulate-mean")
    assert "Loaded the gradient accumulator (every = 3, pending = 1)" in again and "Epoch 1/1" in again
    assert open(ck2 + "_accum_state.txt").read() == "every 3\nmean 1\npending 0\n"  # 1 + 5 windows: two whole cycles
    assert not np.any(np.loadtxt(ck2 + "_accum_b.txt", ndmin=2))
    other = run("--windows", "5", "--load", ck, "--accumulate", "2")
    assert "Loaded the gradient accumulator" not in other and "Loaded Adagrad memory" in other
