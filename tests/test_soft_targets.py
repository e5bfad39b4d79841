"""-m gpu: lstm_hip_set_soft_targets -- label smoothing and distillation from a teacher (include/lstm_hip.h; DESIGN.md section
3.19).

One window in lock-step with the reference of tests/soft_target_ref.py (the unchanged oracle, any dy back-propagated through
it) on every engine form of its table and every setting; then the device loop against five such windows with both handles
carried by hand, chunking and determinism, the off rule, what a borrowed teacher keeps, the interaction with clipping, Adam
and weight drop, and the refusals.  Tolerances and comparison rules are those of
tests/test_hip_parity.py::test_window_matches_oracle (bf16: of its test_bf16_recurrence_matches_bf16_oracle); the KL figure is
held to the loss's tolerance per step.  The reference's own checks and its mutants are in tests/test_soft_targets_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import gpu_util as gu
import soft_target_ref as sr

pytestmark = pytest.mark.gpu
LR = sr.LR
IDS = [sr.case_id(c) for c in sr.CASES]


def _flags(names):
    import lstm_hip
    flags = 0
    for f in names:
        flags |= getattr(lstm_hip, f)
    return flags


def _pair(case):
    import lstm_hip
    (N, S, B, flags), (Nt, tflags) = case
    return lstm_hip.Lstm(N, S, B, flags=_flags(flags)), lstm_hip.Lstm(Nt, S, B, flags=_flags(tflags))


def _close(*handles):
    for L in handles:          # students first: a held teacher refuses to go
        L.close()


def _columns(L):
    S = L.S
    hs, cs = zip(*(L.get_state(t) for t in range(S)))
    gs, ps = zip(*(L.get_activations(t) for t in range(1, S)))
    return np.stack(hs), np.stack(cs), np.stack(gs), np.stack(ps)


def _oracle(case, oracle32, oracle64):
    return oracle32 if sr.is_bf16(case[0][3]) else oracle64


@pytest.mark.parametrize("case", sr.CASES, ids=IDS)
def test_window_in_lock_step_with_the_reference(case, oracle32, oracle64):
    import lstm_hip
    (N, S, B, flags), _ = case
    bf16 = sr.is_bf16(flags)
    orc = _oracle(case, oracle32, oracle64)
    act_tol, loss_tol, grad_tol = sr.tolerances(case)
    inp = sr.case_inputs(case)
    L, T = _pair(case)
    try:
        T.set_params(inp["Pt"])
        for i, setting in enumerate(sr.SETTINGS):
            teacher = i > 0
            want = sr.window(orc, case, inp, setting, teacher=teacher)
            L.set_params(inp["P"])
            L.set_params(np.zeros_like(inp["P"]), lstm_hip.P_MEM)
            L.set_window(inp["xi"], inp["ti"])
            L.set_state(0, inp["h0"], inp["c0"])
            T.set_state(0, inp["ht0"], inp["ct0"])
            L.set_soft_targets(T if teacher else None, *setting)
            got_t, a, tau, eps = L.soft_targets()
            assert (got_t is T if teacher else got_t is None) and (a, tau, eps) == setting
            L.forward()
            loss = L.loss()
            h, c, g, p = _columns(L)
            fw = want["fw"]
            act = 0.0
            for t in range(1, S):
                for name, got in (("h", h[t]), ("c", c[t]), ("g", g[t - 1]), ("probs", p[t - 1])):
                    act = max(act, gu.max_rel(got, fw[name][t]))
            fig = dict(act=act, loss=abs(loss - fw["loss_bits"]))        # the loss is the hard-target loss
            if teacher:
                kl = L.teacher_kl()
                assert kl.shape == (1,)
                fig["kl"] = abs(kl[0] - want["kl"])
                ht, ct = zip(*(T.get_state(t) for t in range(S)))       # the teacher ran on the student's inputs
                fig["teacher"] = max(gu.max_rel(ht[t], want["fwt"]["h"][t]) for t in range(1, S))
            else:
                with pytest.raises(lstm_hip.LstmHipError, match="no teacher"):
                    L.teacher_kl(1)
            L.backward()
            grads = L.get_grads()
            rep = gu.grads_report(grads, want["grads"], N)
            fig["grad"] = max(rep.values())
            L.adagrad(LR)
            if not bf16:  # (test_train_texts.py's rule: no bound for the step under bf16)
                Pref, mref = sr.adagrad_ref(orc, inp["P"], want["grads"], np.zeros_like(inp["P"]), LR)
                dref = np.asarray(want["grads"])
                mask = np.abs(dref) > 1e-3 * np.abs(dref).max()
                fig["step"] = float(np.abs(L.get_params()[mask] - Pref[mask]).max())
            print(f"{sr.case_id(case)} {setting}: " + ", ".join(f"{k} {v:.3g}" for k, v in fig.items()))
            assert fig["act"] <= act_tol, (setting, fig)
            assert fig["loss"] <= loss_tol * (S - 1), (setting, fig, loss, fw["loss_bits"])
            if teacher:
                assert fig["kl"] <= loss_tol * (S - 1), (setting, fig, kl[0], want["kl"])
                assert fig["teacher"] <= (2e-3 if sr.is_bf16(case[1][1]) else 2e-5), (setting, fig)
            assert fig["grad"] <= grad_tol, (setting, rep)
            if not bf16:
                assert fig["step"] <= 2e-4 * LR + 1e-6, (setting, fig)
                np.testing.assert_allclose(L.get_params(lstm_hip.P_MEM), mref, rtol=1e-3, atol=1e-3 * float(mref.max()))
    finally:
        _close(L, T)


# ---- the device loop -------------------------------------------------------------------------------------------------------
LOOP_CASES = [sr.CASES[1], sr.CASES[3], sr.CASES[6]]
LOOP_SETTING = (0.5, 2.0, 0.1)


def _text(S, B, seed):
    return gu.text_bytes(40 * S + 7 * B, seed)


def _loop_start(case, stride=None, teacher=True, setting=LOOP_SETTING):
    """student and teacher ready for train_windows: the window loop's first slide takes column carry_col as the carry, so
    the start states go there"""
    import lstm_hip
    (N, S, B, flags), _ = case
    inp = sr.case_inputs(case)
    L, T = _pair(case)
    text = _text(S, B, N + B)
    carry = 1
    if stride is not None:
        L.set_stride(*stride)
        carry = stride[1]
    L.set_params(inp["P"])
    T.set_params(inp["Pt"])
    L.set_text(text)
    L.set_cursors(lstm_hip.initial_cursors(text.size, S, B))
    L.set_state(carry, inp["h0"], inp["c0"])
    T.set_state(carry, inp["ht0"], inp["ct0"])
    if teacher:
        L.set_soft_targets(T, *setting)
    return L, T, inp, text, carry


def _windows_of_the_slide(case, stride, count):
    """the windows the loop's slide makes: a plain handle trained at learning rate 0 (indices do not depend on the model)"""
    L, T, _, _, _ = _loop_start(case, stride, teacher=False)
    out = []
    for _ in range(count):
        L.train_windows(1, 0.0)
        out.append(L.get_window())
    _close(L, T)
    return out


@pytest.mark.parametrize("case,stride", [(LOOP_CASES[0], None), (LOOP_CASES[0], "half"), (LOOP_CASES[1], None), (LOOP_CASES[2], None)],
                         ids=lambda v: sr.case_id(v) if isinstance(v, tuple) else str(v))
def test_device_loop_against_windows_carried_by_hand(case, stride, oracle32, oracle64):
    """train_windows(5) against the same five windows run one at a time in lock-step with the reference, both handles carried
    by hand; then chunks of 3 + 2 and a second run, bit for bit"""
    import lstm_hip
    (N, S, B, flags), (Nt, _) = case
    stride = (S // 2, S // 2 - 1) if stride == "half" else None
    orc = _oracle(case, oracle32, oracle64)
    _, loss_tol, _ = sr.tolerances(case)
    wins = _windows_of_the_slide(case, stride, 5)

    def run(chunks):
        L, T, inp, _, carry = _loop_start(case, stride)
        losses, kls = [], []
        for n in chunks:
            losses.append(L.train_windows(n, LR))
            kls.append(L.teacher_kl())
            assert kls[-1].shape == (n,)
        out = dict(losses=np.concatenate(losses), kls=np.concatenate(kls), P=L.get_params(), mem=L.get_params(lstm_hip.P_MEM),
                   Pt=T.get_params(), window=L.get_window(), inp=inp, carry=carry)
        _close(L, T)
        return out

    one = run((5,))
    inp, carry = one["inp"], one["carry"]
    assert one["Pt"].tobytes() == inp["Pt"].tobytes()                  # the teacher's parameters are only read
    assert all((a == b).all() for a, b in zip(one["window"], wins[-1]))
    # the same five windows one at a time: each handle's column carry_col moved to its column 0 by hand, the window set by
    # hand, and every window checked against the reference from the parameters and the states it started with
    _, _, grad_tol = sr.tolerances(case)
    L, T, _, _, _ = _loop_start(case, stride)
    losses, kls = np.zeros(5), np.zeros(5)
    for k, (xi, ti) in enumerate(wins):
        L.set_window(xi, ti)
        L.set_state(0, *L.get_state(carry))
        T.set_state(0, *T.get_state(carry))
        P, hc, ht = L.get_params(), L.get_state(0), T.get_state(0)
        L.forward()
        losses[k], kls[k] = L.loss(), L.teacher_kl()[0]
        L.backward()
        want = sr.window(orc, case, inp, LOOP_SETTING, P=P, xi=xi, ti=ti, h0=hc[0], c0=hc[1], ht0=ht[0], ct0=ht[1])
        fig = (abs(losses[k] - want["fw"]["loss_bits"]), abs(kls[k] - want["kl"]), max(gu.grads_report(L.get_grads(), want["grads"], N).values()))
        print(f"{sr.case_id(case)} window {k}: loss {losses[k]:.6f} (off by {fig[0]:.3g}), kl {kls[k]:.6f} (off by {fig[1]:.3g}), "
              f"gradients {fig[2]:.3g}")
        assert max(fig[:2]) <= loss_tol * (S - 1) and fig[2] <= grad_tol, (k, fig)
        L.adagrad(LR)
    by_hand = dict(losses=losses, kls=kls, P=L.get_params(), mem=L.get_params(lstm_hip.P_MEM))
    _close(L, T)
    for key, val in by_hand.items():   # the loop makes the single windows' launches on the same data (tests/handle_replay.py, op W)
        assert val.tobytes() == one[key].tobytes(), key
    two, again = run((3, 2)), run((5,))
    for other in (two, again):
        for key in ("losses", "kls", "P", "mem"):
            assert other[key].tobytes() == one[key].tobytes(), key


def test_off_is_off():
    """(1, 1, 0) without a teacher, and a teacher set and cleared again: the bytes of a handle that never made the call, and
    no launch of the new kernel"""
    import lstm_hip
    case = sr.CASES[1]

    def run(prepare):
        L, T, _, _, _ = _loop_start(case, teacher=False)
        prepare(L, T)
        L.set_profiling(True)
        losses = L.train_windows(5, LR)
        stats = {name: v[0] for name, v in L.kernel_stats().items()}
        out = (losses.tobytes(), L.get_params().tobytes(), L.get_params(lstm_hip.P_MEM).tobytes(), stats)
        assert L.soft_targets() == (None, 1.0, 1.0, 0.0)
        _close(L, T)
        return out

    def cleared(L, T):
        L.set_soft_targets(T, 0.5, 2.0, 0.1)
        L.set_soft_targets()

    never = run(lambda L, T: None)
    assert never[3]["softmax_soft"] == 0 and never[3]["softmax_loss_dy"] == 5
    for prepare in (lambda L, T: L.set_soft_targets(None, 1.0, 1.0, 0.0), cleared):
        assert run(prepare) == never

    def smoothed(L, T):
        L.set_soft_targets(smoothing=0.1)
    L, T, _, _, _ = _loop_start(case, teacher=False)
    smoothed(L, T)
    L.set_profiling(True)
    L.train_windows(2, LR)
    stats = {name: v[0] for name, v in L.kernel_stats().items()}
    assert stats["softmax_soft"] == 2 and stats["softmax_loss_dy"] == 0
    _close(L, T)


def test_the_teacher_is_only_borrowed():
    import lstm_hip
    case = sr.CASES[1]
    L, T, inp, _, _ = _loop_start(case)
    lib = L.lib
    L.train_windows(3, LR)
    assert T.get_params().tobytes() == inp["Pt"].tobytes()
    assert lib.lstm_hip_backward(T._h) == lstm_hip.ESTATE
    assert lib.lstm_hip_last_error().decode() == "backward: this handle's last forward pass was a teacher's, not a training forward"
    assert lib.lstm_hip_destroy(T._h) == lstm_hip.ESTATE
    assert lib.lstm_hip_last_error().decode() == ("destroy: 1 student handle(s) hold this handle as their teacher "
                                                  "(lstm_hip_set_soft_targets); clear or destroy them first")
    # slide_state and set_state on the student never touch the teacher
    before = [T.get_state(t) for t in range(T.S)]
    L.slide_state()
    L.set_state(0, inp["h0"], inp["c0"])
    after = [T.get_state(t) for t in range(T.S)]
    assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() for a, b in zip(before, after))
    # the teacher still works as a handle of its own
    T.set_window(inp["xi"], inp["ti"])
    T.forward()
    assert np.isfinite(T.loss())
    T.backward()
    L.set_soft_targets()
    T.close()                                      # released
    assert not T._h
    L.close()


def test_inference_between_windows_reads_the_student_alone():
    """eval_bits and generate on a student between distilled windows: what a handle without a teacher returns on the same
    parameters; and the loop goes on as if they had not been called"""
    import lstm_hip
    case = sr.CASES[1]
    (N, S, B, _), _ = case
    text = gu.text_bytes(300, 5)
    u = np.random.RandomState(3).random_sample((6, 4))

    def infer(H):
        out = H.generate(prompts=[b"ab", b"c", b"", b"defg"], count=6, u=u)
        return H.eval_bits(text), out[0].tobytes(), out[2].tobytes()

    L, T, _, _, _ = _loop_start(case)
    la = L.train_windows(2, LR)
    got = infer(L)
    twin = lstm_hip.Lstm(N, S, B)
    twin.set_params(L.get_params())
    assert infer(twin) == got
    lb = L.train_windows(2, LR)
    L2, T2, _, _, _ = _loop_start(case)
    assert L2.train_windows(4, LR).tobytes() == np.concatenate([la, lb]).tobytes()
    assert L2.get_params().tobytes() == L.get_params().tobytes()
    _close(L, T, L2, T2, twin)


def test_window_with_clipping_adam_and_weight_drop(oracle64):
    """one window with everything on: the gradient is the reference's on the masked matrix (the published mask), the recorded
    norm is the gradient's, and the step is Adam's rule on the clipped gradient"""
    import lstm_hip
    from test_optimizer_adam import B1, B2, EPS, _check_rule, _scalars
    case = sr.CASES[1]
    (N, S, B, _), _ = case
    setting, rate, seed, t0, lr = (0.5, 2.0, 0.1), 0.25, 11, 3, 2e-3
    inp = sr.case_inputs(case)
    keep = lstm_hip.weight_drop_mask(N, rate, seed, t0)
    scale = np.float32(1.0 / (1.0 - rate))
    Pe = inp["P"].copy()
    Ue = gu.split_params(Pe, N)["U"]                   # a view of Pe
    Ue[...] = np.where(keep, Ue * scale, np.float32(0))
    want = sr.window(oracle64, case, inp, setting, P=Pe)
    dref = np.array(want["grads"])
    dU = gu.split_params(dref, N)["U"]
    dU[...] = np.where(keep, dU * float(scale), 0.0)
    L, T = _pair(case)
    try:
        T.set_params(inp["Pt"])
        L.set_params(inp["P"])
        L.set_optimizer(lstm_hip.OPT_ADAM, B1, B2, EPS, 0.01)
        L.set_weight_drop(rate, seed, t0)
        L.set_window(inp["xi"], inp["ti"])
        L.set_state(0, inp["h0"], inp["c0"])
        T.set_state(0, inp["ht0"], inp["ct0"])
        L.set_soft_targets(T, *setting)
        L.forward()
        assert abs(L.loss() - want["fw"]["loss_bits"]) <= 2e-5 * (S - 1)
        assert abs(L.teacher_kl()[0] - want["kl"]) <= 2e-5 * (S - 1)
        L.backward()
        d = L.get_grads()
        rep = gu.grads_report(d, dref, N)
        assert max(rep.values()) <= 2e-4, rep
        norm = np.sqrt(np.sum(d.astype(np.float64) ** 2))
        L.set_grad_clip(norm / 2)
        m0, v0 = L.get_params(lstm_hip.P_MEM), L.get_params(lstm_hip.P_ADAM_V)
        L.adagrad(lr)
        rec = L.grad_norms()[0]
        assert abs(rec - norm) <= 1e-9 * norm, (rec, norm)
        coef = np.float32(norm / 2 / (rec + 1e-6))
        got = (L.get_params(), L.get_params(lstm_hip.P_MEM), L.get_params(lstm_hip.P_ADAM_V))
        _check_rule(got, inp["P"], d * coef, m0, v0, _scalars(lr, 1, 0.01))
        assert L.weight_drop() == (rate, seed, t0 + 1)
    finally:
        _close(L, T)


def test_refusals():
    """every refusal by its return code and its whole message; the handle stays usable and nothing is launched"""
    import lstm_hip
    N, S, B = 32, 4, 2
    E, ST = lstm_hip.EINVAL, lstm_hip.ESTATE
    L, T, T2, Tb, Ts = (lstm_hip.Lstm(n, s, b) for n, s, b in ((N, S, B), (48, S, B), (16, S, B), (N, S, B + 1), (N, S + 1, B)))
    P = gu.random_case(N, S, B, seed=5)[0]
    L.set_params(P)
    L.set_profiling(True)
    stats = L.kernel_stats()
    lib = L.lib

    def refused(rc, code, msg):
        assert rc == code, (rc, lib.lstm_hip_last_error().decode())
        assert lib.lstm_hip_last_error().decode() == msg

    def opt(alpha=1.0, tau=1.0, eps=0.0, size=None):
        return lstm_hip._SoftTargets(C.sizeof(lstm_hip._SoftTargets) if size is None else size, alpha, tau, eps)

    def set_(h, teacher, o):
        return lib.lstm_hip_set_soft_targets(h._h, teacher._h if teacher is not None else None, C.byref(o) if o is not None else None)

    nan, inf = float("nan"), float("inf")
    refused(set_(L, T, None), E, "set_soft_targets: a teacher needs options (opt is NULL)")
    refused(set_(L, T, opt(size=24)), E, "set_soft_targets: opt->size is 24, not sizeof(lstm_hip_soft_targets) = 32")
    for a in (-0.1, 1.5, nan):
        refused(set_(L, T, opt(alpha=a)), E, f"set_soft_targets: alpha must lie in [0, 1] (got {a:g})")
    for tau in (0.0, -1.0, inf, nan):
        refused(set_(L, T, opt(0.5, tau)), E, f"set_soft_targets: temperature must be finite and > 0 (got {tau:g})")
    for eps in (-0.1, 1.0, nan):
        refused(set_(L, T, opt(0.5, 1.0, eps)), E, f"set_soft_targets: smoothing must lie in [0, 1) (got {eps:g})")
    refused(set_(L, None, opt(0.5)), E, "set_soft_targets: without a teacher alpha and temperature must be 1 (got 0.5, 1)")
    refused(set_(L, None, opt(1.0, 2.0)), E, "set_soft_targets: without a teacher alpha and temperature must be 1 (got 1, 2)")
    refused(set_(L, L, opt(0.5)), E, "set_soft_targets: a handle cannot be its own teacher")
    refused(set_(L, Tb, opt(0.5)), E, f"set_soft_targets: the teacher's (S, B, device) = ({S}, {B + 1}, 0) differ from the student's ({S}, {B}, 0)")
    refused(set_(L, Ts, opt(0.5)), E, f"set_soft_targets: the teacher's (S, B, device) = ({S + 1}, {B}, 0) differ from the student's ({S}, {B}, 0)")
    assert set_(T, T2, opt(0.5)) == 0
    refused(set_(L, T, opt(0.5)), E, "set_soft_targets: the teacher has a teacher of its own")
    refused(set_(T2, L, opt(0.5)), E, "set_soft_targets: this handle is itself held as a teacher")
    assert set_(T, None, None) == 0
    kl = np.zeros(4)
    refused(lib.lstm_hip_get_teacher_kl(L._h, lstm_hip._ptr(kl, C.c_double), C.c_int64(1)), ST,
            "get_teacher_kl: this handle has no teacher (lstm_hip_set_soft_targets)")
    assert L.soft_targets() == (None, 1.0, 1.0, 0.0)                      # a refused set sets nothing
    assert L.kernel_stats() == stats
    # with soft targets on
    assert set_(L, T, opt(0.5, 2.0, 0.1)) == 0 and L.soft_targets()[1:] == (0.5, 2.0, 0.1)
    refused(lib.lstm_hip_get_teacher_kl(L._h, lstm_hip._ptr(kl, C.c_double), C.c_int64(1)), ST,
            "get_teacher_kl: no forward / train_windows call since the teacher was set")
    refused(lib.lstm_hip_backward(L._h), ST, "backward called before forward")
    L.set_train_texts([b"abcdef"])
    refused(lib.lstm_hip_train_text_windows(L._h, C.c_int64(1), C.c_double(0.1), None, None), ST,
            "train_text_windows: soft targets are on (lstm_hip_set_soft_targets); the text windows train on hard targets")
    text, off = np.frombuffer(b"abcdefgh", np.uint8), np.array([0, 4, 8], np.uint64)
    code, code_off, bits = np.zeros(256, np.uint8), np.zeros(B + 1, np.uint64), np.zeros(B)
    refused(lib.lstm_hip_encode_adaptive(L._h, lstm_hip._ptr(text, C.c_uint8), lstm_hip._ptr(off, C.c_uint64), C.c_double(0.1),
                                         lstm_hip._ptr(code, C.c_uint8), C.c_uint64(code.size), lstm_hip._ptr(code_off, C.c_uint64),
                                         lstm_hip._ptr(bits, C.c_double), None, None), ST,
            "encode_adaptive: soft targets are on (lstm_hip_set_soft_targets); the adaptive coders train on hard targets")
    out = np.zeros(8, np.uint8)
    refused(lib.lstm_hip_decode_adaptive(L._h, lstm_hip._ptr(code, C.c_uint8), lstm_hip._ptr(code_off, C.c_uint64),
                                         lstm_hip._ptr(off, C.c_uint64), C.c_double(0.1), lstm_hip._ptr(out, C.c_uint8)), ST,
            "decode_adaptive: soft targets are on (lstm_hip_set_soft_targets); the adaptive coders train on hard targets")
    T.set_weight_drop(0.5, 1, 0)
    msg = "the teacher has weight drop on (lstm_hip_set_weight_drop); a teacher runs its unmasked parameters"
    refused(lib.lstm_hip_forward(L._h), ST, "forward: " + msg)
    L.set_text(gu.text_bytes(64, 1))
    L.set_cursors(lstm_hip.initial_cursors(64, S, B))
    refused(lib.lstm_hip_train_windows(L._h, C.c_int64(1), C.c_double(0.1), None, None), ST, "train_windows: " + msg)
    T.set_weight_drop(0.0)
    refused(lib.lstm_hip_get_teacher_kl(L._h, None, C.c_int64(1)), ST,
            "get_teacher_kl: no forward / train_windows call since the teacher was set")
    assert L.kernel_stats() == stats and L.optimizer_steps() == 0        # nothing ran on the handle
    refused(lib.lstm_hip_comm_init(L._h, (C.c_uint8 * lstm_hip.UNIQUE_ID_BYTES)(), 1, 0), ST,
            "comm_init: soft targets are on (lstm_hip_set_soft_targets); they run on one device")
    refused(lib.lstm_hip_destroy(T._h), ST, "destroy: 1 student handle(s) hold this handle as their teacher "
                                            "(lstm_hip_set_soft_targets); clear or destroy them first")
    # the handle stays usable
    L.set_window(*gu.random_case(N, S, B, seed=5)[1:3])
    L.forward()
    assert L.loss() > 0 and L.teacher_kl().shape == (1,)
    refused(lib.lstm_hip_get_teacher_kl(L._h, lstm_hip._ptr(kl, C.c_double), C.c_int64(2)), E,
            "get_teacher_kl: n = 2 outside [0, 1] or null pointer")
    L.close()                                                            # destroying the student releases the teacher
    assert lib.lstm_hip_destroy(T._h) == 0
    T._h = C.c_void_p()
    _close(T2, Tb, Ts)


def test_a_communicator_on_the_student_is_refused():
    import lstm_hip
    L, T = lstm_hip.Lstm(32, 4, 2), lstm_hip.Lstm(16, 4, 2)
    try:
        L.comm_init(lstm_hip.comm_unique_id(), 1, 0)   # (one rank, as test_rccl_path_with_a_single_rank_communicator)
        o = lstm_hip._SoftTargets(C.sizeof(lstm_hip._SoftTargets), 0.5, 1.0, 0.0)
        assert L.lib.lstm_hip_set_soft_targets(L._h, T._h, C.byref(o)) == lstm_hip.ESTATE
        assert L.lib.lstm_hip_last_error().decode() == "set_soft_targets: this handle has a communicator; soft targets run on one device"
        assert L.soft_targets() == (None, 1.0, 1.0, 0.0)
    finally:
        _close(L, T)
