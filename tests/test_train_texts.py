"""-m gpu: lstm_hip_train_text_windows -- training on separate texts, each from its zero state (include/lstm_hip.h; DESIGN.md
section 3.18).

One window at a time in lock-step with the reference of tests/text_train_ref.py (the unchanged oracle, lane by lane, by
truncation) on every engine plan of its table and with fewer streams than lanes, as many, and 3B + 1; then the properties of
the call: chunking, determinism, the update counters, the streams' bits against the losses, the refusals, and the handle it
leaves.  Tolerances and comparison rules are those of tests/test_hip_parity.py::test_window_matches_oracle (bf16: of its
test_bf16_recurrence_matches_bf16_oracle).  The reference's own checks and its mutant are in tests/test_train_texts_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import gpu_util as gu
import handle_replay as hr
import handle_sequence_cases as hsc
import text_train_ref as tr

pytestmark = pytest.mark.gpu
LR = 0.1


def _flags(names):
    import lstm_hip
    flags = 0
    for f in names:
        flags |= getattr(lstm_hip, f)
    return flags


def _handle(case, P=None, seed=None):
    import lstm_hip
    N, S, B, flags = case
    L = lstm_hip.Lstm(N, S, B, flags=_flags(flags))
    if P is None:
        P = gu.random_case(N, S, B, seed=N + S + B if seed is None else seed, scale=0.05 if "BF16_RECURRENCE" in flags else 0.08)[0]
    L.set_params(P)
    return L


def _columns(L):
    S = L.S
    hs, cs = zip(*(L.get_state(t) for t in range(S)))
    gs, ps = zip(*(L.get_activations(t) for t in range(1, S)))
    return np.stack(hs), np.stack(cs), np.stack(gs), np.stack(ps)


@pytest.mark.parametrize("case,kind", tr.all_cases(), ids=[tr.case_id(c, k) for c, k in tr.all_cases()])
def test_windows_in_lock_step_with_the_reference(case, kind, oracle32, oracle64):
    import lstm_hip
    N, S, B, flags = case
    bf16 = "BF16_RECURRENCE" in flags
    orc = oracle32 if bf16 else oracle64
    act_tol, loss_tol, grad_tol = tr.tolerances(case)
    txts = tr.case_texts(case, kind)
    wins = tr.windows_ref(S, B, txts)
    L = _handle(case)
    worst = dict(act=0.0, loss=0.0, grad=0.0, step=0.0)
    if bf16:
        orc.set_bf16_recurrence(True), orc.set_bf16_products(True)
    try:
        assert L.set_train_texts(txts) == len(wins) and L.train_texts_progress() == (len(wins), 0)
        bits = np.zeros(len(txts))
        for k, win in enumerate(wins):
            P, mem = L.get_params(), L.get_params(lstm_hip.P_MEM)
            carry_h, carry_c = L.get_state(S - 1)
            loss = L.train_text_windows(1, LR)[0]
            assert L.train_texts_progress() == (len(wins), k + 1)
            want = tr.window_ref(orc, N, P, win, carry_h, carry_c)
            xi, ti = L.get_window()
            assert (xi == win["xi"]).all() and (ti == win["ti"]).all(), k       # -1 on every row without a step
            h, c, g, p = _columns(L)
            fresh = win["fresh"]
            assert not h[0][fresh].any() and not c[0][fresh].any(), k          # a text's start, an idle lane: the zero state
            assert h[0][~fresh].tobytes() == carry_h[~fresh].tobytes() and c[0][~fresh].tobytes() == carry_c[~fresh].tobytes(), k
            for t in range(1, S):
                m = want["mask"][t]
                if not m.any():
                    continue
                for name, got in (("h", h[t]), ("c", c[t]), ("g", g[t - 1]), ("probs", p[t - 1])):
                    err = gu.max_rel(got[m], want[name][t][m])
                    worst["act"] = max(worst["act"], err)
                    assert err <= act_tol, (k, name, t, err)
            worst["loss"] = max(worst["loss"], abs(loss - want["loss"]))
            assert abs(loss - want["loss"]) <= loss_tol * (S - 1), (k, loss, want["loss"])
            grads = L.get_grads()
            rep = gu.grads_report(grads, want["grads"], N)
            worst["grad"] = max(worst["grad"], max(rep.values()))
            assert max(rep.values()) <= grad_tol, (k, rep)
            # the update, from the parameters and the memory the window started with (test_window_matches_oracle's mask and bound)
            # (not under bf16: its test in tests/test_hip_parity.py sets no bound for the step, and a gradient within 1e-2 of
            # the tensor's scale bounds nothing at an entry of 1e-3 of that scale)
            if not bf16:
                Pref, mref = tr.adagrad_ref(orc, P, want["grads"], mem, LR)
                dref = want["grads"]
                mask = np.abs(dref) > 1e-3 * np.abs(dref).max()
                step = np.abs(L.get_params()[mask] - Pref[mask]).max()
                worst["step"] = max(worst["step"], float(step))
                assert step <= 2e-4 * LR + 1e-6, (k, step)
                np.testing.assert_allclose(L.get_params(lstm_hip.P_MEM), mref, rtol=1e-3, atol=1e-3 * float(mref.max()))
            for lane in range(B):
                if win["stream"][lane] >= 0:
                    bits[win["stream"][lane]] += want["surprisal"][:, lane].sum()
        got_bits = L.train_texts_bits()
        steps = np.array([max(len(t) - 1, 0) for t in txts])
        assert np.abs(got_bits - bits).max() <= loss_tol * max(steps.max(), 1), (got_bits, bits)
        assert not got_bits[steps == 0].any()
    finally:
        if bf16:
            orc.set_bf16_recurrence(False), orc.set_bf16_products(False)
        L.close()
    print(f"{tr.case_id(case, kind)}: {len(wins)} windows; activations {worst['act']:.3g}, loss {worst['loss']:.3g}, "
          f"gradients {worst['grad']:.3g}, step {worst['step']:.3g}")


def _run(case, txts, chunks, setup=None):
    """train the whole plan in calls of `chunks` windows; returns every result a cut could show in"""
    import lstm_hip
    L = _handle(case)
    try:
        if setup:
            setup(L)
        n = L.set_train_texts(txts)
        assert sum(chunks) == n, (chunks, n)
        losses = np.concatenate([L.train_text_windows(k, 0.05) for k in chunks])
        out = dict(losses=losses, bits=L.train_texts_bits(), params=L.get_params(), mem=L.get_params(lstm_hip.P_MEM),
                   steps=np.array([L.optimizer_steps()]))
        hs, cs = zip(*(L.get_state(t) for t in range(L.S)))
        out["h"], out["c"] = np.stack(hs), np.stack(cs)
        out["xi"], out["ti"] = L.get_window()
        if setup:
            out["adam_v"] = L.get_params(lstm_hip.P_ADAM_V)
            out["avg"] = L.get_average()
            out["norms"] = L.grad_norms(chunks[-1])
        return out
    finally:
        L.close()


def _everything_on(L):
    import lstm_hip
    L.set_optimizer(lstm_hip.OPT_ADAM)
    L.set_grad_clip(0.5)
    L.set_averaging(lstm_hip.AVG_EMA, decay=0.9)
    L.set_weight_drop(0.25, seed=3)


PROPERTY_CASES = [tr.CASES[1], tr.CASES[3], tr.CASES[6], tr.CASES[7]]


@pytest.mark.parametrize("case", PROPERTY_CASES, ids=tr.case_id)
@pytest.mark.parametrize("setup", [None, _everything_on], ids=["adagrad", "adam-clip-ema-weightdrop"])
def test_chunking_and_determinism(case, setup):
    """train_text_windows(k) once against k calls of 1 and against another cut: the same bytes; and a second handle too"""
    txts = tr.case_texts(case, "queue")
    n = len(tr.windows_ref(case[1], case[2], txts))
    assert n >= 3
    whole = _run(case, txts, [n], setup)
    ones = _run(case, txts, [1] * n, setup)
    cut = _run(case, txts, [2, 0, n - 2], setup)
    again = _run(case, txts, [n], setup)
    assert np.isfinite(whole["losses"]).all() and (whole["losses"] > 0).all()
    for name, other in (("calls of one window", ones), ("calls of 2, 0 and the rest", cut)):
        hr.assert_same({k: v for k, v in whole.items() if k != "norms"}, other, f"one call against {name}")
    hr.assert_same(whole, again, "a second handle with the same texts")


def test_update_counters_advance_once_per_window():
    import lstm_hip
    case = tr.CASES[1]
    txts = tr.case_texts(case, "queue")
    L = _handle(case)
    try:
        _everything_on(L)
        n = L.set_train_texts(txts)
        before = L.get_params()
        L.train_text_windows(2, 0.01)
        assert L.optimizer_steps() == 2 and L.averaging_counts() == (2, 2) and L.weight_drop()[2] == 2
        norms = L.grad_norms()
        assert norms.shape == (2,) and (norms > 0).all() and np.isfinite(norms).all()
        L.train_text_windows(n - 2, 0.01)
        assert L.optimizer_steps() == n and L.averaging_counts() == (n, n) and L.weight_drop()[2] == n
        assert L.grad_norms().shape == (n - 2,)
        assert L.train_texts_progress() == (n, n)
        assert (L.get_params() != before).any()
        L.set_profiling(True)          # a profiled pass names the three launches
        L.set_train_texts(txts)
        L.reset_kernel_stats()
        L.train_text_windows(3, 0.01)
        st = L.kernel_stats()
        assert st["text_window"][0] == 3 and st["text_fold"][0] == 3 and st["softmax_loss_dy_text"][0] == 3
        assert st["softmax_loss_dy"][0] == 0 and st["slide"][0] == 0
    finally:
        L.close()


@pytest.mark.parametrize("case", [tr.CASES[1], tr.CASES[4]], ids=tr.case_id)
def test_bits_against_losses(case):
    """bits.sum() / B is losses.sum() up to the float sums inside a loss: per row a float sum of B surprisals and a float
    division, so each of the (S - 1) * windows row sums is off by at most (B + 1) roundings of a partial sum no larger than
    the row's total."""
    N, S, B, _ = case
    txts = tr.case_texts(case, "queue")
    L = _handle(case)
    try:
        n = L.set_train_texts(txts)
        losses = L.train_text_windows(n, 0.05)
        bits = L.train_texts_bits()
    finally:
        L.close()
    eps = 2.0 ** -24
    bound = (B + 1) * eps * losses.sum() + 1e-12          # sum over rows of (B + 1) eps x (row total / B)
    assert abs(bits.sum() / B - losses.sum()) <= bound, (bits.sum() / B, losses.sum(), bound)
    assert (bits[[len(t) >= 2 for t in txts]] > 0).all()


@pytest.mark.parametrize("shape", [s for s in hsc.SHAPES if s.forms in hsc.INFERENCE_ROWS], ids=hsc.shape_id)
def test_the_handle_stays_usable(shape):
    """after a call, lstm_hip_train_windows on the same handle gives the bytes a fresh handle loaded with the same observable
    state gives; text, cursors, stride and loss mode are as they were"""
    text = np.frombuffer(bytes(gu.text_bytes(4000, 51)), np.uint8)
    txts = tr.texts(tr.lengths(shape.S, shape.B + 3, 77), 78)
    A, twin = hr.start(shape, text), None
    try:
        A.train_windows(2, hr.LR)
        cursors = A.get_cursors()
        n = A.set_train_texts(txts)
        A.train_text_windows(n - 1, hr.LR)
        assert (A.get_cursors() == cursors).all()
        snap = hr.snapshot(A, text)
        twin = hr.restore(shape, snap)
        la, lt = A.train_windows(3, hr.LR), twin.train_windows(3, hr.LR)
        assert la.tobytes() == lt.tobytes()
        hr.assert_same(hr.snapshot(A, text), hr.snapshot(twin, text), "train_windows after train_text_windows against a fresh twin")
        A.train_text_windows(1, hr.LR)     # and the plan goes on where it stood
        assert A.train_texts_progress() == (n, n)
    finally:
        A.close()
        if twin is not None:
            twin.close()


def test_refusals_launch_nothing():
    """every refusal's return code and whole text; the handle stays usable"""
    import lstm_hip
    N, S, B = 32, 4, 2
    L = lstm_hip.Lstm(N, S, B)
    L.set_params(gu.random_case(N, S, B, seed=71)[0])
    L.set_profiling(True)
    stats = L.kernel_stats()
    lib, p = L.lib, lstm_hip._ptr
    text = np.arange(10, dtype=np.uint8)
    off = np.array([0, 4, 10], np.uint64)
    losses = np.zeros(8)

    def refused(rc, code, msg):
        assert rc == code, (rc, lib.lstm_hip_last_error().decode())
        assert lib.lstm_hip_last_error().decode() == msg

    def set_texts(streams=2, text=text, off=off):
        return lib.lstm_hip_set_train_texts(L._h, C.c_int32(streams), p(text, C.c_uint8) if text is not None else None,
                                            p(off, C.c_uint64) if off is not None else None)

    def train(count=1, lr=0.1):
        return lib.lstm_hip_train_text_windows(L._h, C.c_int64(count), C.c_double(lr), p(losses, C.c_double), None)

    E, ST = lstm_hip.EINVAL, lstm_hip.ESTATE
    w, nx = C.c_int64(), C.c_int64()
    refused(train(), ST, "train_text_windows before set_train_texts")
    refused(lib.lstm_hip_get_train_texts(L._h, C.byref(w), C.byref(nx)), ST, "get_train_texts before set_train_texts")
    refused(lib.lstm_hip_get_train_texts_bits(L._h, p(losses, C.c_double)), ST, "get_train_texts_bits before set_train_texts")
    refused(set_texts(streams=0), E, "set_train_texts: streams must be >= 1 (got 0)")
    refused(set_texts(streams=-1), E, "set_train_texts: streams must be >= 1 (got -1)")
    refused(set_texts(off=None), E, "set_train_texts: null text_off")
    refused(set_texts(off=np.array([1, 4, 10], np.uint64)), E, "set_train_texts: text_off[0] must be 0 (got 1)")
    refused(set_texts(off=np.array([0, 11, 10], np.uint64)), E, "set_train_texts: text_off decreases at stream 1 (10 < 11)")
    refused(set_texts(text=None), E, "set_train_texts: null text with 10 bytes to read")
    refused(train(), ST, "train_text_windows before set_train_texts")     # a refused set sets nothing
    assert set_texts() == 0                                               # 3 and 5 steps on 3 rows: 1 and 2 windows
    assert lib.lstm_hip_get_train_texts(L._h, C.byref(w), C.byref(nx)) == 0 and (w.value, nx.value) == (2, 0)
    refused(train(count=-1), E, "train_text_windows: count -1 outside [0, 2] (the plan has 2 windows, the next is 0)")
    refused(train(count=3), E, "train_text_windows: count 3 outside [0, 2] (the plan has 2 windows, the next is 0)")
    refused(train(lr=-0.5), E, "train_text_windows: learning_rate must be finite and >= 0 (got -0.5)")
    refused(train(lr=float("nan")), E, "train_text_windows: learning_rate must be finite and >= 0 (got nan)")
    refused(train(lr=float("inf")), E, "train_text_windows: learning_rate must be finite and >= 0 (got inf)")
    L.set_loss_mode(lstm_hip.LOSS_LAST_STEP_NATS)
    refused(train(), ST, "train_text_windows: the loss mode is 1; the text windows report LSTM_HIP_LOSS_ALL_STEPS_BITS only")
    L.set_loss_mode(lstm_hip.LOSS_ALL_STEPS_BITS)
    refused(lib.lstm_hip_get_train_texts_bits(L._h, None), E, "get_train_texts_bits: null pointer")
    assert L.kernel_stats() == stats and L.optimizer_steps() == 0        # nothing ran on the handle
    assert train(count=0) == 0 and train(count=1) == 0 and losses[0] > 0
    refused(train(count=2), E, "train_text_windows: count 2 outside [0, 1] (the plan has 2 windows, the next is 1)")
    assert set_texts(streams=0, text=None, off=None) == 0                 # dropped
    refused(train(), ST, "train_text_windows before set_train_texts")
    assert set_texts(text=None, off=np.zeros(3, np.uint64)) == 0          # no bytes to read: no text needed, no window
    assert lib.lstm_hip_get_train_texts(L._h, C.byref(w), C.byref(nx)) == 0 and (w.value, nx.value) == (0, 0)
    L.close()


def test_a_communicator_is_refused():
    import lstm_hip
    L = lstm_hip.Lstm(32, 4, 2)
    try:
        L.comm_init(lstm_hip.comm_unique_id(), 1, 0)   # (one rank, as test_rccl_path_with_a_single_rank_communicator)
        L.set_train_texts([b"abcdef"])
        rc = L.lib.lstm_hip_train_text_windows(L._h, C.c_int64(1), C.c_double(0.1), None, None)
        assert rc == lstm_hip.ESTATE
        assert L.lib.lstm_hip_last_error().decode() == "train_text_windows: a handle with a communicator cannot train on separate texts"
        assert L.optimizer_steps() == 0
    finally:
        L.close()


def test_program_records(tmp_path):
    """lstm --records: the records of --data, cut after the delimiter, in a seeded order; the epoch line carries the
    prequential bits/char over the bytes that were scored; --save, --load and --test-streams go on working"""
    import os
    import re
    import subprocess
    lstm = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eigen-lstm_amd", "lstm")
    rs = np.random.RandomState(21)
    lines = [bytes(rs.randint(97, 123, size=rs.randint(0, 30)).astype(np.uint8)) + b"\n" for _ in range(120)]
    corpus = b"".join(lines) + b"tail without its delimiter"
    f = tmp_path / "records.txt"
    f.write_bytes(corpus)
    S, B = 8, 4
    lens = [len(x) for x in lines] + [26]
    scored = sum(max(n - 1, 0) for n in lens)
    ck = tmp_path / "ck"
    args = [lstm, str(f), "32", str(S), str(B), "0.05", "--epochs", "2", "--seed", "1", "--sample", "0", "--records", "--quiet",
            "--eval-file", str(f), "--test-streams", "4"]

    def run(extra):
        out = subprocess.run(args + extra, capture_output=True, text=True, errors="replace", timeout=120)
        assert out.returncode == 0, out.stderr
        return out.stdout

    a = run(["--save", str(ck)])
    assert f"Records: {len(lens)}, cut after byte 10" in a
    rows = re.findall(r"records: (\d+) texts in (\d+) windows, ([\d.]+)% of the rows filled, ([\d.]+) prequential bits/char over (\d+) bytes", a)
    assert len(rows) == 2 and all(int(r[0]) == len(lens) and int(r[4]) == scored for r in rows), a
    for r in rows:   # the plan of the shuffled order is not ours to know; its size is bounded by the rows it must hold
        assert scored <= int(r[1]) * (S - 1) * B and abs(float(r[2]) - 100.0 * scored / (int(r[1]) * (S - 1) * B)) < 0.06
    first, second = float(rows[0][3]), float(rows[1][3])
    assert 4.0 < second < first < 8.5, rows          # 26 letters and a newline from a flat start of 8 bits
    tests = [float(v) for v in re.findall(r"Test error: ([\d.]+) bits/char", a)]
    assert len(tests) == 2 and max(tests) < first     # the trained model against the average over the epoch that trained it
    pat = r"records: .* prequential bits/char over \d+ bytes|Test error: [\d.]+ bits/char"
    assert re.findall(pat, run([])) == re.findall(pat, a)                                          # seeded: the same run
    assert re.findall(pat, run(["--shuffle-seed", "5"])) != re.findall(pat, a)                     # another order
    c = run(["--load", str(ck), "--epochs", "1", "--windows", "3"])
    m = re.search(r"records: \d+ texts in 3 windows, [\d.]+% of the rows filled, ([\d.]+) prequential", c)
    assert m and float(m.group(1)) < first, c                                                       # resumed from the trained model
    other = run(["--record-delim", "97"])
    assert f"Records: {corpus[:-1].count(b'a') + 1}, cut after byte 97" in other
