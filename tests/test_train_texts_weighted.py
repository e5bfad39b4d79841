"""-m gpu: lstm_hip_set_train_texts_weighted -- a weight per target byte on the text windows: completion-only training,
importance weights (include/lstm_hip.h).

One window at a time in lock-step with the reference of tests/text_weight_ref.py (the unchanged oracle, telescoped over the
truncation lengths) on every engine plan of tests/text_train_ref.py's table, with drawn weights and with completion weights;
then the properties of the call: weight 1 is the unweighted call's bytes, weight 2 doubles the gradient block exactly, a
window of weight 0 updates nothing, a non-finite context poisons nothing, chunking and determinism, replacement, refusals
and the handle it leaves.  Tolerances and comparison rules are those of tests/test_train_texts.py.  The reference's own
checks and its two mutants are in tests/test_train_texts_weighted_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import gpu_util as gu
import handle_replay as hr
import handle_sequence_cases as hsc
import text_train_ref as tr
import text_weight_ref as wr

pytestmark = pytest.mark.gpu
LR = 0.1


def _flags(names):
    import lstm_hip
    flags = 0
    for f in names:
        flags |= getattr(lstm_hip, f)
    return flags


def _handle(case, extra_flags=(), P=None):
    import lstm_hip
    N, S, B, flags = case
    L = lstm_hip.Lstm(N, S, B, flags=_flags(tuple(flags) + tuple(extra_flags)))
    L.set_params(gu.random_case(N, S, B, seed=N + S + B, scale=0.05 if "BF16_RECURRENCE" in flags else 0.08)[0] if P is None else P)
    return L


def _columns(L):
    S = L.S
    hs, cs = zip(*(L.get_state(t) for t in range(S)))
    gs, ps = zip(*(L.get_activations(t) for t in range(1, S)))
    return np.stack(hs), np.stack(cs), np.stack(gs), np.stack(ps)


def _stats(L):
    return {name: v[0] for name, v in L.kernel_stats().items()}


@pytest.mark.parametrize("case,kind,wkind", wr.lock_step_params(), ids=[wr.lock_step_id(p) for p in wr.lock_step_params()])
def test_weighted_windows_in_lock_step_with_the_reference(case, kind, wkind, oracle32, oracle64):
    import lstm_hip
    N, S, B, flags = case
    bf16 = "BF16_RECURRENCE" in flags
    orc = oracle32 if bf16 else oracle64
    act_tol, loss_tol, grad_tol = tr.tolerances(case)
    txts, weights = wr.case_texts_and_weights(case, kind, wkind)
    if wkind == "completion":
        got = lstm_hip.completion_weights(txts, wr.SEP)
        assert all((a == b).all() for a, b in zip(got, weights))
        weights = got
    wins = tr.windows_ref(S, B, txts)
    L = _handle(case)
    worst = dict(act=0.0, loss=0.0, grad=0.0, step=0.0)
    if bf16:
        orc.set_bf16_recurrence(True), orc.set_bf16_products(True)
    try:
        assert L.set_train_texts(txts, weights) == len(wins) and L.train_texts_progress() == (len(wins), 0)
        bits = np.zeros(len(txts))
        for k, win in enumerate(wins):
            P, mem = L.get_params(), L.get_params(lstm_hip.P_MEM)
            carry_h, carry_c = L.get_state(S - 1)
            loss = L.train_text_windows(1, LR)[0]
            assert L.train_texts_progress() == (len(wins), k + 1)
            want = wr.window_ref(orc, N, P, win, wr.window_weights(win, weights), carry_h, carry_c)
            xi, ti = L.get_window()
            assert (xi == win["xi"]).all() and (ti == win["ti"]).all(), k       # a weight-0 byte keeps its input AND its target
            h, c, g, p = _columns(L)
            fresh = win["fresh"]
            assert not h[0][fresh].any() and not c[0][fresh].any(), k
            assert h[0][~fresh].tobytes() == carry_h[~fresh].tobytes() and c[0][~fresh].tobytes() == carry_c[~fresh].tobytes(), k
            for t in range(1, S):
                m = want["mask"][t]
                if not m.any():
                    continue
                for name, got in (("h", h[t]), ("c", c[t]), ("g", g[t - 1]), ("probs", p[t - 1])):   # probs: the plain p
                    err = gu.max_rel(got[m], want[name][t][m])
                    worst["act"] = max(worst["act"], err)
                    assert err <= act_tol, (k, name, t, err)
            worst["loss"] = max(worst["loss"], abs(loss - want["loss"]))
            assert abs(loss - want["loss"]) <= loss_tol * (S - 1), (k, loss, want["loss"])
            grads = L.get_grads()
            if np.abs(want["grads"]).max() == 0.0:      # (a window whose rows all have weight 0)
                assert not grads.any(), k
            else:
                rep = gu.grads_report(grads, want["grads"], N)
                worst["grad"] = max(worst["grad"], max(rep.values()))
                assert max(rep.values()) <= grad_tol, (k, rep)
            if not bf16:    # the update (test_train_texts.py's mask and bound; not under bf16, as there)
                Pref, mref = tr.adagrad_ref(orc, P, want["grads"], mem, LR)
                dref = want["grads"]
                mask = np.abs(dref) > 1e-3 * np.abs(dref).max()
                if mask.any():
                    step = np.abs(L.get_params()[mask] - Pref[mask]).max()
                    worst["step"] = max(worst["step"], float(step))
                    assert step <= 2e-4 * LR + 1e-6, (k, step)
                np.testing.assert_allclose(L.get_params(lstm_hip.P_MEM), mref, rtol=1e-3, atol=1e-3 * max(float(mref.max()), 1e-30))
            for lane in range(B):
                if win["stream"][lane] >= 0:
                    bits[win["stream"][lane]] += want["surprisal"][:, lane].sum()
        got_bits = L.train_texts_bits()
        steps = np.array([max(len(t) - 1, 0) for t in txts])
        assert np.abs(got_bits - bits).max() <= loss_tol * max(steps.max(), 1), (got_bits, bits)
        assert not got_bits[[not w[1:].any() for w in weights]].any()           # nothing learned: exactly 0 bits
    finally:
        if bf16:
            orc.set_bf16_recurrence(False), orc.set_bf16_products(False)
        L.close()
    print(f"{wr.lock_step_id((case, kind, wkind))}: {len(wins)} windows; activations {worst['act']:.3g}, loss {worst['loss']:.3g}, "
          f"gradients {worst['grad']:.3g}, step {worst['step']:.3g}")


def _run(case, txts, weights, chunks, setup=None, profile=False):
    """train the whole plan in calls of `chunks` windows; returns every result a cut could show in"""
    import lstm_hip
    L = _handle(case)
    try:
        if setup:
            setup(L)
        L.set_profiling(profile)
        n = L.set_train_texts(txts, weights)
        assert sum(chunks) == n, (chunks, n)
        losses = np.concatenate([L.train_text_windows(k, 0.05) for k in chunks])
        out = dict(losses=losses, bits=L.train_texts_bits(), params=L.get_params(), mem=L.get_params(lstm_hip.P_MEM),
                   steps=np.array([L.optimizer_steps()]), grads=L.get_grads())
        hs, cs = zip(*(L.get_state(t) for t in range(L.S)))
        out["h"], out["c"] = np.stack(hs), np.stack(cs)
        out["xi"], out["ti"] = L.get_window()
        if setup:
            out["adam_v"] = L.get_params(lstm_hip.P_ADAM_V)
            out["avg"] = L.get_average()
            out["norms"] = L.grad_norms(chunks[-1])
        return out, (_stats(L) if profile else None)
    finally:
        L.close()


def _everything_on(L):
    import lstm_hip
    L.set_optimizer(lstm_hip.OPT_ADAM)
    L.set_grad_clip(0.5)
    L.set_averaging(lstm_hip.AVG_EMA, decay=0.9)
    L.set_weight_drop(0.25, seed=3)


@pytest.mark.parametrize("case", [tr.CASES[1], tr.CASES[7], tr.CASES[8]], ids=tr.case_id)
def test_weight_one_is_the_unweighted_call(case):
    """w == 1.0f everywhere: losses, bits, parameters, memory, states and gradients are the bytes of set_train_texts without
    weights (a multiply by 1 is exact); only the statistics row of the softmax launch tells the two runs apart"""
    txts = tr.case_texts(case, "queue")
    n = len(tr.windows_ref(case[1], case[2], txts))
    ones = [np.ones(len(t), np.float32) for t in txts]
    plain, plain_stats = _run(case, txts, None, [n], profile=True)
    weighted, weighted_stats = _run(case, txts, ones, [n], profile=True)
    scalar, _ = _run(case, txts, [1.0] * len(txts), [n], profile=True)          # (a scalar per text is broadcast)
    hr.assert_same(plain, weighted, "weights of 1.0 against no weights")
    hr.assert_same(weighted, scalar, "a scalar 1.0 per text against arrays of 1.0")
    assert set(plain) == set(weighted) and np.isfinite(plain["losses"]).all() and plain["grads"].any()
    assert plain_stats["softmax_loss_dy_text"] == n and plain_stats["softmax_loss_dy_weighted"] == 0
    assert weighted_stats["softmax_loss_dy_weighted"] == n and weighted_stats["softmax_loss_dy_text"] == 0
    for st in (plain_stats, weighted_stats):
        assert st["softmax_loss_dy"] == 0 and st["text_window"] == n and st["text_fold"] == n


@pytest.mark.parametrize("case", [tr.CASES[1], tr.CASES[6], tr.CASES[5]], ids=tr.case_id)
def test_weight_two_doubles_the_gradient_block_exactly(case):
    """one window, clip off: every step from dy to the gradient block is linear, and a scaling by 2 commutes with every
    rounding (no value here is near the denormals or the overflow), so the block is 2x byte for byte and the loss exactly 2x"""
    txts = tr.case_texts(case, "queue")
    out = {}
    for w in (1.0, 2.0):
        L = _handle(case)
        try:
            L.set_train_texts(txts, [np.full(len(t), w, np.float32) for t in txts])
            out[w] = (L.train_text_windows(1, LR)[0], L.get_grads(), L.train_texts_bits())
        finally:
            L.close()
    (l1, g1, b1), (l2, g2, b2) = out[1.0], out[2.0]
    assert g1.any() and np.isfinite(g1).all() and l1 > 0
    assert (2 * g1).tobytes() == g2.tobytes()
    assert l2 == 2 * l1 and (b2 == 2 * b1).all()


@pytest.mark.parametrize("clip", [0.0, 0.5], ids=["clip-off", "clip-on"])
@pytest.mark.parametrize("case", [tr.CASES[1], tr.CASES[3]], ids=tr.case_id)
def test_a_window_of_weight_zero_updates_nothing(case, clip):
    """all weights 0: the gradient block is all zeros, Adagrad's parameters and memory are the bytes they were, the update
    still ran (optimizer_steps advanced); with clipping on the recorded norm is 0 and the step is not scaled"""
    import lstm_hip
    txts = tr.case_texts(case, "queue")
    L = _handle(case)
    try:
        if clip:
            L.set_grad_clip(clip)
        L.set_train_texts(txts, [0.0] * len(txts))
        P, mem = L.get_params(), L.get_params(lstm_hip.P_MEM)
        losses = L.train_text_windows(2, LR)
        assert (losses == 0.0).all() and not np.signbit(losses).any()
        assert not L.get_grads().any()
        assert L.get_params().tobytes() == P.tobytes() and L.get_params(lstm_hip.P_MEM).tobytes() == mem.tobytes()
        assert L.optimizer_steps() == 2 and L.train_texts_progress()[1] == 2
        assert not L.train_texts_bits().any()
        if clip:
            assert (L.grad_norms() == 0.0).all() and L.grad_norms().shape == (2,)
        _, p = L.get_activations(1)
        assert np.isfinite(p).all() and np.abs(p.sum(axis=-1) - 1.0).max() < 1e-5    # the forward pass ran: the plain p
    finally:
        L.close()


def test_a_non_finite_context_poisons_nothing():
    """A STABLE_SOFTMAX handle whose by holds one +inf: z - zmax is inf - inf, so every p is NaN.  On a window whose weights
    are all 0 the weighted form SELECTS dy = +0 and a surprisal of 0 (0 * NaN would be NaN): the loss and the bits, which are
    the sums of colloss, are exactly 0, and the gradient block -- dby is the row sums of dy, dWhy its product with h -- is all
    zeros.  Then the same handle trains on the same texts with weight 1 and shows the NaN, so the 0 above was the selection.
    This runs no faulting path: only arithmetic on NaN."""
    import lstm_hip
    from oracle_lib import split_params
    case = tr.CASES[1]
    N, S, B, _ = case
    P = gu.random_case(N, S, B, seed=N + S + B)[0].copy()
    split_params(P, N, 256)["by"][37] = np.inf
    L = _handle(case, extra_flags=("STABLE_SOFTMAX",), P=P)
    txts = tr.case_texts(case, "queue")
    try:
        L.set_train_texts(txts, [0.0] * len(txts))
        loss = L.train_text_windows(1, LR)[0]
        _, p = L.get_activations(1)
        assert np.isnan(p).all()                                   # the context's p is what the window cannot use
        assert loss == 0.0 and not L.train_texts_bits().any()
        grads = L.get_grads()
        assert not grads.any() and np.isfinite(grads).all()
        after = L.get_params()
        assert after.tobytes() == P.tobytes()
        L.set_train_texts(txts, [1.0] * len(txts))
        assert np.isnan(L.train_text_windows(1, 0.0)[0])
    finally:
        L.close()


@pytest.mark.parametrize("case", [tr.CASES[1], tr.CASES[3], tr.CASES[7]], ids=tr.case_id)
def test_chunking_and_determinism(case):
    """with weights and with Adam, clipping, EMA and weight drop on: one call, calls of one window, another cut and a second
    handle give the same bytes"""
    txts, weights = wr.case_texts_and_weights(case, "queue", "drawn")
    n = len(tr.windows_ref(case[1], case[2], txts))
    assert n >= 3
    whole, _ = _run(case, txts, weights, [n], _everything_on)
    ones, _ = _run(case, txts, weights, [1] * n, _everything_on)
    cut, _ = _run(case, txts, weights, [2, 0, n - 2], _everything_on)
    again, _ = _run(case, txts, weights, [n], _everything_on)
    assert np.isfinite(whole["losses"]).all() and (whole["losses"] > 0).any()
    for name, other in (("calls of one window", ones), ("calls of 2, 0 and the rest", cut)):
        hr.assert_same({k: v for k, v in whole.items() if k != "norms"}, other, f"one call against {name}")
    hr.assert_same(whole, again, "a second handle with the same texts and weights")


def test_replacement_and_refusals():
    """weighted -> unweighted -> weighted on one handle is three fresh sets; a negative, a NaN and an infinite weight are
    refused with the stream and the byte's offset in the text, and the texts set before still train"""
    import lstm_hip
    case = tr.CASES[1]
    N, S, B, _ = case
    txts, weights = wr.case_texts_and_weights(case, "queue", "drawn")
    n = len(tr.windows_ref(S, B, txts))

    def reset(L):
        L.set_params(gu.random_case(N, S, B, seed=N + S + B)[0])
        L.set_params(np.zeros_like(L.get_params(lstm_hip.P_MEM)), lstm_hip.P_MEM)

    def trained(L, w):
        reset(L)
        assert L.set_train_texts(txts, w) == n and L.train_texts_progress() == (n, 0) and not L.train_texts_bits().any()
        losses = L.train_text_windows(n, 0.05)
        return dict(losses=losses, bits=L.train_texts_bits(), params=L.get_params(), mem=L.get_params(lstm_hip.P_MEM), grads=L.get_grads())

    fresh = []
    for w in (weights, None):
        L = _handle(case)
        try:
            fresh.append(trained(L, w))
        finally:
            L.close()
    assert fresh[0]["params"].tobytes() != fresh[1]["params"].tobytes()
    L = _handle(case)
    try:
        L.set_profiling(True)
        for i, (w, want) in enumerate(((weights, fresh[0]), (None, fresh[1]), (weights, fresh[0]))):
            L.reset_kernel_stats()
            hr.assert_same(want, trained(L, w), f"set number {i + 1} on one handle against a fresh handle")
            st = _stats(L)
            assert (st["softmax_loss_dy_weighted"], st["softmax_loss_dy_text"]) == ((n, 0) if w is not None else (0, n))
        L.set_profiling(False)

        # refusals: the handle keeps the weighted texts it has
        lib, p = L.lib, lstm_hip._ptr
        reset(L)
        assert L.set_train_texts(txts, weights) == n
        head = L.train_text_windows(1, 0.05)
        stats, steps = L.kernel_stats(), L.optimizer_steps()
        text = np.arange(10, dtype=np.uint8)
        off = np.array([0, 4, 10], np.uint64)

        def set_weighted(wv, streams=2, text=text, off=off):
            wv = None if wv is None else np.asarray(wv, np.float32)
            return lib.lstm_hip_set_train_texts_weighted(L._h, C.c_int32(streams), p(text, C.c_uint8) if text is not None else None,
                                                         p(off, C.c_uint64) if off is not None else None,
                                                         p(wv, C.c_float) if wv is not None else None)

        def refused(rc, msg):
            assert rc == lstm_hip.EINVAL, (rc, lib.lstm_hip_last_error().decode())
            assert lib.lstm_hip_last_error().decode() == msg

        good = np.ones(10, np.float32)
        for at, (stream, byte) in ((0, (0, 0)), (3, (0, 3)), (4, (1, 0)), (9, (1, 5))):      # byte 0 of a stream is validated too
            for bad, shown in ((-0.5, "-0.5"), (float("nan"), "nan"), (float("inf"), "inf"), (float("-inf"), "-inf")):
                wv = good.copy()
                wv[at] = bad
                refused(set_weighted(wv), f"set_train_texts_weighted: the weight of byte {byte} of stream {stream} is {shown}; "
                                          "a weight must be finite and >= 0")
        refused(set_weighted(good, streams=0), "set_train_texts: streams must be >= 1 (got 0)")       # ... in its existing words
        refused(set_weighted(good, off=None), "set_train_texts: null text_off")
        refused(set_weighted(good, off=np.array([1, 4, 10], np.uint64)), "set_train_texts: text_off[0] must be 0 (got 1)")
        refused(set_weighted(good, off=np.array([0, 11, 10], np.uint64)), "set_train_texts: text_off decreases at stream 1 (10 < 11)")
        refused(set_weighted(good, text=None), "set_train_texts: null text with 10 bytes to read")
        with pytest.raises(lstm_hip.LstmHipError):
            L.set_train_texts(txts, weights[:-1])                     # the wrapper: one array per text ...
        with pytest.raises(lstm_hip.LstmHipError):
            L.set_train_texts(txts, [np.ones(len(t) + 1, np.float32) for t in txts])      # ... of the text's length
        assert L.kernel_stats() == stats and L.optimizer_steps() == steps and L.train_texts_progress() == (n, 1)
        rest = L.train_text_windows(n - 1, 0.05)                      # the texts set before the refusals still train
        assert np.concatenate([head, rest]).tobytes() == fresh[0]["losses"].tobytes()
        assert set_weighted(np.array([0.0, -0.0, 1e-30, 3e38] + [1.0] * 6, np.float32)) == 0          # -0.0 is 0, not negative
        assert set_weighted(None, streams=0, text=None, off=None) == 0                                 # dropped
        assert lib.lstm_hip_train_text_windows(L._h, C.c_int64(1), C.c_double(0.1), None, None) == lstm_hip.ESTATE
    finally:
        L.close()


@pytest.mark.parametrize("shape", [s for s in hsc.SHAPES if s.forms in hsc.INFERENCE_ROWS], ids=hsc.shape_id)
def test_the_handle_stays_usable(shape):
    """after a weighted call, lstm_hip_train_windows on the same handle gives the bytes a fresh handle loaded with the same
    observable state gives: the window's weights are scratch and show in no later call"""
    text = np.frombuffer(bytes(gu.text_bytes(4000, 51)), np.uint8)
    txts = tr.texts(tr.lengths(shape.S, shape.B + 3, 77), 78)
    rs = np.random.RandomState(79)
    weights = [rs.choice(np.array(wr.DRAW, np.float32), size=len(t)).astype(np.float32) for t in txts]
    A, twin = hr.start(shape, text), None
    try:
        A.train_windows(2, hr.LR)
        cursors = A.get_cursors()
        n = A.set_train_texts(txts, weights)
        A.train_text_windows(n - 1, hr.LR)
        assert (A.get_cursors() == cursors).all()
        snap = hr.snapshot(A, text)
        twin = hr.restore(shape, snap)
        la, lt = A.train_windows(3, hr.LR), twin.train_windows(3, hr.LR)
        assert la.tobytes() == lt.tobytes()
        hr.assert_same(hr.snapshot(A, text), hr.snapshot(twin, text), "train_windows after weighted text windows against a fresh twin")
        A.train_text_windows(1, hr.LR)     # and the plan goes on where it stood
        assert A.train_texts_progress() == (n, n)
    finally:
        A.close()
        if twin is not None:
            twin.close()


def test_program_train_after(tmp_path):
    """lstm --records --train-after B: the epoch line counts the weight-1 target bytes ("trained bytes"), the figure is the
    weighted bits over them, and it differs from the run that learns every byte"""
    import os
    import re
    import subprocess
    lstm = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eigen-lstm_amd", "lstm")
    rs = np.random.RandomState(22)
    lines = []
    for i in range(100):
        key = bytes(rs.randint(97, 123, size=rs.randint(1, 6)).astype(np.uint8))
        lines.append((key + b"\t" + key[::-1] + b"\n") if i % 10 else key + b"\n")          # every tenth record has no separator
    f = tmp_path / "pairs.txt"
    f.write_bytes(b"".join(lines))
    trained = sum(len(x) - x.index(b"\t") - 1 for x in lines if b"\t" in x)
    scored = sum(len(x) - 1 for x in lines)
    args = [lstm, str(f), "32", "8", "4", "0.05", "--epochs", "2", "--seed", "1", "--sample", "0", "--records", "--quiet"]
    pat = r"records: (\d+) texts in (\d+) windows, ([\d.]+)% of the rows filled, ([\d.]+) prequential bits/char over (\d+) (trained )?bytes"

    def run(extra):
        out = subprocess.run(args + extra, capture_output=True, text=True, errors="replace", timeout=120)
        assert out.returncode == 0, out.stderr
        return re.findall(pat, out.stdout)

    plain, after = run([]), run(["--train-after", "9"])
    assert len(plain) == len(after) == 2
    assert all(int(r[4]) == scored and r[5] == "" for r in plain)
    assert all(int(r[4]) == trained and r[5] == "trained " and r[1] == p[1] and r[2] == p[2] for r, p in zip(after, plain))
    first, second = float(after[0][3]), float(after[1][3])
    assert 0.0 < second < first < 8.5, after            # learned from a flat start of 8 bits
    assert after[0][3] != plain[0][3]
