"""CPU side of lstm_hip_set_train_texts_weighted (include/lstm_hip.h): the header, the export and the
wrapper; and the reference the GPU test (tests/test_train_texts_weighted.py) holds the weighted windows to,
tests/text_weight_ref.py: against torch float64 autograd of the weighted loss, against the unweighted reference at weight 1,
its batched oracle runs against runs of one lane, and the two mutants it has to tell apart on every case of the GPU test."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gpu_util as gu
import text_train_ref as tr
import text_weight_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "lstm_hip_set_train_texts_weighted"


def test_header_export_wrapper_and_statistics_row():
    import lstm_hip
    code = open(os.path.join(ROOT, "include", "lstm_hip.h")).read()
    lib = lstm_hip.load_library()
    assert re.search(r"\b%s\(" % NAME, code) and NAME in lstm_hip.SYMBOLS and hasattr(lib, NAME)
    assert callable(lstm_hip.completion_weights)
    assert "weights" in lstm_hip.Lstm.set_train_texts.__code__.co_varnames
    api = open(os.path.join(ROOT, "eigen-lstm_amd", "csrc", "lstm_hip_api.cpp")).read()
    assert re.search(r"RUN\(K_SOFTMAX_WEIGHTED,", api) and '"softmax_loss_dy_weighted"' in api
    # the unweighted set is a caller of the weighted one, and the text form of the softmax launch is still there
    body = api[api.index("int lstm_hip_set_train_texts(lstm_hip_t *h"):]
    body = body[:body.index("}")]
    assert "return lstm_hip_set_train_texts_weighted(h, streams, text, text_off, nullptr);" in body
    assert re.search(r"RUN\(K_SOFTMAX_TEXT,", api)
    kernels = open(os.path.join(ROOT, "eigen-lstm_amd", "csrc", "kernels.hip")).read()
    for sym in ("k_softmax_loss_dy_weighted<true>", "k_softmax_loss_dy_weighted<false>", "softmax_loss_dy_body<STABLE, true, true>",
                "softmax_loss_dy_body<STABLE, false>", "softmax_loss_dy_body<STABLE, true>"):
        assert sym in kernels, sym
    # a call without a handle is refused before anything is read
    assert lib.lstm_hip_set_train_texts_weighted(None, C.c_int32(1), None, None, None) == lstm_hip.EINVAL


def test_completion_weights():
    import lstm_hip
    texts = [b"key\tvalue\n", b"\tx", b"x\t", b"none", b"", b"a\tb\tc", np.frombuffer(b"q\tr", np.uint8)]
    got = lstm_hip.completion_weights(texts, 9)
    want = wr.completion_weights_ref(texts, 9)
    assert len(got) == len(texts)
    for g, w, t in zip(got, want, texts):
        assert g.dtype == np.float32 and g.shape == (len(t),) and (g == w).all(), t
    assert got[0].tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 1, 1] and got[1].tolist() == [0, 1] and got[2].tolist() == [0, 0]
    assert not got[3].any() and got[5].tolist() == [0, 0, 1, 1, 1]          # the FIRST separator; a later one is learned
    for sep in (-1, 256):
        with pytest.raises(lstm_hip.LstmHipError):
            lstm_hip.completion_weights(texts, sep)


def _case(N=12, S=6, seed=5):
    """a window that continues two texts (one to its end, so it has padded rows) and has an idle lane, with a carry"""
    B, L = 3, S - 1
    txts = tr.texts([2 * L + 1, L + 3, 1], seed=seed)
    wins = tr.windows_ref(S, B, txts)
    assert len(wins) == 2
    win = wins[1]
    assert win["rows"].tolist() == [L, 2, 0] and win["fresh"].tolist() == [False, False, True]
    P, _, _, h0, c0 = gu.random_case(N, S, B, seed=seed + 1, scale=0.3)
    return N, S, B, txts, win, P, h0, c0


def _torch_weighted(P, N, S, B, xi, ti, wt, h0, c0, M=256):
    """The recurrence of tests/test_oracle_pinning.py::_torch_model (torch ops and autograd, nothing shared with the oracle)
    with the loss sum_t w_t (-ln p_t[target]).  Returns (weighted bits / B, the gradient of the weighted nats)."""
    import torch
    torch.set_num_threads(1)
    Pt = torch.tensor(np.asarray(P, np.float64), dtype=torch.float64, requires_grad=True)
    o, mats = 0, {}
    for name, r, c in (("W", 4 * N, M), ("U", 4 * N, N), ("b", 4 * N, 1), ("Why", M, N), ("by", M, 1)):
        mats[name] = Pt[o:o + r * c].reshape(c, r).T  # column-major
        o += r * c
    h = torch.tensor(np.asarray(h0, dtype=np.float64).T)
    c = torch.tensor(np.asarray(c0, dtype=np.float64).T)
    nats = torch.zeros((), dtype=torch.float64)
    for t in range(1, S):
        x = torch.zeros(M, B, dtype=torch.float64)
        for b in range(B):
            if xi[t, b] >= 0:
                x[xi[t, b], b] = 1.0
        g = mats["W"] @ x + mats["U"] @ h + mats["b"]
        i, o_, f, u = torch.sigmoid(g[:N]), torch.sigmoid(g[N:2 * N]), torch.sigmoid(g[2 * N:3 * N]), torch.tanh(g[3 * N:])
        c = torch.tanh(i * u + f * c)
        h = o_ * c
        y = mats["Why"] @ h + mats["by"]
        logp = y - torch.logsumexp(y, 0, keepdim=True)
        for b in range(B):
            if ti[t, b] >= 0:
                nats = nats - float(wt[t, b]) * logp[ti[t, b], b]
    nats.backward()
    return float(nats.detach()) / np.log(2.0) / B, Pt.grad.numpy()


def test_reference_against_autograd(oracle64):
    """the telescoped reference is the gradient of sum w_t (-ln p_t): float64 autograd of an independent model agrees to
    rounding, and a reference that ignores the weights is nowhere near"""
    N, S, B, txts, win, P, h0, c0 = _case(N=16, S=7)
    wt = np.zeros((S, B), np.float32)
    wt[1:, 0] = [0, 0, 1, 0.25, 0, 3]      # context in front, a weight-0 byte in the middle of what is learned
    wt[1:3, 1] = [0.25, 0]                 # (this lane's text ends behind row 2; the third lane is idle)
    h_in, c_in = np.where(win["fresh"][:, None], 0.0, h0), np.where(win["fresh"][:, None], 0.0, c0)
    bits, grad = _torch_weighted(P, N, S, B, win["xi"], win["ti"], wt, h_in, c_in)
    ref = wr.window_ref(oracle64, N, P, win, wt, h0, c0)
    scale = np.abs(grad).max()
    err = np.abs(ref["grads"] - grad).max()
    off = np.abs(wr.window_ref(oracle64, N, P, win, wt, h0, c0, mutant="ignored")["grads"] - grad).max()
    print(f"telescoped reference against autograd: {err:.3g} at a gradient scale of {scale:.3g}; weights ignored: {off / scale:.3g} of the scale")
    assert err <= 1e-9 * scale and abs(ref["loss"] - bits) <= 1e-12 * (S - 1)
    assert off > 0.1 * scale
    assert abs(ref["surprisal"].sum() / B - bits) <= 1e-12 * (S - 1)
    assert not ref["surprisal"][wt == 0].any()


@pytest.mark.parametrize("together", [True, False], ids=["batched", "one-lane"])
def test_reference_at_weight_one_is_the_unweighted_reference(oracle64, together):
    N, S, B, txts, win, P, h0, c0 = _case(N=16, seed=8)
    ones = wr.window_weights(win, [np.ones(len(t), np.float32) for t in txts])
    assert ones[1:][win["ti"][1:] >= 0].all() and not ones[win["ti"] < 0].any() and not ones[0].any()
    a = wr.window_ref(oracle64, N, P, win, ones, h0, c0, together=together)
    b = tr.window_ref(oracle64, N, P, win, h0, c0)
    assert max(gu.grads_report(a["grads"], b["grads"], N).values()) <= 1e-12 and abs(a["loss"] - b["loss"]) <= 1e-12
    assert (a["mask"] == b["mask"]).all() and np.abs(a["surprisal"] - b["surprisal"]).max() <= 1e-12
    for name in ("h", "c", "g", "probs"):
        assert gu.max_rel(a[name][a["mask"]], b[name][b["mask"]]) <= 1e-13, name


def test_batched_oracle_runs_are_the_one_lane_runs(oracle64):
    """lanes with one coefficient share an oracle run (text_weight_ref.window_ref): the result is that of B = 1 runs"""
    case, kind, wkind = wr.LOCK_STEP[1][0], "queue", "drawn"
    N, S, B, _ = case
    txts, weights = wr.case_texts_and_weights(case, kind, wkind)
    P, _, _, h0, c0 = gu.random_case(N, S, B, seed=N + S + B)
    win, wt = wr.fullest_window(tr.windows_ref(S, B, txts), weights)
    a, b = (wr.window_ref(oracle64, N, P, win, wt, h0, c0, together=t) for t in (True, False))
    assert max(gu.grads_report(a["grads"], b["grads"], N).values()) <= 1e-12 and abs(a["loss"] - b["loss"]) <= 1e-12 * (S - 1)
    assert np.abs(a["surprisal"] - b["surprisal"]).max() <= 1e-12


def test_window_weights_follow_the_targets():
    """row t of a lane holding step j carries the stream's entry j + 1; every other row 0; every entry but byte 0 is used once"""
    for case, kind, wkind in wr.lock_step_params():
        N, S, B, _ = case
        txts, weights = wr.case_texts_and_weights(case, kind, wkind)
        assert all(w.dtype == np.float32 and w.shape == (len(t),) for w, t in zip(weights, txts))
        if wkind == "drawn":
            assert set(np.concatenate(weights).tolist()) <= set(wr.DRAW)
        else:
            seps = [int(np.flatnonzero(t == wr.SEP)[0]) if (t == wr.SEP).any() else None for t in txts]
            assert all((t == wr.SEP).sum() <= 1 for t in txts)
            if len(txts) >= 8:      # the edges: the separator as the first byte, as the last byte, absent
                first, last, absent = [i for i, t in enumerate(txts) if len(t) >= 2][-3:]
                assert seps[first] == 0 and seps[last] == len(txts[last]) - 1 and seps[absent] is None
                assert weights[first][1:].all() and not weights[last].any() and not weights[absent].any()
        total = 0.0
        for win in tr.windows_ref(S, B, txts):
            wt = wr.window_weights(win, weights)
            assert not wt[0].any() and not wt[win["ti"] < 0].any()
            for lane in range(B):
                s, j0 = int(win["stream"][lane]), int(win["j0"][lane])
                for t in range(1, int(win["rows"][lane]) + 1):
                    assert wt[t, lane] == weights[s][j0 + t] and win["ti"][t, lane] == txts[s][j0 + t]
            total += float(wt.sum(dtype=np.float64))
        assert total == sum(float(w[1:].sum(dtype=np.float64)) for w in weights)


def _oracle(case, oracle32, oracle64):
    return oracle32 if "BF16_RECURRENCE" in case[3] else oracle64


@pytest.mark.parametrize("case,kind,wkind", wr.lock_step_params(), ids=[wr.lock_step_id(p) for p in wr.lock_step_params()])
def test_the_gradient_tolerance_tells_the_mutants_apart(case, kind, wkind, oracle32, oracle64):
    """On the fullest window of every case of the GPU test a reference that ignores the weights, and one that takes a
    weight-0 row for a text's end, fall outside the gradient tolerance of the right one: otherwise the case shows nothing."""
    N, S, B, flags = case
    orc = _oracle(case, oracle32, oracle64)
    bf16 = "BF16_RECURRENCE" in flags
    P, _, _, h0, c0 = gu.random_case(N, S, B, seed=N + S + B, scale=0.05 if bf16 else 0.08)
    txts, weights = wr.case_texts_and_weights(case, kind, wkind)
    win, wt = wr.fullest_window(tr.windows_ref(S, B, txts), weights)
    if bf16:
        orc.set_bf16_recurrence(True), orc.set_bf16_products(True)
    try:
        right = wr.window_ref(orc, N, P, win, wt, h0, c0)
        off = {m: max(gu.grads_report(wr.window_ref(orc, N, P, win, wt, h0, c0, mutant=m)["grads"], right["grads"], N).values())
               for m in ("ignored", "cut")}
    finally:
        if bf16:
            orc.set_bf16_recurrence(False), orc.set_bf16_products(False)
    tol = tr.tolerances(case)[2]
    print(f"{wr.lock_step_id((case, kind, wkind))}: {int(win['rows'].sum())} filled rows, {int((wt != 0).sum())} with a weight; weights "
          f"ignored: off by {off['ignored']:.3g}, cut at a weight-0 row: off by {off['cut']:.3g} (tolerance {tol:g})")
    assert off["ignored"] > tol and off["cut"] > tol, off


def test_program_option_refusals():
    """lstm --train-after: decided before any device is touched: exit status 2 and the message"""
    lstm = os.path.join(ROOT, "eigen-lstm_amd", "lstm")
    base = [lstm, "nofile.txt", "32", "8", "4", "0.05"]
    for extra, text in ((["--train-after", "9"], "--train-after needs --records"),
                        (["--records", "--train-after", "256"], "--train-after needs a byte value 0..255"),
                        (["--records", "--train-after", "-1"], "--train-after")):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and text in out.stderr, (extra, out.stderr)
    usage = subprocess.run([lstm, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--train-after B" in usage and "--records --record-delim B --shuffle-seed K" in usage
