"""CPU side of lstm_hip_train_text_windows (include/lstm_hip.h): the header and the exports, the
schedule (lstm_hip_text_plan runs on the host) against the Python plan of tests/text_train_ref.py, and the reference the GPU
test (tests/test_train_texts.py) holds the call to: the truncation identity it rests on, and the mutant it has to tell apart."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import eval_texts_ref as er
import gpu_util as gu
import text_train_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lstm_hip_text_plan", "lstm_hip_set_train_texts", "lstm_hip_get_train_texts", "lstm_hip_train_text_windows",
       "lstm_hip_get_train_texts_bits")


def test_header_exports_and_wrapper():
    import lstm_hip
    code = open(os.path.join(ROOT, "include", "lstm_hip.h")).read()
    lib = lstm_hip.load_library()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, code) and name in lstm_hip.SYMBOLS and hasattr(lib, name), name
    for name in ("set_train_texts", "train_text_windows", "train_texts_bits"):
        assert callable(getattr(lstm_hip.Lstm, name))
    # the launches have statistics rows of their own, and the softmax's text form is a launch beside the old one
    api = open(os.path.join(ROOT, "eigen-lstm_amd", "csrc", "lstm_hip_api.cpp")).read()
    for kid, name in (("K_TEXT_WINDOW", "text_window"), ("K_TEXT_FOLD", "text_fold"), ("K_SOFTMAX_TEXT", "softmax_loss_dy_text")):
        assert re.search(r"RUN\(%s," % kid, api) and '"%s"' % name in api, kid
    kernels = open(os.path.join(ROOT, "eigen-lstm_amd", "csrc", "kernels.hip")).read()
    for sym in ("k_text_window", "k_text_fold", "k_softmax_loss_dy_text<true>", "k_softmax_loss_dy_text<false>"):
        assert sym in kernels, sym


@pytest.mark.parametrize("case,kind", tr.all_cases(), ids=[tr.case_id(c, k) for c, k in tr.all_cases()])
def test_plan_on_the_table(case, kind):
    import lstm_hip
    N, S, B, _ = case
    lens = [len(t) for t in tr.case_texts(case, kind)]
    assert len(lens) == tr.stream_count(kind, B)
    want = tr.plan_ref(S - 1, B, lens)
    got = lstm_hip.text_plan(S - 1, B, lens)
    assert got[0] == want[0] >= 1 and (got[1] == want[1]).all() and (got[2] == want[2]).all()
    wins = tr.windows_ref(S, B, tr.case_texts(case, kind))
    assert len(wins) == want[0]
    # every step of every stream stands in exactly one row, in order
    seen = {s: 0 for s in range(len(lens))}
    for win in wins:
        for lane in range(B):
            s, r = int(win["stream"][lane]), int(win["rows"][lane])
            assert (s < 0) == (r == 0)
            if s >= 0:
                assert win["j0"][lane] == seen[s] and win["fresh"][lane] == (seen[s] == 0)
                seen[s] += r
            assert (win["xi"][r + 1:, lane] == -1).all() and (win["ti"][r + 1:, lane] == -1).all()
    assert all(seen[s] == max(n - 1, 0) for s, n in enumerate(lens))
    ragged = [w for w in wins if (w["rows"] < S - 1).any()]
    assert ragged, "a case without a padded row shows nothing"
    if kind == "queue":   # a text starts on a lane another has just left
        assert any(((a["stream"] >= 0) & (b["stream"] >= 0) & (a["stream"] != b["stream"])).any() for a, b in zip(wins, wins[1:]))


def test_plan_on_random_offsets():
    import lstm_hip
    rs = np.random.RandomState(5)
    for _ in range(200):
        steps, lanes, streams = int(rs.randint(1, 40)), int(rs.randint(1, 12)), int(rs.randint(1, 60))
        lens = [int(v) for v in rs.choice([0, 1, 2, steps, steps + 1, steps + 2, 3 * steps + 2, int(rs.randint(0, 200))], size=streams)]
        want, got = tr.plan_ref(steps, lanes, lens), lstm_hip.text_plan(steps, lanes, lens)
        assert got[0] == want[0] and (got[1] == want[1]).all() and (got[2] == want[2]).all(), (steps, lanes, lens)


def test_eval_plan_is_the_text_plan_of_128_steps():
    import lstm_hip
    rs = np.random.RandomState(6)
    for lens in (list(er.LENGTHS), [int(v) for v in rs.randint(0, 700, size=50)]):
        for lanes in (1, 3, 16):
            a, b = lstm_hip.eval_plan(lanes, lens), lstm_hip.text_plan(128, lanes, lens)
            assert a[0] == b[0] and (a[1] == b[1]).all() and (a[2] == b[2]).all()
            c = er.plan_ref(lanes, lens)
            assert a[0] == c[0] and (a[1] == c[1]).all() and (a[2] == c[2]).all()


def test_plan_refusals():
    import lstm_hip
    lib = lstm_hip.load_library()
    off = np.array([0, 4, 10], np.uint64)

    def call(steps=4, lanes=2, streams=2, off=off):
        return lib.lstm_hip_text_plan(steps, lanes, streams, lstm_hip._ptr(off, C.c_uint64) if off is not None else None, None, None)

    assert call() == 2   # outputs may be NULL
    for kw, text in ((dict(steps=0), "text_plan: steps must be >= 1 (got 0)"),
                     (dict(lanes=0), "text_plan: lanes must be in [1, 4096] (got 0)"),
                     (dict(lanes=4097), "text_plan: lanes must be in [1, 4096] (got 4097)"),
                     (dict(streams=0), "text_plan: streams must be >= 1 (got 0)"),
                     (dict(off=None), "text_plan: null text_off"),
                     (dict(off=np.array([1, 4, 10], np.uint64)), "text_plan: text_off[0] must be 0 (got 1)"),
                     (dict(off=np.array([0, 11, 10], np.uint64)), "text_plan: text_off decreases at stream 1 (10 < 11)")):
        assert call(**kw) == lstm_hip.EINVAL, kw
        assert lib.lstm_hip_last_error().decode() == text
    assert lib.lstm_hip_eval_plan(0, 2, lstm_hip._ptr(off, C.c_uint64), None, None) == lstm_hip.EINVAL
    assert lib.lstm_hip_last_error().decode() == "eval_plan: lanes must be in [1, 4096] (got 0)"   # under its own name, as before


def test_truncation_identity(oracle64):
    """On a window without padding the sum of the B one-lane oracle gradients is the B-column oracle gradient, and the
    lanes' losses sum to B times its loss, to float64 rounding: what lets the reference be built lane by lane."""
    N, S, B = 16, 5, 3
    P, _, _, h0, c0 = gu.random_case(N, S, B, seed=9)
    txts = tr.texts([2 * (S - 1) + 1] * B, seed=10)      # two whole windows on every lane
    wins = tr.windows_ref(S, B, txts)
    assert len(wins) == 2 and all((w["rows"] == S - 1).all() for w in wins)
    win = wins[1]                                         # the one that continues: the carry is read
    assert not win["fresh"].any()
    by_lane = tr.window_ref(oracle64, N, P, win, h0, c0)
    whole = tr.window_ref(oracle64, N, P, win, h0, c0, mutant=True)
    assert abs(by_lane["loss"] - whole["loss"]) <= 1e-12 * (S - 1)
    rep = gu.grads_report(by_lane["grads"], whole["grads"], N)
    assert max(rep.values()) <= 1e-12, rep
    fw = oracle64.forward(N, 256, S, B, P, win["xi"], win["ti"], h0, c0)
    assert by_lane["mask"][1:].all() and gu.max_rel(by_lane["probs"][1:], fw["probs"][1:]) <= 1e-13


def _oracle(case, oracle32, oracle64):
    return oracle32 if "BF16_RECURRENCE" in case[3] else oracle64


@pytest.mark.parametrize("case,kind", tr.all_cases(), ids=[tr.case_id(c, k) for c, k in tr.all_cases()])
def test_the_gradient_tolerance_tells_the_mutant_apart(case, kind, oracle32, oracle64):
    """A reference that gives dy = p on the padded rows (the oracle on the window as it stands) must fall outside the
    gradient tolerance of the right one, on the most padded window of every case: otherwise the case shows nothing."""
    N, S, B, flags = case
    orc = _oracle(case, oracle32, oracle64)
    P, _, _, h0, c0 = gu.random_case(N, S, B, seed=N + S + B, scale=0.05 if "BF16_RECURRENCE" in flags else 0.08)
    wins = tr.windows_ref(S, B, tr.case_texts(case, kind))
    win = max(wins, key=lambda w: int((S - 1 - w["rows"]).sum()))
    bf16 = "BF16_RECURRENCE" in flags
    if bf16:
        orc.set_bf16_recurrence(True), orc.set_bf16_products(True)
    try:
        right = tr.window_ref(orc, N, P, win, h0, c0)
        wrong = tr.window_ref(orc, N, P, win, h0, c0, mutant=True)
    finally:
        if bf16:
            orc.set_bf16_recurrence(False), orc.set_bf16_products(False)
    rep = gu.grads_report(wrong["grads"], right["grads"], N)
    tol = tr.tolerances(case)[2]
    print(f"{tr.case_id(case, kind)}: {int((S - 1 - win['rows']).sum())} padded rows, mutant off by {max(rep.values()):.3g} (tolerance {tol:g})")
    assert max(rep.values()) > tol, rep
    assert abs(wrong["loss"] - right["loss"]) <= 1e-4 * (S - 1)   # (the loss cannot tell them apart: colloss is 0 either way)


def test_program_option_refusals():
    """the refusals of lstm --records that are decided before any device is touched: exit status 2 and the message"""
    import subprocess
    lstm = os.path.join(ROOT, "eigen-lstm_amd", "lstm")
    base = [lstm, "nofile.txt", "32", "8", "4", "0.05"]
    for extra, text in ((["--record-delim", "10"], "--record-delim needs --records"),
                        (["--shuffle-seed", "3"], "--shuffle-seed needs --records"),
                        (["--records", "--record-delim", "256"], "--record-delim needs a byte value 0..255"),
                        (["--records", "--gpus", "2"], "--records runs on one GPU"),
                        (["--records", "--stride", "2"], "--records does not take --stride"),
                        (["--records", "--last-step-loss"], "--records reports the all-steps loss only")):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and text in out.stderr, (extra, out.stderr)
    usage = subprocess.run([lstm, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--records --record-delim B --shuffle-seed K" in usage
