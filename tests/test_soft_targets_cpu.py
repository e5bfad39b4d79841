"""Device-free control of tests/soft_target_ref.py, the reference of lstm_hip_set_soft_targets (include/lstm_hip.h; DESIGN.md
section 3.19): the probs-as-dy identity it rests on, its agreement with oracle.backward where the feature is off, a numeric
gradient check of alpha CE + (1 - alpha) tau^2 KL, three mutants it must tell apart, its own float32 error against the
tolerances of tests/test_soft_targets.py, and the exported symbols."""
import ctypes as C

import numpy as np
import pytest

import gpu_util as gu
import soft_target_ref as sr

SMALL = ((16, 5, 3, ()), (24, ()))


@pytest.fixture(autouse=True, scope="module")
def _the_library_has_the_call():
    """the reference restates lstm_hip_set_soft_targets: without the call in the built library there is nothing to control"""
    import lstm_hip
    assert hasattr(lstm_hip.load_library(), "lstm_hip_set_soft_targets"), "liblstm_hip.so lacks lstm_hip_set_soft_targets"


def test_probs_as_dy_is_the_ordinary_backward(oracle64):
    """ti = -1 everywhere with dy in place of probs gives oracle.backward's bytes (one empty target in the window)"""
    (N, S, B, _), _ = SMALL
    inp = sr.case_inputs(SMALL)
    assert (inp["ti"][1:] < 0).sum() == 1
    fw = oracle64.forward(N, 256, S, B, inp["P"].astype(np.float64), inp["xi"], inp["ti"], inp["h0"], inp["c0"])
    want = oracle64.backward(N, 256, S, B, inp["P"].astype(np.float64), inp["xi"], inp["ti"], fw)
    dy = fw["probs"].copy()
    for t in range(1, S):
        for b in range(B):
            if inp["ti"][t, b] >= 0:
                dy[t, b, inp["ti"][t, b]] -= 1.0
    got = sr.backward_dy(oracle64, N, inp["P"], inp["xi"], fw, dy)
    assert got.tobytes() == want.tobytes()


def test_off_is_the_oracles_backward(oracle64):
    (N, S, B, _), _ = SMALL
    inp = sr.case_inputs(SMALL)
    ref = sr.window(oracle64, SMALL, inp, (1.0, 1.0, 0.0), teacher=False)
    want = oracle64.backward(N, 256, S, B, inp["P"].astype(np.float64), inp["xi"], inp["ti"], ref["fw"])
    assert ref["grads"].tobytes() == want.tobytes() and ref["kl"] == 0.0


def _numeric_check(orc, setting, mutant=None):
    """central differences (delta 1e-5, float64) of the objective on 16 entries of each tensor against the reference's
    gradients; returns the worst (max rel, mean rel, abs / scale) over the tensors, in the form of the gradient check of
    tests/test_oracle_pinning.py"""
    (N, S, B, _), _ = SMALL
    inp = sr.case_inputs(SMALL, empty=False)
    assert (inp["ti"][1:] >= 0).all()
    P = inp["P"].astype(np.float64)
    ana = sr.window(orc, SMALL, inp, setting, mutant=mutant, P=P)["grads"]
    rs = np.random.RandomState(0)
    worst = [0.0, 0.0, 0.0]
    o, delta = 0, 1e-5
    for name, r, c in (("W", 4 * N, 256), ("U", 4 * N, N), ("b", 4 * N, 1), ("Why", 256, N), ("by", 256, 1)):
        idx = o + rs.choice(r * c, size=16, replace=False)
        num = np.zeros(16)
        for j, i in enumerate(idx):
            vals = []
            for sgn in (1.0, -1.0):
                Q = P.copy()
                Q[i] += sgn * delta
                vals.append(sr.window(orc, SMALL, inp, setting, P=Q)["value"])
            num[j] = (vals[0] - vals[1]) / (2 * delta)
        a = ana[idx]
        den = np.abs(a + num)
        rel = np.where(den > 0, np.abs(a - num) / np.where(den > 0, den, 1), 0.0)
        worst = [max(worst[0], rel.max()), max(worst[1], rel.mean()), max(worst[2], np.abs(a - num).max() / max(1.0, np.abs(a).max()))]
        o += r * c
    return worst


def _numeric_ok(w):
    return w[0] <= 1e-1 and w[1] <= 1e-3 and w[2] <= 1e-7      # test_gradient_check_reference_thresholds' bounds


@pytest.mark.parametrize("setting", [(0.5, 2.0, 0.1), (0.0, 4.0, 0.0)], ids=str)
def test_numeric_gradient(oracle64, setting):
    w = _numeric_check(oracle64, setting)
    print(f"{setting}: max rel {w[0]:.3g}, mean rel {w[1]:.3g}, abs {w[2]:.3g}")
    assert _numeric_ok(w), w


def test_mutants_are_caught(oracle64):
    """the factor tau dropped: the numeric check fails; smoothing mass on an empty-target column, the teacher's term left out
    of one: the gradients leave a table case's tolerance"""
    assert not _numeric_ok(_numeric_check(oracle64, (0.5, 2.0, 0.1), mutant="no_tau"))
    case = sr.CASES[0]
    inp = sr.case_inputs(case)
    assert (inp["ti"][1:] < 0).sum() == 1
    good = sr.window(oracle64, case, inp, (0.5, 2.0, 0.1))
    for mutant in ("smooth_empty", "no_teacher_on_empty"):
        bad = sr.window(oracle64, case, inp, (0.5, 2.0, 0.1), mutant=mutant)
        fig = sr.compare(bad, good, case[0][1])
        assert fig["grad"] > sr.tolerances(case)[2], (mutant, fig)
    assert set(sr.MUTANTS) == {"no_tau", "smooth_empty", "no_teacher_on_empty"}


@pytest.mark.parametrize("case", sr.CASES, ids=[sr.case_id(c) for c in sr.CASES])
def test_float32_reference_is_well_inside_the_tolerances(case, oracle32, oracle64):
    """the float32 reference against the float64 one (both in the oracle's bf16 modes where the case has them) stays within
    half of the case's tolerances on every setting"""
    act_tol, loss_tol, grad_tol = sr.tolerances(case)
    S = case[0][1]
    inp = sr.case_inputs(case)
    for i, setting in enumerate(sr.SETTINGS):
        a = sr.window(oracle32, case, inp, setting, teacher=i > 0)
        b = sr.window(oracle64, case, inp, setting, teacher=i > 0)
        fig = sr.compare(a, b, S)
        print(f"{sr.case_id(case)} {setting}: {fig}")
        assert fig["act"] <= act_tol / 2 and fig["loss"] <= loss_tol / 2 and fig["kl"] <= loss_tol / 2, (setting, fig)
        assert fig["grad"] <= grad_tol / 2, (setting, fig)
        assert (b["kl"] > 1e-3) == (i > 0)       # the teacher's term is there to be measured


def test_symbols_are_exported():
    import lstm_hip
    lib = lstm_hip.load_library()
    for name in ("lstm_hip_set_soft_targets", "lstm_hip_get_soft_targets", "lstm_hip_get_teacher_kl"):
        assert name in lstm_hip.SYMBOLS and hasattr(lib, name), name
    assert C.sizeof(lstm_hip._SoftTargets) == 32
