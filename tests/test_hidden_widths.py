"""-m gpu: hidden widths outside the persistent forms, on every entry point, against the oracle.

An fp32 handle has a persistent recurrence at hidden 64, 128, 256, 512 and 1024 only (plan_engine, csrc/persistent.hip); 192,
320, 768, every width above 1024 and every padded width off that list train, evaluate and sample on the per-step engine, and
so does 1024 with more streams than its grid holds.  The host programs always pad, so `lstm text 768 ...` or `lstm text 2000
...` runs there.  The other suites run that engine at hidden 16 to 128 and once at 512, where k_fwd_step and k_bwd_step have
one operand chunk or only full ones; here every case is at a width the plan itself puts there (hidden_width_cases.py: no
case passes LSTM_HIP_STEP_KERNELS, every case asserts its plan and fails, not skips, on another):

  window cases     one window and one Adagrad step per row of hidden_width_cases.SHAPES against the float64 oracle: h, c, g
                   and probs of every step within 2e-5 of the step's scale, loss 2e-5 bits per step, gradients per tensor and
                   per dW column 2e-4 of scale, db against dW, the stepped parameters within 2e-4 lr where the gradient is
                   above noise, the memory within 1e-3
  padded twins     (1030 -> 1040) and (30 -> 32): bit identity with the explicit padded model, evaluator and sampler included
  device loop      train_windows at (192, 6, 17) and (1040, 4, 5) in lock step with the oracle's trainer (hidden 1040 at
                   learning rate 0.01: hidden_width_cases.LOOPS says why)
  evaluator        k_eval_bits at 192, 320, 1040, 2688 and 2704 against the float32 oracle's, 1e-4 bits per character
  sampler          k_sample at 192, 1040 and 2704 against the float32 oracle's: at least 99 % of the draws, then the states
The evaluator and the sampler keep h, c and the gates in (6 N + 256) * 4 bytes of LDS: 64 KB, what a launch gets unasked, at
2688.  Above, the kernels are granted their request first and both calls return LSTM_HIP_EINVAL, naming N, where the
device's limit per workgroup is below it (include/lstm_hip.h); before, nothing read the status of either launch.  A gfx950
has 160 KB per CU: 6800 is past that on every device, 2704 is an answer or a refusal by the limit the message names.

Worst figures on an MI355X (every case: profiles/hidden_widths/parity.jsonl), beside the control's (the float32 oracle
against the float64 oracle, tests/test_hidden_widths_cpu.py):
                                       fp32 handles   float32 oracle   tolerance
  h, c, g, probs, of the step's scale     7.7e-7          1.4e-6          2e-5
  loss, bits per step                     5.7e-7          3.5e-7          2e-5
  gradient tensor, of scale               7.6e-7          8.3e-7          2e-4
  dW per byte column, of scale            8.3e-7          1.0e-6          2e-4
  db - sum dW, of max|db|                 2.8e-7          1.3e-7          2e-4
  stepped parameters (lr 0.1)             3.0e-8          3.0e-8          2.1e-5
Device loop: loss within 3.8e-6 bits, carry 1.0e-6, parameters 2.6e-6 of 2.1e-5 (192) and 1.6e-7 of 3e-6 (1040).  Evaluator:
within 4.4e-7 bits per character at every width, 2704 included (the device's limit per workgroup is 160 KB).  Sampler: every
draw equal, states within 1.1e-6.  6800 refused by both calls.  The file takes 10 s beside 16 CPUs.
"""
import json
import os
import re
import time

import numpy as np
import pytest

import gpu_util as gu
import hidden_width_cases as hwc
from test_hip_parity import device_loop_follows_the_oracle_trainer
from test_pad_hidden import _twins

pytestmark = pytest.mark.gpu

REPORT = os.environ.get("HIDDEN_WIDTHS_REPORT")  # a file to append one JSON line per case to (profiles/hidden_widths)


def _report(rec):
    print(rec)
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(json.dumps(rec) + "\n")


@pytest.fixture(scope="module")
def references(request):
    t0 = time.time()
    cases = hwc.selected_cases(request)
    pool = hwc.ReferencePool(cases, fn=hwc.any_reference, key=hwc.any_id)
    yield pool
    pool.close()
    _report(dict(file="tests/test_hidden_widths.py", wall_seconds=round(time.time() - t0, 1), references=len(cases)))


def _step_handle(N, S=2, B=1, flags=0, want=hwc.STEP):
    import lstm_hip
    L = lstm_hip.Lstm(N, S, B, flags=flags)
    try:
        return L, hwc.assert_plan(L, want)
    except BaseException:
        L.close()
        raise


@pytest.mark.parametrize("case", hwc.CASES, ids=hwc.case_id)
def test_window_on_the_planned_step_engine(case, references):
    import lstm_hip
    sh = case.shape
    P, xi, ti, h0, c0 = hwc.inputs(case)
    flags = 0
    for f in sh.flags:
        flags |= getattr(lstm_hip, f)
    L, plan = _step_handle(sh.N, sh.S, sh.B, flags, sh.plan)
    try:
        L.set_params(P)
        L.set_state(0, h0, c0)
        L.set_window(xi, ti)
        L.forward()
        got = dict(loss=L.loss(), h=[], c=[], g=[], probs=[])
        for t in range(1, sh.S):
            h, c = L.get_state(t)
            g, p = L.get_activations(t)
            got["h"].append(h), got["c"].append(c), got["g"].append(g), got["probs"].append(p)
        got["h_last"] = got["h"][-1]
        L.backward()
        got["grads"] = L.get_grads()
        L.adagrad(hwc.LR)
        got["params"], got["mem"] = L.get_params(), L.get_params(lstm_hip.P_MEM)
    finally:
        L.close()
    fig = None
    try:
        fig = hwc.check_case(case, got, references.get(case), xi)
    finally:
        _report(dict(case=hwc.case_id(case), what=sh.path, plan=plan, k_steps=hwc.k_steps(sh), figures=fig))


@pytest.mark.parametrize("N,S,B", [(1030, 3, 5), (30, 4, 9)])
def test_padded_twins_on_the_step_engine(N, S, B):
    """test_pad_hidden.py's bit identity with the explicit padded model, at widths whose padded width has no persistent
    recurrence either (1040, 32): losses, every block, states, activations, the evaluator and the sampler."""
    import lstm_hip
    L, _ = _step_handle(N, S, B, lstm_hip.PAD_HIDDEN, dict(hwc.STEP, np=-(-N // 16) * 16))
    L.close()
    _twins(N, S, B, 0, windows=3)


@pytest.mark.parametrize("N,S,B,windows,lr", hwc.LOOPS)
def test_device_loop_follows_the_oracle_trainer(N, S, B, windows, lr, oracle32):
    fig = device_loop_follows_the_oracle_trainer(N, S, B, windows, oracle32, plan=hwc.STEP, lr=lr)
    _report(dict(loop=f"{N}x{S}x{B}", windows=windows, lr=lr, figures=fig))


def _refused(N, call, what):
    """The call must raise LSTM_HIP_EINVAL with a message that names N and a limit below the kernels' request."""
    import lstm_hip
    with pytest.raises(lstm_hip.LstmHipError) as e:
        call()
    text = str(e.value)
    m = re.search(r"needs (\d+) bytes of LDS in one workgroup, the device grants (\d+)", text)
    assert text.startswith(f"lstm_hip error {lstm_hip.EINVAL}:") and f"{what}: N={N} " in text and m, text
    assert int(m.group(1)) == hwc.lds_bytes(N) and hwc.LDS_UNASKED <= int(m.group(2)) < hwc.lds_bytes(N), text
    return int(m.group(2))


def _still_usable(L, N):
    """after a refusal the handle goes on taking and returning a state"""
    h0 = (np.random.RandomState(1).randn(1, N) * 0.1).astype(np.float32)
    L.set_state(0, h0, -h0)
    h, c = L.get_state(0)
    assert np.array_equal(h, h0) and np.array_equal(c, -h0)


@pytest.mark.parametrize("case", hwc.EVAL, ids=hwc.aux_id)
def test_evaluator_in_one_workgroup(case, references):
    import lstm_hip
    N = case.N
    P, text = hwc.aux_inputs(case)
    L, plan = _step_handle(N)
    try:
        L.set_params(P)
        want = references.get(case)
        rec = dict(eval=N, bytes=int(text.size), plan=plan, lds_bytes=hwc.lds_bytes(N))
        try:
            got = L.eval_bits(text)
        except lstm_hip.LstmHipError:
            assert hwc.lds_bytes(N) > hwc.LDS_UNASKED, "refused below what every launch is granted"
            rec["refused_by_limit"] = _refused(N, lambda: L.eval_bits(text), "eval_bits")
            _still_usable(L, N)
            _report(rec)
            return
        rec.update(bits=got, difference=abs(got - want))
        _report(rec)
        assert abs(got - want) <= hwc.EVAL_TOL, (got, want)
        assert L.eval_bits(text) == got                     # (the same launch again: granted once, the same sum)
    finally:
        L.close()


@pytest.mark.parametrize("case", hwc.SAMPLE, ids=hwc.aux_id)
def test_sampler_in_one_workgroup(case, references):
    import lstm_hip
    N = case.N
    P, h0, c0, u = hwc.aux_inputs(case)
    L, plan = _step_handle(N)
    try:
        L.set_params(P)
        want, hw, cw = references.get(case)
        rec = dict(sample=N, draws=int(u.size), plan=plan, lds_bytes=hwc.lds_bytes(N))
        try:
            got, hg, cg = L.sample(h0, c0, u)
        except lstm_hip.LstmHipError:
            assert hwc.lds_bytes(N) > hwc.LDS_UNASKED, "refused below what every launch is granted"
            rec["refused_by_limit"] = _refused(N, lambda: L.sample(h0, c0, u), "sample")
            _still_usable(L, N)
            _report(rec)
            return
    finally:
        L.close()
    # test_generate.py's rule: identical draws pick identical bytes unless u lands within rounding of a cdf edge
    rec["agree"] = float((got == want).mean())
    if (got == want).all():
        rec.update(h=gu.max_rel(hg, hw), c=gu.max_rel(cg, cw))
    _report(rec)
    assert rec["agree"] >= 0.99, rec
    if (got == want).all():
        assert rec["h"] <= 1e-3 and rec["c"] <= 1e-3, rec


def test_width_past_the_lds_of_a_cu_is_refused_by_both():
    """(6 * 6800 + 256) * 4 bytes are more than the 160 KB a gfx950 CU has: LSTM_HIP_EINVAL naming N, not a launch that the
    runtime refuses behind the caller's back, and a handle that goes on working."""
    N = hwc.N_PAST_LDS
    assert hwc.lds_bytes(N) > hwc.LDS_GFX950 >= hwc.lds_bytes(N - 16)
    L, _ = _step_handle(N)
    try:
        text = np.arange(32, 56, dtype=np.uint8)
        z = np.zeros(N, np.float32)
        limit = _refused(N, lambda: L.eval_bits(text), "eval_bits")
        assert _refused(N, lambda: L.sample(z, z, np.full(4, 0.5)), "sample") == limit
        _still_usable(L, N)
        _report(dict(refused=N, lds_bytes=hwc.lds_bytes(N), limit=limit))
    finally:
        L.close()
