"""-m gpu: the training window on the parameter statistics of a trained model, every pair of recurrence forms, against the oracle.

Every other parity test of the window draws its parameters from one Gaussian of scale 0.02-0.08 and a state of scale 0.1: all
gates about 0.5, tanh linear, the softmax flat at 1/256.  Here each pair of forms of csrc/kernels.h runs with saturated gates
(a quarter of the sigmoid gates outside (0.01, 0.99)), the reference's trained weights tiled to the width at hand on their own
held-out text (p(target) from 4e-4 to 0.99), per-unit scales over two and a half orders of magnitude, a carried state with
|c0| up to 0.999 and weights of order 1-10 (param_stats_cases.py, gpu_util.regime_params).

One window through the C ABI per case.  Reference: the float64 oracle (bf16 handles: the float32 oracle in bf16 mode).
  every step               : h, c, g, probs at every t, each of its step's scale (2e-5; bf16 2e-3; LSTM_HIP_FAST_MATH 1e-4)
  at the extremes          : element-wise, relative: sigmoid gates below 0.01; 1 - g of gates above 0.99 and 1 - |c| of cells
                             above 0.9 (both against a floor of 2^-14); p(target).  Bounds: param_stats_cases.EXTREME
  loss                     : 2e-5 * (S-1) bits (bf16 1e-3, fast math 1e-4)
  gradients                : per tensor, and every row of dW and dU and every column of dWhy of its own scale (2e-4; bf16 1e-2)
  tiled cases              : the k diagonal blocks of dU agree, the k row-copies of dW agree (the gradient tolerance)
  update (`every` rows)    : Adagrad from a memory of the gradient's size: p within 2e-4 * lr, m within 1e-3; then forward and
                             loss again on the rewritten weight images: last h and loss against the oracle's
  determinism              : a second backward returns the same bits
A bf16 bound is max(TOL_BF16, 4 x the case's distance between the bf16-mode oracle summed in ascending and in descending
order), at most 5 x TOL_BF16.  Each case asserts its forms from lstm_hip_plan_identity and fails (not skips) otherwise.

Then the known answers at every width: fixture A's logged 3.24396 and B's 2.75851 bits/char, tiled to hidden 64-1024, through
lstm_hip_eval_bits, the prompt bits of lstm_hip_generate and forward + loss chained through the carry, each within 1e-4.

Worst figures over the cases, on an MI355X (every case: profiles/param_statistics/parity.jsonl), beside the control's
(tests/test_param_statistics_cpu.py: the float32 oracle against the float64 oracle on the fp32 inputs):
                                      fp32 handles  float32 oracle   bound   |  bf16 handles  between the orders  bound
  h, c, g, probs, worst step, of scale   1.6e-6        4.7e-6        2e-5    |    2.2e-3          2.2e-3        2e-3 .. 8.9e-3
  sigmoid gates below 0.01, relative     4.5e-6        7.4e-6        3.0e-5  |    3.0e-3          2.5e-3        2e-3 .. 1.0e-2
  1 - g above 0.99, floor 2^-14          1.04e-3       1.04e-3       4.4e-3  |    3.0e-3          3.3e-3        2e-3 .. 1.3e-2
  1 - |c| above 0.9, floor 2^-14         3.2e-6        3.8e-6        1.6e-5  |    1.8e-3          2.0e-3        2e-3 .. 8.2e-3
  p(target), relative                    5.4e-6        1.5e-5        6.4e-5  |    4.1e-3          2.6e-3        2e-3 .. 1.1e-2
  loss, bits per step                    2.6e-6        1.5e-6        2e-5    |    1.6e-5          2.1e-5        1e-3
  gradient tensor, of scale              1.4e-6        4.0e-6        2e-4    |    1.4e-3          1.1e-3        1e-2
  row of dW, dU / column of dWhy         4.9e-5        3.0e-5        2e-4    |    6.7e-3          5.4e-3        1e-2 .. 2.2e-2
  tiled: blocks of dU, copies of dW      1.7e-7          0           2e-4    |      0               0           1e-2
  update: p, of lr                       2.7e-7        1.5e-6        2e-4    |    2.1e-4          1.9e-4        1e-2
  update: m (beyond 1e-3 relative)         0             0           1e-3    |      0               0           1e-3
  after the update: last h / loss        5.4e-7/7.7e-7 1.9e-6/5.4e-7 2e-5    |  2.2e-3/2.5e-5   1.9e-3/3.8e-5   2e-3 .. 7.6e-3 / 1e-3
(1 - g: the float32 spacing of g against the floor, the same in every saturated case; the largest bf16 bound used is 4.5 x its
TOL_BF16 value, g at 512x12x64 saturated.)  LSTM_HIP_FAST_MATH: h, c, g, probs within 9.3e-7, loss within 4.4e-7 bits per
step (1e-4).  Every second backward returned the same bits.  The known answers, hidden 64 ... 1024: 3.243898 ... 3.243899
(logged 3.24396) and 2.758511 (2.75851) through all three entry points; the bf16 handle's bits equal the fp32 handle's.
The file takes 14 s on 16 CPUs beside the GPU (56 windows, 9 known answers; the references come from worker processes).
"""
import json
import os
import time

import numpy as np
import pytest

import gpu_util as gu
import param_stats_cases as psc

pytestmark = pytest.mark.gpu

REPORT = os.environ.get("PARAM_STATISTICS_REPORT")  # a file to append one JSON line per case to (profiles/param_statistics)


def _report(rec):
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(json.dumps(rec) + "\n")


@pytest.fixture(scope="module")
def references(request):
    t0 = time.time()
    cases = psc.selected_cases(request)
    pool = psc.reference_pool(cases, True)
    yield pool
    pool.close()
    _report(dict(file="tests/test_param_statistics.py", wall_seconds=round(time.time() - t0, 1), cases=len(cases)))


def _window(L, S):
    """forward, loss and every step's activations: dict(h, c, g, probs: [S-1, B, rows], loss)"""
    L.forward()
    out = dict(loss=L.loss())
    steps = [L.get_state(t) + L.get_activations(t) for t in range(1, S)]
    for i, k in enumerate(("h", "c", "g", "probs")):
        out[k] = np.stack([s[i] for s in steps])
    return out


@pytest.mark.parametrize("case", psc.CASES, ids=psc.case_id)
def test_window_with_parameter_statistics(case, references, monkeypatch):
    import lstm_hip
    t0 = time.time()
    sh = case.shape
    N, S, B = sh.N, sh.S, sh.B
    P, xi, ti, h0, c0 = psc.inputs(case)
    flags = 0
    for f in sh.flags:
        flags |= getattr(lstm_hip, f)
    for k, v in sh.env.items():
        monkeypatch.setenv(k, v)                    # read per handle at create
    L = lstm_hip.Lstm(N, S, B, flags=flags)
    for k in sh.env:
        monkeypatch.delenv(k)
    r = references.get(case)
    try:
        plan = psc.assert_plan(L, sh.plan)
        L.set_params(P)
        L.set_state(0, h0, c0)
        L.set_window(xi, ti)
        got = _window(L, S)
        L.backward()
        got["grads"] = L.get_grads()
        L.backward()
        again = L.get_grads()
        upd = None
        if psc.has_update(case):
            L.set_params(r["mem0"], lstm_hip.P_MEM)
            L.adagrad(psc.UPDATE_LR)
            upd = dict(p=L.get_params(), m=L.get_params(lstm_hip.P_MEM))
            L.forward()                             # the weight images the update launch rewrote, through the recurrence
            upd["loss"] = L.loss()
            upd["h_last"] = L.get_state(S - 1)[0]
    except lstm_hip.LstmHipError as e:              # nothing more is started on a device that reported an error
        pytest.exit(f"{psc.case_id(case)}: {e}", returncode=3)
    finally:
        L.close()
    fig = psc.figures(case, got, r["ref"], ti)
    if upd is not None:
        fig.update(psc.update_figures(upd, r["upd"]))
    same = bool(np.array_equal(got["grads"].view(np.uint32), again.view(np.uint32)))
    tol = None
    try:
        if r["control"] is not None and not psc.fast_math(case):       # (also where the reference-only control does not run)
            psc.check_window(case, r["control"], fraction=0.25)
        assert psc.has_update(case) == (upd is not None)
        tol = psc.check_window(case, fig, dist=r["dist"], dist_ulp=r["dist_ulp"])
    finally:
        _report(dict(case=psc.case_id(case), forms=sh.forms, plan=plan, figures=fig, control=r["control"], bf16_distance=r["dist"],
                     bf16_one_spacing_distance=r["dist_ulp"],
                     tolerance=tol, second_backward_same_bits=same, seconds=round(time.time() - t0, 2)))
    assert same, "the second backward on the same handle changed bits of the gradient"


# ---- the known answers at every width ---------------------------------------------------------------------------------------
KNOWN = [("A", 64, ()), ("A", 128, ()), ("A", 256, ()), ("A", 512, ()), ("A", 1024, ()), ("B", 128, ()), ("B", 512, ()),
         ("A", 96, ("PAD_HIDDEN",))]    # 3 x 32 units, run at the padded width 128


def _flags(lstm_hip, names):
    flags = 0
    for f in names:
        flags |= getattr(lstm_hip, f)
    return flags


def _prompt_bits(L, text):
    """the text as one stream of four, as tests/test_generate.py::test_known_answer_fixture_as_one_stream_of_four"""
    rs = np.random.RandomState(31)
    others = [rs.randint(32, 127, size=n).astype(np.uint8) for n in (500, 0, 1500)]
    _, bits, _, _ = L.generate([others[0], others[1], text, others[2]], score=True)
    return bits[2] / (text.size - 1)


@pytest.mark.parametrize("name,N,flags", KNOWN, ids=[f"{n}-{w}" + "".join("-" + f.lower() for f in fl) for n, w, fl in KNOWN])
def test_tiled_fixture_reproduces_the_logged_bits(name, N, flags):
    """The reference's logged bits/char of its saved weights is a known answer at every width the weights tile to: through
    lstm_hip_eval_bits, the prompt bits of lstm_hip_generate (four streams), and forward + loss on windows chained through
    the carry (S = 26), each within the 1e-4 of the hidden-32 / hidden-16 tests."""
    import lstm_hip
    from test_oracle_pinning import chained_windows_bits
    fx = gu.fixture(name)
    P = gu.tile_params(fx["params"], fx["N"], N // fx["N"])
    text, want, S = fx["text"], fx["bits"], 26
    got = {}
    L = lstm_hip.Lstm(N, S, 1, flags=_flags(lstm_hip, flags))
    try:
        L.set_params(P)
        got["eval_bits"] = L.eval_bits(text)
        got["generate"] = _prompt_bits(L, text)

        def fwd(xi, ti, h0, c0, steps):
            L.set_state(0, h0, c0)
            L.set_window(xi, ti)
            L.forward()
            bits = L.loss()
            h, c = L.get_state(steps)
            return bits, h, c

        got["windows"] = chained_windows_bits(fwd, N, text, S)
    finally:
        L.close()
    _report(dict(known_answer=f"{name}-{N}", flags=list(flags), logged=want, **got))
    print(name, N, flags, want, got)
    for k, v in got.items():
        assert abs(v - want) <= 1e-4, (k, v, want)


def test_tiled_fixture_through_a_bf16_handle_equals_the_fp32_handle():
    """include/lstm_hip.h: lstm_hip_eval_bits and lstm_hip_generate read only the fp32 parameters, so a handle with
    LSTM_HIP_BF16_RECURRENCE returns the fp32 handle's bits -- and with them the logged answer."""
    import lstm_hip
    fx = gu.fixture("A")
    N = 256
    P = gu.tile_params(fx["params"], fx["N"], N // fx["N"])
    got = {}
    for flags in (0, lstm_hip.BF16_RECURRENCE):
        L = lstm_hip.Lstm(N, 4, 8, flags=flags)
        try:
            L.set_params(P)
            got[flags] = (L.eval_bits(fx["text"]), _prompt_bits(L, fx["text"]))
        finally:
            L.close()
    assert got[0] == got[lstm_hip.BF16_RECURRENCE], got
    assert abs(got[0][0] - fx["bits"]) <= 1e-4 and abs(got[0][1] - fx["bits"]) <= 1e-4, got
