"""-m gpu: the per-byte gradient sums (dW, db) on the input statistics of real use, against the oracle.

Every other parity test draws its input bytes uniformly, so the code that turns the one-hot input into dW and db -- the LDS
tables inside the fused backward recurrences, k_dW_table, the sort and segment-sum passes, the group-partial folds -- only ever
met buckets of about T/256 columns.  Here each path runs on text-distributed bytes (a bucket of thousands, bytes seen once),
one repeated byte, only bytes 0 and 255, windows that are half or wholly empty, column groups sharing one byte at every step,
and buckets of exactly 0, 1, 31, 32, 33, 64 and 65 columns (input_stats_cases.py, gpu_util.window_bytes).

One window through the C ABI per case.  Reference: the float64 oracle (bf16 handles: the float32 oracle in bf16 mode).
  the project's tolerances : last h 2e-5 of scale, loss 2e-5*(S-1) bits, every gradient tensor 2e-4 of scale
                             (bf16: 2e-3, 1e-3*(S-1), 1e-2)
  per input byte           : max|dW[:, v] - ref[:, v]| <= 2e-4 * max|ref[:, v]| for every byte v that occurs (bf16: 1e-2) --
                             grads_report scales by the largest bucket's sum and so hides a lost column of a small bucket
  absent bytes             : their dW columns are bit-exactly 0
  all_empty                : loss exactly 0, dW exactly 0; db, dU, dWhy, dby still against the oracle (dy = p)
  db against dW            : db - sum_v dW[:, v] (the empty columns' share) equals the reference's within 2e-4 of max|db_ref|
  determinism              : a second backward on the same handle, profiled (everything on one stream), returns the same bits
Each case asserts the path it is on from lstm_hip_plan_identity and the profiled launch counts, and fails (not skips) with the
plan string when the device at hand plans otherwise.

Then three lock-step blocks through lstm_hip_train_windows at two shapes, four windows from reset_window (mostly empty rows):
the fold deferred into the update launch, which get_grads never sees; one block per shape with set_grad_clip(inf) (the fold in
k_grad_sumsq), its recorded norm against the oracle gradient's at 2e-4 relative.

Worst figures over the cases, on an MI355X (every case: profiles/input_statistics/parity.jsonl), beside the control's
(tests/test_input_statistics_cpu.py: the float32 oracle against the float64 oracle on the same fp32 cases):
                                  fp32 handles   float32 oracle   tolerance  |  bf16 handles   tolerance
  last h, of scale                  1.0e-6          6.4e-7          2e-5     |    6.5e-4         2e-3
  loss, bits per step               3.5e-6          3.3e-6          2e-5     |    8.1e-7         1e-3
  gradient tensor, of scale         6.8e-6          9.1e-6          2e-4     |    3.1e-3         1e-2
  dW per byte column, of scale      2.7e-6          9.1e-6          2e-4     |    3.6e-4         1e-2
  db - sum dW, of max|db|           4.7e-6          4.5e-6          2e-4     |    1.2e-5         2e-4
Absent bytes' columns, all_empty's loss and dW: exactly 0 everywhere; every second backward returned the same bits.
Lock-step blocks: loss within 6.3e-5 bits (S = 100), parameters within 3.4e-6, recorded norm within 2.3e-6 relative.
The file takes 16 s on 16 CPUs beside the GPU (103 windows and 6 blocks; the references come from worker processes).
"""
import json
import os
import time

import numpy as np
import pytest

import gpu_util as gu
import input_stats_cases as isc

pytestmark = pytest.mark.gpu

REPORT = os.environ.get("INPUT_STATISTICS_REPORT")  # a file to append one JSON line per case to (profiles/input_statistics)


def _report(rec):
    if REPORT:
        with open(REPORT, "a") as f:
            f.write(json.dumps(rec) + "\n")


@pytest.fixture(scope="module")
def references(request):
    t0 = time.time()
    cases = isc.selected_cases(request)
    pool = isc.ReferencePool(cases)
    yield pool
    pool.close()
    _report(dict(file="tests/test_input_statistics.py", wall_seconds=round(time.time() - t0, 1), cases=len(cases)))


_assert_plan = isc.assert_plan


@pytest.mark.parametrize("case", isc.CASES, ids=isc.case_id)
def test_window_with_input_statistics(case, references, monkeypatch):
    import lstm_hip
    sh = case.shape
    N, S, B, T = sh.N, sh.S, sh.B, (sh.S - 1) * sh.B
    P, xi, ti, h0, c0 = isc.inputs(case)
    flags = 0
    for f in sh.flags:
        flags |= getattr(lstm_hip, f)
    for k, v in sh.env.items():
        monkeypatch.setenv(k, v)                    # read per handle at create
    L = lstm_hip.Lstm(N, S, B, flags=flags)
    for k in sh.env:
        monkeypatch.delenv(k)
    try:
        plan = _assert_plan(L, sh.plan)
        L.set_params(P)
        L.set_state(0, h0, c0)
        L.set_window(xi, ti)
        L.forward()
        got = dict(loss=L.loss())
        got["h_last"] = L.get_state(S - 1)[0]
        L.backward()                                # as training runs it (side stream and all)
        got["grads"] = L.get_grads()
        L.set_profiling(True)                       # the same again, one timed launch after the other
        L.reset_kernel_stats()
        L.backward()
        stats = {k: v[0] for k, v in L.kernel_stats().items()}
        L.set_profiling(False)
        again = L.get_grads()
    finally:
        L.close()
    # the path, by launch counts: column-range launches of the recurrence; who summed dW and db
    rec = "bwd_step" if sh.plan["bwd"] == isc.BWD_STEP else "bwd_persistent"
    assert stats.get(rec, 0) == sh.launches, (plan, stats)
    assert stats.get("dW_db", 0) == 1, (plan, stats)
    if sh.dw == "fold":
        assert stats.get("gemm_dWhy", 0) == 0 and stats.get("gemm_DHy", 0) == 0, (plan, stats)   # inside the recurrence
    else:
        assert stats.get("gemm_dWhy", 0) == 1, (plan, stats)
        assert {"table": T <= isc.DWT_MAX_T, "rank": isc.DWT_MAX_T < T <= isc.RANK_MAX_T, "sort": T > isc.RANK_MAX_T}[sh.dw], T
    fig = None
    try:
        fig = isc.check_window(case, got, references.get(case), xi)
    finally:
        same = bool(np.array_equal(got["grads"].view(np.uint32), again.view(np.uint32)))
        _report(dict(case=isc.case_id(case), path=sh.path, plan=plan, dw=sh.dw, figures=fig, second_backward_same_bits=same))
    assert same, "the second backward on the same handle changed bits of the gradient"


# ---- lock-step blocks through the device-resident loop --------------------------------------------------------------------
def _texts(S):
    return dict(text=gu.text_bytes(6000, seed=12), one_byte=np.full(3000, gu.ONE_BYTE, np.uint8),
                wrapping=gu.text_bytes(S + 24, seed=13))


@pytest.mark.parametrize("corpus", ["text", "one_byte", "wrapping"])
@pytest.mark.parametrize("N,S,B", [(256, 20, 32), (512, 100, 64)])
def test_train_windows_from_an_empty_window_follows_the_oracle_trainer(N, S, B, corpus):
    """The form of test_hip_parity.py::test_device_resident_loop_follows_the_oracle_trainer (state re-synchronised before every
    window; loss within 2e-5*(S-1), parameters after the step within 2e-4*lr where the gradient is above noise, indices bit for
    bit), at two fused shapes, four windows from reset_window, on a text-distributed corpus, a run of one byte and a corpus
    so short that the cursors wrap.  The `wrapping` block measures the gradient norm (set_grad_clip(inf))."""
    import lstm_hip
    from oracle_lib import Oracle
    text = _texts(S)[corpus]
    lr, windows = 0.1, 4
    clip = corpus == "wrapping"
    orc = Oracle("f32_omp")
    tr = orc.trainer(text, N, S, B, lr=lr, seed=1)
    tr.epoch_reset()
    L = lstm_hip.Lstm(N, S, B)
    try:
        plan = _assert_plan(L, dict(bwd=isc.BWD_SCATTER, fused=1, gc=8 if B > 32 else 4))
        L.set_text(text)
        pos0 = lstm_hip.initial_cursors(len(text), S, B)
        L.set_cursors(pos0)
        L.reset_window()
        if clip:
            L.set_grad_clip(float("inf"))
        for w in range(windows):
            L.set_params(tr.params.copy())
            L.set_params(tr.mem.copy(), lstm_hip.P_MEM)
            L.set_state(1, tr.h[1], tr.c[1])  # column 1 becomes the carry after the slide
            got = L.train_windows(1, lr)[0]
            want = tr.window()
            xi, ti = L.get_window()
            d = np.asarray(tr.grads, np.float64)
            mask = np.abs(d) > 1e-3 * np.abs(d).max()
            p_err = float(np.abs(L.get_params()[mask] - tr.params[mask]).max())
            empty_rows = int(np.sum(np.all(xi[1:] < 0, axis=1)))
            rec = dict(block=f"{N}x{S}x{B}-{corpus}", plan=plan, window=w, empty_rows=empty_rows, loss=abs(got - want), params=p_err)
            if clip:
                norm, want_norm = float(L.grad_norms()[0]), float(np.sqrt(np.sum(d * d)))
                rec["norm_rel"] = abs(norm - want_norm) / want_norm
            print(rec)
            _report(rec)
            assert abs(got - want) <= 2e-5 * (S - 1), (w, got, want)
            assert np.array_equal(xi, tr.xi) and np.array_equal(ti, tr.ti), w
            h1, c1 = L.get_state(1)
            assert gu.max_rel(h1, tr.h[1]) <= 2e-5 and gu.max_rel(c1, tr.c[1]) <= 2e-5, w
            assert p_err <= 2e-4 * lr + 1e-6, w
            if clip:
                assert rec["norm_rel"] <= 2e-4, (w, norm, want_norm)
            assert empty_rows == S - 1 - w                      # the inputs lag the targets: window 0 has targets only
        if corpus == "wrapping":
            assert np.any(L.get_cursors().astype(np.int64) < pos0.astype(np.int64) + windows)   # a cursor went back to S
    finally:
        L.close()
