"""The reference-only control of tests/test_hidden_widths.py, and the facts of the source its table rests on.

Tolerance control: for every case of hidden_width_cases.CASES the float32 oracle -- a correct float32 implementation with
another summation order and libm -- goes through the assertions of the GPU file (hidden_width_cases.check_case) against the
float64 oracle with every tolerance cut to a quarter.  A case that could not meet this would be one whose tolerance sits inside
float32 rounding, and would need another seed or scale.
Mutation: the float32 oracle with the last 16 columns of U zeroed computes what a recurrence that dropped its final k-step
would; it must fail the same assertions, at the full tolerances, on every case.

Measured, float32 against float64 oracle, worst over the eight cases (a quarter of the tolerance beside it): h, c, g, probs
1.4e-6 of the step's scale (5e-6; h at 2048x3x3), loss 3.5e-7 bits per step (5e-6), gradients per tensor 8.3e-7 (5e-5), dW per
used byte column 1.0e-6 (5e-5), db minus the dW columns 1.3e-7 of max|db| (5e-5), the stepped parameters 3.0e-8 (5.25e-6), the
memory exact to 4e-12.  Without the last k-step: h, c and g 6.5e-2 to 2.4e-1, probs 2.9e-3 to 2.8e-2, on every case.

The device loop's two blocks and the evaluator's and sampler's inputs have the same control further down (a float32 trainer
in the device's place; the float32 oracle's evaluator and sampler, and the same without the last k-step).
"""
import os
import re

import numpy as np
import pytest

import gpu_util as gu
import hidden_width_cases as hwc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "eigen-lstm_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _body(src, head):
    """the text of the function whose definition starts with `head`, up to the closing brace in column 0"""
    at = src.index(head)
    return src[at:src.index("\n}\n", at)]


def test_step_kernels_stream_their_operands_in_chunks_of_CH():
    src = _src("kernels.hip")
    for head in ("void k_fwd_step(", "void k_bwd_step("):
        body = _body(src, head)
        assert re.findall(r"constexpr int CH = (\d+);", body) == [str(hwc.CH)], head
        assert re.search(r"const bool more = c0 \+ CH < (nk4|per);", body), head


def test_persistent_widths_match_the_plan_source():
    src = _src("persistent.hip")
    # the resolvers of the fp32 one-recurrence forms name the widths that have an instantiation, and refuse every other
    fwd_rungs = _body(src, "template <class F> static bool with_fwd_persistent(int N, bool fast, F &&f)")
    bwd_rungs = _body(src, "template <class F> static bool with_bwd_persistent(int N, int cols, bool fuse, bool stamp, bool bf16, F &&f)")
    for rungs in (fwd_rungs, bwd_rungs):
        assert tuple(int(n) for n in re.findall(r"case (\d+): return ", rungs)) == hwc.PERSISTENT_WIDTHS
        assert "default: return false;" in rungs
    body = _body(src, "static bool persistent_supported(int N, int B, int n_cus, bool fused, bool fast, bool stamp)")
    assert "if (N % 64 != 0 || N > 1024) return false;" in body
    assert "if (!with_fwd_persistent(N, fast, fwd)) return false;" in body
    assert "if (!with_bwd_persistent(N, cols, fused && cols == 8, stamp, false, bwd)) return false;" in body


def test_evaluator_and_sampler_lds_request_matches_the_source():
    src = _src("kernels.hip")
    assert "size_t b1_lds_bytes(int N) { return (size_t)(6 * N + 256) * sizeof(float); }" in src
    for head in ("hipError_t eval_bits(", "hipError_t sample("):
        assert "const size_t lds = b1_lds_bytes(N);" in _body(src, head), head
    for kernel in ("k_eval_bits", "k_sample"):
        assert "*ps = sm + 6 * N;" in _body(src, f"void {kernel}("), kernel
    assert hwc.lds_bytes(2688) == hwc.LDS_UNASKED < hwc.lds_bytes(2704)
    assert hwc.lds_bytes(hwc.N_PAST_LDS - 16) <= hwc.LDS_GFX950 < hwc.lds_bytes(hwc.N_PAST_LDS)
    # both launches are checked, and refused with the width before anything is allocated
    api = _src("lstm_hip_api.cpp")
    for call in ("eval_bits", "sample"):
        assert f'b1_lds_check(h, "{call}")' in api and f'b1_status("{call}", {call}(h->P, N,' in api, call


def test_table_reaches_what_it_says():
    shapes = {(sh.N, sh.S, sh.B): sh for sh in hwc.SHAPES}
    assert len(shapes) == len(hwc.SHAPES) == len({hwc.case_id(c) for c in hwc.CASES}) == 8
    for sh in hwc.SHAPES:
        Np = hwc.internal_width(sh)
        assert Np % 16 == 0 and Np == -(-sh.N // 16) * 16 and ("PAD_HIDDEN" in sh.flags) == (Np != sh.N), sh
        assert sh.plan["fwd"] == hwc.FWD_STEP and sh.plan["bwd"] == hwc.BWD_STEP
        assert sh.S > 2                                              # every case has its empty column
    ks = {hwc.internal_width(sh): hwc.k_steps(sh) for sh in hwc.SHAPES}
    assert (ks[80], ks[192], ks[320], ks[1040], ks[2048]) == (5, 12, 20, 65, 128)
    # a partial last chunk after a full one, with one, two and eight full chunks before it; and only full chunks, many
    assert [(k // hwc.CH, k % hwc.CH) for k in (ks[192], ks[320], ks[1040], ks[2048])] == [(1, 4), (2, 4), (8, 1), (16, 0)]
    off = [sh.N for sh in hwc.SHAPES if hwc.internal_width(sh) not in hwc.PERSISTENT_WIDTHS]
    assert sorted(off) == [30, 80, 192, 320, 1030, 1040, 2048]      # (1024 is on the list: its grid is what does not fit)
    assert (59 - 1) // 16 * 16 + 11 == 59 and (10 - 1) * 59 == 531 and 17 == 16 + 1
    # evaluator and sampler: b1_step's row loop passes 1024 rows at 320, its unit loop 1024 units at 1040
    assert [a.N for a in hwc.EVAL] == [192, 320, 1040, 2688, 2704] and [a.N for a in hwc.SAMPLE] == [192, 1040, 2704]
    assert 4 * 192 <= 1024 < 4 * 320 and 320 <= 1024 < 1040
    assert all(a.count == (24 if a.N > 1040 else 300) for a in hwc.EVAL)
    assert [(a.count, a.scale) for a in hwc.SAMPLE] == [(200, 0.1), (200, 0.05), (8, 0.05)]
    assert [a.scale for a in hwc.EVAL] == [0.1, 0.1, 0.05, 0.05, 0.05]


def test_dropping_the_last_k_step_zeroes_the_last_sixteen_columns_of_U():
    from oracle_lib import split_params
    N = 48
    P = gu.random_case(N, 2, 1, seed=1)[0]
    Q = hwc.drop_last_k_step(P, N)
    p, q = split_params(P, N), split_params(Q, N)
    assert not q["U"][:, N - 16:].any() and np.array_equal(q["U"][:, :N - 16], p["U"][:, :N - 16]) and p["U"][:, N - 16:].all()
    assert all(np.array_equal(p[k], q[k]) for k in p if k != "U")


@pytest.fixture(scope="module")
def controls(request):
    pool = hwc.ReferencePool(hwc.selected_cases(request), "control", fn=hwc.reference, key=hwc.case_id)
    yield pool
    pool.close()


@pytest.mark.parametrize("case", hwc.CASES, ids=hwc.case_id)
def test_float32_oracle_meets_a_quarter_and_the_mutation_fails(case, controls):
    out = controls.get(case)            # (a float32 oracle outside a quarter of a tolerance raises from check_case here)
    print(hwc.case_id(case), "float32 oracle:", " ".join(f"{k}={v:.2e}" if isinstance(v, float) else f"{k}={v}" for k, v in out["fig"].items()))
    print(hwc.case_id(case), "without the last k-step:", out["mutant_act"], "->", out["mutant"])
    assert out["mutant"] is not None, "a window without the last k-step of U passes every check of the case"
    # ... and by the recurrence itself, at the first thing it changes: the gates of some step
    assert out["mutant_act"]["g"] > hwc.TOL_FP32["h"], out["mutant_act"]


# The evaluator's cases at 2688 and 2704 take the serial oracle 3 to 6 s each and stay out of this file; measured once, 24
# bytes: float32 against float64 oracle 2.1e-7 and 1.8e-7 bits per character, without the last k-step 2.1e-2 and 2.1e-3.
AUX = [a for a in hwc.EVAL if a.N <= 1040] + hwc.SAMPLE


@pytest.fixture(scope="module")
def aux_controls(request):
    cases = [it.callspec.params["aux"] for it in request.session.items
             if it.module is request.module and "aux" in getattr(getattr(it, "callspec", None), "params", {})]
    pool = hwc.ReferencePool(cases, fn=hwc.aux_control, key=hwc.any_id)
    yield pool
    pool.close()


@pytest.mark.parametrize("aux", AUX, ids=hwc.any_id)
def test_evaluator_and_sampler_inputs_tell_a_lost_k_step_from_rounding(aux, aux_controls):
    """The inputs of the GPU file's evaluator and sampler tests: the float32 oracle is within a quarter of the evaluator's
    tolerance of the float64 oracle, and draws every byte the float64 oracle draws; without the last k-step of U it misses
    the evaluator's tolerance, and the sampler's 99 %."""
    w32, w64, mut = aux_controls.get(aux)
    if aux.kind == "eval":
        print(hwc.any_id(aux), f"bits {w64:.6f} float32 {abs(w32 - w64):.2e} without the last k-step {abs(mut - w64):.2e}")
        assert abs(w32 - w64) <= 0.25 * hwc.EVAL_TOL and abs(mut - w64) > hwc.EVAL_TOL
    else:
        print(hwc.any_id(aux), "float32", (w32[0] == w64[0]).mean(), "without the last k-step", (mut[0] == w64[0]).mean())
        assert np.array_equal(w32[0], w64[0]) and gu.max_rel(w32[1], w64[1]) <= 0.25 * 1e-3 and gu.max_rel(w32[2], w64[2]) <= 0.25 * 1e-3
        assert (mut[0] == w64[0]).mean() < 0.99


def _trainers_in_lock_step(N, S, B, windows, lr):
    """The float32 oracle's trainer in the place of the device in test_hip_parity.py's device-loop check: before every window
    the float64 trainer takes its parameters, memory and carry.  Returns the largest distances: (loss, carry, parameters)."""
    from oracle_lib import Oracle
    from test_hip_parity import _synthetic_text
    text = _synthetic_text(S + 24)
    a, b = (Oracle(k).trainer(text, N, S, B, lr=lr, seed=1) for k in ("f32", "f64"))
    a.epoch_reset(), b.epoch_reset()
    worst = np.zeros(3)
    for _ in range(windows):
        b.params[:], b.mem[:], b.h[1][:], b.c[1][:] = a.params, a.mem, a.h[1], a.c[1]
        loss_b, loss_a = b.window(), a.window()
        assert np.array_equal(a.xi, b.xi) and np.array_equal(a.ti, b.ti)
        d = np.asarray(b.grads)
        mask = np.abs(d) > 1e-3 * np.abs(d).max()
        worst = np.maximum(worst, [abs(loss_a - loss_b), max(gu.max_rel(a.h[1], b.h[1]), gu.max_rel(a.c[1], b.c[1])),
                                   np.abs(a.params[mask] - b.params[mask]).max()])
    return worst


@pytest.mark.parametrize("N,S,B,windows,lr", hwc.LOOPS)
def test_float32_trainer_meets_a_quarter_of_the_device_loop_bounds(N, S, B, windows, lr):
    loss, carry, params = _trainers_in_lock_step(N, S, B, windows, lr)
    print(f"{N}x{S}x{B} lr {lr}: loss {loss:.2e} carry {carry:.2e} parameters {params:.2e} of {2e-4 * lr + 1e-6:.2e}")
    assert loss <= 0.25 * 2e-5 * (S - 1) and carry <= 0.25 * 2e-5 and params <= 0.25 * (2e-4 * lr + 1e-6)


def test_hidden_1040_at_learning_rate_one_tenth_is_inside_float32_rounding():
    """why hidden_width_cases.LOOPS runs hidden 1040 at 0.01: at 0.1 the float32 oracle itself is not within the bound"""
    N, S, B, windows, _ = hwc.LOOPS[1]
    assert N == 1040
    assert _trainers_in_lock_step(N, S, B, windows, 0.1)[2] > 2e-4 * 0.1 + 1e-6
