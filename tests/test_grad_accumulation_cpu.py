"""CPU: gradient accumulation (lstm_hip_set_grad_accumulation) without a device.

The comparison that tests/test_grad_accumulation.py makes against the oracle (grad_accum_ref.accumulators_agree, with the
tolerance that module derives from tests/test_hip_parity.py's GRAD_TOL) is run here on the oracle alone: the float64
oracle under the right rule is the reference, the float32 oracle stands in for the handle.  Under the right rule it must
agree; under each of three wrong rules -- the first window of a cycle dropped, an update at every window, the mean applied
when not asked -- it must not.  Then the boundary: the header declares the four calls, lstm_hip.py binds them, and the API
file refuses where the header says it does."""
import inspect
import os

import numpy as np
import pytest

import grad_accum_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lstm_hip_set_grad_accumulation", "lstm_hip_get_grad_accumulation", "lstm_hip_get_grad_accumulator",
         "lstm_hip_set_grad_accumulator")
N, S, B, EVERY, WINDOWS, STRIDE, CARRY, LR = 8, 6, 3, 3, 7, 2, 1, 0.05


@pytest.fixture(scope="module")
def case():
    rs = np.random.RandomState(11)
    text = rs.randint(32, 127, size=400).astype(np.uint8)
    pos = np.array([S + 37 * b for b in range(B)], np.uint64)
    xi, ti = np.full((S, B), -1, np.int32), np.full((S, B), -1, np.int32)
    ref.host_slide(xi, ti, pos, text, S, S)
    windows = []
    for _ in range(WINDOWS):
        ref.host_slide(xi, ti, pos, text, S, STRIDE)
        windows.append((xi.copy(), ti.copy()))
    n = 4 * N * 256 + 4 * N * N + 4 * N + 256 * N + 256
    P0 = (rs.randn(n) * 0.08).astype(np.float32)
    h0, c0 = (rs.randn(B, N) * 0.1).astype(np.float32), (rs.randn(B, N) * 0.1).astype(np.float32)
    return P0, windows, h0, c0


@pytest.fixture(scope="module")
def reference(case, oracle64):
    P0, windows, h0, c0 = case
    return ref.run_rule(oracle64, "right", N, S, B, P0, windows, h0, c0, CARRY, EVERY, False, LR)


def test_the_right_rule_agrees_with_the_reference(case, reference, oracle32):
    P0, windows, h0, c0 = case
    rec, _, updates = ref.run_rule(oracle32, "right", N, S, B, P0, windows, h0, c0, CARRY, EVERY, False, LR)
    ok, worst = ref.accumulators_agree(rec, reference[0], N)
    print("worst error / tolerance under the right rule:", worst)
    assert ok, worst
    assert updates == reference[2] == WINDOWS // EVERY
    assert [r[1] for r in rec] == [1, 2, 0, 1, 2, 0, 1]
    # the tolerance is a few GRAD_TOL, not a licence: the windows of a cycle do not cancel at this shape
    tol = ref.accum_tolerance([r[2] for r in reference[0][:EVERY]], N)
    assert max(tol.values()) <= 10 * ref.GRAD_TOL, tol


@pytest.mark.parametrize("rule", [r for r in ref.RULES if r != "right"])
def test_a_wrong_rule_does_not(case, reference, oracle32, rule):
    P0, windows, h0, c0 = case
    rec, _, _ = ref.run_rule(oracle32, rule, N, S, B, P0, windows, h0, c0, CARRY, EVERY, False, LR)
    ok, worst = ref.accumulators_agree(rec, reference[0], N)
    print(rule, "worst error / tolerance:", worst)
    assert not ok, (rule, worst)


def test_entry_points_are_declared_and_bound():
    import lstm_hip
    header = open(os.path.join(ROOT, "include", "lstm_hip.h")).read()
    for line in ("int lstm_hip_set_grad_accumulation(lstm_hip_t *h, int32_t every, int32_t mean);",
                 "int lstm_hip_get_grad_accumulation(lstm_hip_t *h, int32_t *every, int32_t *mean, int32_t *pending);",
                 "int lstm_hip_get_grad_accumulator(lstm_hip_t *h, float *host_block);",
                 "int lstm_hip_set_grad_accumulator(lstm_hip_t *h, const float *host_block, int32_t pending);"):
        assert line in header, line
    assert set(NAMES) <= set(lstm_hip.SYMBOLS)
    sig = {name: str(inspect.signature(getattr(lstm_hip.Lstm, name)))
           for name in ("set_grad_accumulation", "grad_accumulation", "grad_accumulator", "set_grad_accumulator")}
    assert sig == {"set_grad_accumulation": "(self, every, mean=False)", "grad_accumulation": "(self)",
                   "grad_accumulator": "(self)", "set_grad_accumulator": "(self, block, pending)"}, sig
    lib = lstm_hip.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name


def _body(src, signature):
    """the text of the function that starts with `signature`, up to the closing brace in column 0"""
    i = src.index(signature)
    return src[i:src.index("\n}\n", i)]


def test_the_api_file_refuses_the_communicator_and_the_adaptive_coders():
    api = open(os.path.join(ROOT, "eigen-lstm_amd", "csrc", "lstm_hip_api.cpp")).read()
    setter = _body(api, "int lstm_hip_set_grad_accumulation(lstm_hip_t *h, int32_t every, int32_t mean) {")
    assert 'if (every > 1 && h->comm)' in setter
    assert 'LSTM_HIP_ESTATE, "set_grad_accumulation: a handle with a communicator cannot accumulate gradients"' in setter
    assert setter.index("h->comm") < setter.index("h->own.alloc(")  # refused before anything is allocated or changed
    comm = _body(api, "int lstm_hip_comm_init(lstm_hip_t *h, const uint8_t id[LSTM_HIP_UNIQUE_ID_BYTES], int32_t nranks, int32_t rank) {")
    assert ('LSTM_HIP_ESTATE, "comm_init: gradient accumulation is on (lstm_hip_set_grad_accumulation); it runs on one device"'
            in comm)
    assert comm.index("h->acc_every > 1") < comm.index("rccl_load()")  # before the library is loaded or a communicator made
    adaptive = _body(api, "static int adaptive_checks(lstm_hip_t *h, const char *what, double lr) {")
    assert "h->acc_every > 1" in adaptive
    assert ('"%s: gradient accumulation is on (lstm_hip_set_grad_accumulation); the adaptive coders update after every block"'
            in adaptive)
    # the statistics row sits behind the rows the earlier features added, with its name in the second table
    assert "K_SOFTMAX_WEIGHTED," in api and api.index("K_SOFTMAX_WEIGHTED,") < api.index("K_GRAD_ACCUMULATE,") < api.index("K_COUNT\n")
    assert '{"softmax_soft", "softmax_loss_dy_weighted", "grad_accumulate"}' in api
