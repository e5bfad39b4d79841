"""-m gpu: the two-half forward and the scatter backward give the bits they gave before their chains were rescheduled.

The instruction sequences between "data is there" and "result published" of k_fwd_persistent6 and k_bwd_scatter
(csrc/persistent.hip) were shortened without changing a sum's association, a protocol or a layout, so
every result must be the bits of the commit before.  Those bits are the fixture tests/golden/chain_schedule_bits.jsonl.

test_bits_of_the_recorded_library
  A case is what tools/ab_windows.py::run_case does: one forward / loss / backward through the step API, then three
  train_windows; digests of the gradients, the parameters and the Adagrad memory, and the losses as hex floats.
    N      256, 512
    S      2 (a single step), 3, 4 (the t == 2 and t == S - 2 placement checks), 5, 9 (the four-slot rings wrap)
    B      1, 4 (one half per workgroup), 5 (a ragged second half), 8, 9 (a padded group), 64 (a full launch),
           136 (several launches over column ranges; at S = 5 only)
    flags  0, LSTM_HIP_FAST_MATH, LSTM_HIP_NO_FUSED_GRADS
  Each fixture line keeps the handle's plan string; a case whose plan string differs fails and says so (the bits of another
  kernel are not comparable).

test_two_windows_equal_the_first_replayed_on_a_fresh_handle
  The backward's readiness test must see every slot the launch before left behind: two windows on one handle against the
  same two windows where the second runs on a fresh handle loaded with the first's state, N = 512, B = 8, S = 6 and 7 (the
  ring positions differ between the launches), from the saturated-gate parameters and the carried state of
  tests/test_param_statistics.py's regime, so that large, negative and denormal partial sums cross the ring.

Re-recording, after a change that alters a sum on purpose: build the library of the commit to record from, then
    LSTM_HIP_LIB=/path/to/that/liblstm_hip.so python tests/test_chain_schedule.py --record tests/golden/chain_schedule_bits.jsonl
on an MI355X, and say in the commit which sum changed.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "chain_schedule_bits.jsonl")
FAST, UNFUSED = 1, 64  # LSTM_HIP_FAST_MATH, LSTM_HIP_NO_FUSED_GRADS


def cases():
    out = []
    for N in (256, 512):
        for S in (2, 3, 4, 5, 9):
            for B in (1, 4, 5, 8, 9, 64) + ((136,) if S == 5 else ()):
                for flags in (0, FAST, UNFUSED):
                    out.append((N, S, B, flags))
    return out


CASES = cases()


def case_id(c):
    return "%dx%dx%d-f%d" % c


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:32]


def run_case(lstm_hip, N, S, B, flags):
    L = lstm_hip.Lstm(N, S, B, flags=flags)
    try:
        rs = np.random.RandomState(1000 * N + 10 * B + S)
        L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(N + B), N))
        L.set_state(0, (rs.randn(B, N) * 0.1).astype(np.float32), (rs.randn(B, N) * 0.1).astype(np.float32))
        L.set_window(rs.randint(0, 256, size=(S, B)), rs.randint(0, 256, size=(S, B)))
        L.forward()
        loss = L.loss()
        L.backward()
        rec = {"case": case_id((N, S, B, flags)), "plan": L.plan_identity(), "step_loss": float(loss).hex(),
               "step_grads": digest(L.get_grads())}
        text = rs.randint(0, 256, size=4096).astype(np.uint8)
        L.set_text(text)
        L.set_cursors(lstm_hip.initial_cursors(len(text), S, B))
        rec["losses"] = [float(x).hex() for x in L.train_windows(3, 0.05)]
        rec["grads"] = digest(L.get_grads())
        rec["params"] = digest(L.get_params())
        rec["memory"] = digest(L.get_params(lstm_hip.P_MEM))
    finally:
        L.close()
    return rec


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        recs = [json.loads(line) for line in f if line.strip()]
    return {r["case"]: r for r in recs}


def test_fixture_lists_every_case(recorded):
    assert sorted(recorded) == sorted(case_id(c) for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_bits_of_the_recorded_library(case, recorded):
    import lstm_hip
    want = recorded[case_id(case)]
    try:
        got = run_case(lstm_hip, *case)
    except lstm_hip.LstmHipError as e:  # nothing more is started on a device that reported an error
        pytest.exit(f"{case_id(case)}: {e}", returncode=3)
    assert got["plan"] == want["plan"], (f"{case_id(case)}: the handle's plan is '{got['plan']}', the fixture was recorded under "
                                         f"'{want['plan']}': the bits of different kernels are not comparable")
    differ = [k for k in want if got[k] != want[k]]
    assert not differ, f"{case_id(case)}: {differ} differ from the recorded bits: {[(got[k], want[k]) for k in differ]}"


# ---- the readiness test sees what the launch before left in the ring ---------------------------------------------------------
def _saturated(N, S, B):
    import gpu_util as gu
    seed = N + 3 * S + 7 * B
    P = gu.regime_params("saturated", N, seed)
    xi, ti = gu.window_bytes("text", S, B, seed, "uniform")
    h0, c0 = gu.regime_state("carried", N, B, seed)
    return P, xi, ti, h0, c0


def _window(L, S):
    L.forward()
    out = {"loss": np.array([L.loss()])}
    L.backward()
    out["grads"] = L.get_grads()
    hs, cs = zip(*(L.get_state(t) for t in range(S)))
    out["h"], out["c"] = np.stack(hs), np.stack(cs)
    return out


@pytest.mark.parametrize("S", (6, 7))
def test_two_windows_equal_the_first_replayed_on_a_fresh_handle(S):
    import lstm_hip
    import param_stats_cases as psc
    N, B = 512, 8
    P, xi, ti, h0, c0 = _saturated(N, S, B)
    rs = np.random.RandomState(S)
    xi2, ti2 = rs.randint(0, 256, size=(S, B)), rs.randint(0, 256, size=(S, B))

    def load(L, x, t, h, c):
        L.set_params(P)
        L.set_state(0, h, c)
        L.set_window(x, t)

    try:
        A = lstm_hip.Lstm(N, S, B)
        try:
            psc.assert_plan(A, dict(fwd=psc.FWD_TWO_HALF, bwd=psc.BWD_SCATTER))
            load(A, xi, ti, h0, c0)
            a1 = _window(A, S)
            hc, cc = A.get_state(S - 1)
            load(A, xi2, ti2, hc, cc)     # second window on the same handle: the rings are where the first left them
            a2 = _window(A, S)
        finally:
            A.close()
        F = lstm_hip.Lstm(N, S, B)        # a fresh handle replays the first window
        try:
            load(F, xi, ti, h0, c0)
            f1 = _window(F, S)
        finally:
            F.close()
        G = lstm_hip.Lstm(N, S, B)        # and another the second, from ring position zero
        try:
            load(G, xi2, ti2, hc, cc)
            g2 = _window(G, S)
        finally:
            G.close()
    except lstm_hip.LstmHipError as e:
        pytest.exit(f"S={S}: {e}", returncode=3)
    # The second pair carries the weight: A's second window starts where its first left the rings, G's at ring position
    # zero.  The first pair starts both at zero and can only show a run-to-run difference.
    for name, x, y in (("first window", a1, f1), ("second window", a2, g2)):
        for k in x:
            assert x[k].tobytes() == y[k].tobytes(), f"S={S}, {name}: '{k}' differs between the long-lived and the fresh handle"
    # the regime does what it is here for: saturated gates, and partial sums of both signs reach the ring
    assert np.isfinite(a1["grads"]).all() and np.isfinite(a2["grads"]).all()
    assert (np.abs(a1["c"][1:]) > 0.9).mean() > 0.01


def _record(path):
    sys.path.insert(0, os.path.join(ROOT, "eigen-lstm_amd"))
    import lstm_hip
    with open(path, "w") as f:
        for c in CASES:
            f.write(json.dumps(run_case(lstm_hip, *c), sort_keys=True) + "\n")
            f.flush()
    print(f"{len(CASES)} cases recorded from {lstm_hip.LIB_PATH}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--record":
        _record(sys.argv[2])
    else:
        sys.exit(__doc__)
