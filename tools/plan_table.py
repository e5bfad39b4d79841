"""The engine plan of every shape class, as lstm_hip_plan_identity() prints it (or the text of the create's refusal).

plan_engine (csrc/persistent.hip) decides at create which form of each recurrence a handle runs.  This table pins those
decisions: tests/golden/plan_table.json was written on an MI355X by the library of the commit before the recurrence launchers
and the occupancy questions came to share one resolver per kernel, and tests/test_plan_table.py holds every later library
to it.  A plan depends on the device's CU count, so the table holds for the MI355X only.

  python tools/plan_table.py OUT.json        (LSTM_HIP_LIB selects another build of the library)
"""
import contextlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "eigen-lstm_amd"))
import lstm_hip  # noqa: E402

S = 3
HIDDEN = (64, 128, 192, 256, 512, 768, 1024, 1088)
STREAMS = (1, 3, 8, 16, 64, 72, 136, 520)
FLAGS = (0, lstm_hip.FAST_MATH, lstm_hip.STEP_KERNELS, lstm_hip.DEBUG_STAMPS, lstm_hip.NO_FUSED_GRADS, lstm_hip.BF16_RECURRENCE,
         lstm_hip.BF16_RECURRENCE | lstm_hip.FAST_MATH)
HALVES = ((0, 0), (0, 1), (1, 0), (1, 1))  # LSTM_HIP_FWD_HALVES, LSTM_HIP_BWD_HALVES at N = 256 / 512 / 1024, B = 16
SWITCHES = ("LSTM_HIP_FWD_HALVES", "LSTM_HIP_BWD_HALVES")


def cases():
    """(key, N, B, flags, {switch: value}) in a fixed order; the key names the case in the JSON."""
    for N in HIDDEN:
        for B in STREAMS:
            for flags in FLAGS:
                yield f"N{N} B{B} flags{flags}", N, B, flags, {}
    for N in (256, 512, 1024):
        for flags in FLAGS:
            for fh, bh in HALVES:
                yield f"N{N} B16 flags{flags} fwd_halves{fh} bwd_halves{bh}", N, 16, flags, dict(zip(SWITCHES, (str(fh), str(bh))))


@contextlib.contextmanager
def environment(values):
    """The switches are read at create, per handle."""
    saved = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def plan_of(N, B, flags, env):
    with environment(env):
        try:
            L = lstm_hip.Lstm(N, S, B, flags=flags)
        except lstm_hip.LstmHipError as e:
            return f"refused: {e}"
        try:
            return L.plan_identity()
        finally:
            L.close()


def table():
    return {key: plan_of(N, B, flags, env) for key, N, B, flags, env in cases()}


if __name__ == "__main__":
    t = table()
    with open(sys.argv[1], "w") as f:
        json.dump(t, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(t)} cases, {len(set(t.values()))} distinct answers, {sum(v.startswith('refused') for v in t.values())} refusals")
