"""What a constraint of lstm_hip_generate_constrained costs per step (profiles/constraint/cost.jsonl).

  python tools/constraint_cost.py base --label NAME [--count 2000] [--repeats 5] [--out FILE]
      the plain draw (lstm_hip_generate, temperature 1) and the filtered one (top_k 40, top_p 0.9) at the two shapes of
      profiles/generate/speed.jsonl: 64 and 1024 streams at N = 512.  One JSON line per shape and case.  Uses nothing a
      library before the constraint lacks, so LSTM_HIP_LIB=<a build of the parent commit> runs the parent; run parent and
      branch alternately, twice each: the branch's medians have to lie within the spread of the two parent runs.
  python tools/constraint_cost.py constrained [--count 2000] [--repeats 5] [--out FILE]
      per shape the same two cases and then both under the UTF-8 table (lstm_hip_dfa_utf8), each as a ratio to the plain and
      to the filtered call of the same process; `mean_kept` says how much was cut, `valid` that every stream's output walks
      the table.

A step's time is the call's wall time (it ends in a stream synchronise) over `count`; the best and the median of `repeats`
calls after one untimed call.  The model is tools/sampling_cost.py's: the seeded initialisation with the output layer scaled
by 9.  With --out the lines are appended to FILE as well as printed."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "eigen-lstm_amd"))
import lstm_hip  # noqa: E402

SHAPES = ((512, 64), (512, 1024))  # (N, streams)
OUTPUT_GAIN = 9.0
FILTER = dict(top_k=40, top_p=0.9)


def _handle(N):
    L = lstm_hip.Lstm(N, 2, 1)
    P = lstm_hip.init_params(lstm_hip.MT19937Normal(1), N)
    P[4 * N * 256 + 4 * N * N + 4 * N:] *= np.float32(OUTPUT_GAIN)  # Why, by
    L.set_params(P)
    return L


def _inputs(N, K, count):
    rs = np.random.RandomState(K)
    return dict(count=count, u=rs.random_sample((count, K)), h0=(rs.randn(K, N) * 0.1).astype(np.float32),
                c0=(rs.randn(K, N) * 0.1).astype(np.float32))


def _steps(L, kw, count, repeats, **controls):
    """(best, median) microseconds per step of `repeats` calls, and the last call's result"""
    L.generate(**{**kw, "count": min(count, 50), "u": kw["u"][:50]}, **controls)
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = L.generate(**kw, **controls)
        times.append((time.perf_counter() - t0) / count * 1e6)
    return round(min(times), 2), round(float(np.median(times)), 2), r


def _accepted(table, out):
    """every stream's bytes walk the table from state 0"""
    q = np.zeros(out.shape[1], np.int64)
    for row in out:
        q = table[q, row].astype(np.int64)
        if (q == 0xFFFF).any():
            return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("base", "constrained"))
    ap.add_argument("--label", default="")
    ap.add_argument("--count", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    for N, K in SHAPES:
        L = _handle(N)
        kw = _inputs(N, K, a.count)
        common = dict(label=a.label, N=N, streams=K, count=a.count, repeats=a.repeats)
        pb, pm, _ = _steps(L, kw, a.count, a.repeats)
        emit(dict(case="plain", **common, us_per_step=pb, us_per_step_median=pm))
        fb, fm, _ = _steps(L, kw, a.count, a.repeats, **FILTER)
        emit(dict(case="top_k_40_top_p_0.9", **common, us_per_step=fb, us_per_step_median=fm))
        if a.mode == "constrained":
            table = lstm_hip.dfa_utf8()
            for name, controls in (("utf8", dict()), ("utf8_top_k_40_top_p_0.9", FILTER)):
                b, m, r = _steps(L, kw, a.count, a.repeats, info=True, constraint=table, **controls)
                emit(dict(case=name, **common, us_per_step=b, us_per_step_median=m,
                          ratio_of_medians_to_plain=round(m / pm, 3), ratio_of_medians_to_filtered=round(m / fm, 3),
                          mean_kept=round(float(r[4]["kept"].mean()), 2), valid=_accepted(table, r[0])))
        L.close()


if __name__ == "__main__":
    main()
