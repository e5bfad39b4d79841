"""What the sampling controls of lstm_hip_generate_ex cost per step (profiles/sampling/).

  python tools/sampling_cost.py base --label NAME [--count 2000] [--repeats 5]
      the unfiltered step (lstm_hip_generate, temperature 1) at the two shapes of profiles/generate/speed.jsonl: 64 and
      1024 streams at N = 512.  One JSON line per shape.  Uses nothing a library before the controls lacks, so
      LSTM_HIP_LIB=<a build of the parent commit> runs the parent; run parent and branch alternately, twice each.
  python tools/sampling_cost.py filters [--count 2000] [--repeats 5]
      per shape the unfiltered step and the steps with top_k 40, top_p 0.9, both, and a stop byte alone, each as a ratio to
      the unfiltered step of the same process; `mean_kept` says how much the filter cut.
  python tools/sampling_cost.py prof [--count 500]
      one call with both filters per shape and nothing else timed, for `rocprofv3 --kernel-trace --stats`.

A step's time is the call's wall time (it ends in a stream synchronise) over `count`; the best and the median of `repeats`
calls after one untimed call.  The model is the seeded initialisation with the output layer scaled by 9, which makes the
distributions as peaked as a trained model's (top_p 0.9 then keeps some tens of bytes, not 230)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("base", "filters", "prof"))
    ap.add_argument("--label", default="")
    ap.add_argument("--count", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    for N, K in SHAPES:
        L = _handle(N)
        kw = _inputs(N, K, a.count)
        if a.mode == "prof":
            L.generate(top_k=40, top_p=0.9, **kw)
            L.close()
            continue
        best, med, ref = _steps(L, kw, a.count, a.repeats)
        row = dict(case="unfiltered", label=a.label, N=N, streams=K, count=a.count, repeats=a.repeats, us_per_step=best,
                   us_per_step_median=med)
        print(json.dumps(row), flush=True)
        if a.mode == "filters":
            for name, controls in (("top_k_40", dict(top_k=40)), ("top_p_0.9", dict(top_p=0.9)),
                                   ("top_k_40_top_p_0.9", dict(top_k=40, top_p=0.9)),
                                   ("stop_byte_only", dict(stop_byte=int(np.bincount(ref[0].ravel(), minlength=256).argmin())))):
                b, m, r = _steps(L, kw, a.count, a.repeats, info=True, **controls)
                print(json.dumps(dict(case=name, N=N, streams=K, count=a.count, repeats=a.repeats, us_per_step=b,
                                      us_per_step_median=m, ratio_to_unfiltered=round(b / best, 3),
                                      ratio_of_medians=round(m / med, 3), mean_kept=round(float(r[4]["kept"].mean()), 2),
                                      mean_out_len=round(float(r[4]["out_len"].mean()), 1))), flush=True)
        L.close()


if __name__ == "__main__":
    main()
