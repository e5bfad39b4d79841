"""What a beam-search step costs (profiles/beam/).

  python tools/beam_cost.py steps [--count 2000] [--repeats 5]
      N = 512, 64 streams x W in {4, 16} beams: the beam step (lstm_hip_beam_search) and the generator's greedy step
      (lstm_hip_generate, temperature 0) at the same number of columns, 64 * W streams.  Both are taken twice, alternately
      (beam, greedy, beam, greedy); one JSON line per measurement and one per shape with the ratios.
  python tools/beam_cost.py prof [--count 200] [--constraint trivial|utf8]
      one search per shape and nothing else timed, for `rocprofv3 --kernel-trace --stats` (tools/kernel_stats_from_db.py).
  python tools/beam_cost.py step --constraint none|trivial|utf8 [--label NAME]
      the beam step alone at both shapes, one JSON line per shape (profiles/beam/constrained_cost.jsonl; DESIGN.md section
      3.12): unconstrained, under a one-state table that allows everything, or under the UTF-8 table with state 0 accepting
      (lstm_hip_beam_search_constrained).  One process measures one side; the sides -- the parent commit's library through
      LSTM_HIP_LIB with `none`, then this build's three -- are run alternately, twice each, by the caller.

A step's time is the call's wall time (it ends in a stream synchronise) over `count`; the best and the median of `repeats`
calls after one untimed call.  The model is the seeded initialisation with the output layer scaled by 9, as peaked as a
trained model's (tools/sampling_cost.py)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "eigen-lstm_amd"))
import lstm_hip  # noqa: E402

N, STREAMS, BEAMS = 512, 64, (4, 16)
OUTPUT_GAIN = 9.0


def _handle():
    L = lstm_hip.Lstm(N, 2, 1)
    P = lstm_hip.init_params(lstm_hip.MT19937Normal(1), N)
    P[4 * N * 256 + 4 * N * N + 4 * N:] *= np.float32(OUTPUT_GAIN)  # Why, by
    L.set_params(P)
    return L


def _time(call, count, repeats):
    """(best, median) microseconds per step of `repeats` calls after one untimed call"""
    call()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) / count * 1e6)
    return round(min(times), 2), round(float(np.median(times)), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("steps", "prof", "step"))
    ap.add_argument("--constraint", choices=("none", "trivial", "utf8"), default="none")
    ap.add_argument("--label", default="")
    ap.add_argument("--count", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    L = _handle()
    rs = np.random.RandomState(7)
    con = {}
    if a.constraint == "trivial":
        con = dict(constraint=np.zeros((1, 256), np.uint16))
    elif a.constraint == "utf8":
        con = dict(constraint=lstm_hip.dfa_utf8(), accept=np.arange(8) == 0)
    for W in BEAMS:
        h0 = (rs.randn(STREAMS, N) * 0.1).astype(np.float32)
        c0 = (rs.randn(STREAMS, N) * 0.1).astype(np.float32)
        beam = lambda: L.beam_search(count=a.count, beams=W, h0=h0, c0=c0, streams=STREAMS, **con)
        if a.mode == "prof":
            beam()
            continue
        if a.mode == "step":
            best, med = _time(beam, a.count, a.repeats)
            print(json.dumps(dict(case="beam", side=a.label or a.constraint, constraint=a.constraint, N=N, streams=STREAMS, beams=W,
                                  count=a.count, repeats=a.repeats, us_per_step=best, us_per_step_median=med)), flush=True)
            continue
        hw, cw = np.repeat(h0, W, axis=0), np.repeat(c0, W, axis=0)
        greedy = lambda: L.generate(count=a.count, temperature=0.0, h0=hw, c0=cw, streams=STREAMS * W)
        got = {"beam": [], "greedy": []}
        for rnd in range(2):
            for name, call in (("beam", beam), ("greedy", greedy)):
                best, med = _time(call, a.count, a.repeats)
                got[name].append((best, med))
                print(json.dumps(dict(case=name, round=rnd, N=N, streams=STREAMS, beams=W, columns=STREAMS * W, count=a.count,
                                      repeats=a.repeats, us_per_step=best, us_per_step_median=med)), flush=True)
        b, g = min(x[0] for x in got["beam"]), min(x[0] for x in got["greedy"])
        bm, gm = np.median([x[1] for x in got["beam"]]), np.median([x[1] for x in got["greedy"]])
        print(json.dumps(dict(case="ratio", N=N, streams=STREAMS, beams=W, columns=STREAMS * W, beam_us_per_step=b,
                              greedy_us_per_step=g, ratio_to_greedy=round(b / g, 3), ratio_of_medians=round(float(bm / gm), 3))),
              flush=True)
    L.close()


if __name__ == "__main__":
    main()
