"""What lstm_hip_score costs against the generator's own scorer (profiles/score/cost.jsonl).

  python tools/score_cost.py base --label NAME [--length 2000] [--repeats 5] [--out FILE]
      lstm_hip_generate(count = 0, bits) over texts of `length` bytes at N = 512, 64 and 1024 streams.  One JSON line per
      shape and round.  Uses nothing a library before lstm_hip_score lacks, so LSTM_HIP_LIB=<a build of the parent commit>
      runs the parent; run parent and branch alternately, twice each: the branch's medians have to lie within the spread of
      the two parent runs, since no existing launch has changed.
  python tools/score_cost.py score [--length 2000] [--repeats 5] [--out FILE]
      per shape that call, then lstm_hip_score asked for surprisal, entropy and bits only (the head without the ranking), with
      top_n 0 (Lstm.score: rank as well, so the ranking head) and with top_n 4, each the median of `repeats` calls after one
      untimed call, the four taken alternately in two rounds; the score calls as ratios to the generate call of the same round.

A call's time is its wall time (it ends in a stream synchronise), reported per byte position (the call's time over `length`).
The model is tools/sampling_cost.py's: the seeded initialisation with the output layer scaled by 9; the texts have the byte
statistics of real text.  With --out the lines are appended to FILE as well as printed."""
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
ROUNDS = 2


def _handle(N):
    L = lstm_hip.Lstm(N, 2, 1)
    P = lstm_hip.init_params(lstm_hip.MT19937Normal(1), N)
    P[4 * N * 256 + 4 * N * N + 4 * N:] *= np.float32(OUTPUT_GAIN)  # Why, by
    L.set_params(P)
    return L


def _texts(K, length):
    with open(os.path.join(ROOT, "bench_data", "enwik6_byte_hist.json")) as f:
        p = np.array(json.load(f)["counts"], dtype=np.float64)
    data = np.random.RandomState(K).choice(256, size=K * length, p=p / p.sum()).astype(np.uint8)
    return list(data.reshape(K, length))


def _plain(L, data, off, K):
    """the ABI call with surprisal, entropy and bits wanted and nothing else"""
    import ctypes as C
    p = lstm_hip._ptr
    sur, ent, bits = np.zeros(data.size, np.float32), np.zeros(data.size, np.float32), np.zeros(K)
    opt = lstm_hip._Scoring(C.sizeof(lstm_hip._Scoring), 0, 0, None)
    out = lstm_hip._Scores(C.sizeof(lstm_hip._Scores), p(sur), p(ent), None, None, None, p(bits, C.c_double), None)
    lstm_hip._chk(L.lib.lstm_hip_score(L._h, C.c_int32(K), p(data, C.c_uint8), p(off, C.c_uint64), None, None, C.byref(opt), None,
                                       C.byref(out), None, None))


def _median_us(call, length, repeats):
    """median microseconds per byte position of `repeats` calls after one untimed call"""
    call()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) / length * 1e6)
    return round(float(np.median(times)), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("base", "score"))
    ap.add_argument("--label", default="")
    ap.add_argument("--length", type=int, default=2000)
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
        texts = _texts(K, a.length)
        common = dict(label=a.label, N=N, streams=K, length=a.length, repeats=a.repeats)
        generate = lambda: L.generate(texts, count=0, score=True)
        for rnd in range(ROUNDS):
            g = _median_us(generate, a.length, a.repeats)
            emit(dict(case="generate_count0_bits", round=rnd, **common, us_per_position_median=g))
            if a.mode == "score":
                data, off = lstm_hip._offsets(lstm_hip._bytes_list(texts))
                for name, call in (("score_plain", lambda: _plain(L, data, off, K)), ("score_top0", lambda: L.score(texts, top_n=0)),
                                   ("score_top4", lambda: L.score(texts, top_n=4))):
                    m = _median_us(call, a.length, a.repeats)
                    emit(dict(case=name, round=rnd, **common, us_per_position_median=m, ratio_to_generate=round(m / g, 3)))
        L.close()


if __name__ == "__main__":
    main()
