"""Batched generation and scoring (lstm_hip_generate) against the equivalent sequential calls, in one process.

  python tools/generate_speed.py [--count 2000] [--seq-calls 8]

Prints one JSON line per case:
  generate  N in (512, 1024), K in (1, 64, 256, 1024) streams of `count` bytes: one batched call against K calls of
            lstm_hip_sample.  The sequential side is timed on min(K, seq-calls) streams and scaled to K (the calls are
            identical in cost; `seq_measured` says how many ran); the bytes of those streams must match the batched ones.
  score     64 texts of 16 KiB at N = 512: one batched call against 64 calls of lstm_hip_eval_bits (all measured).
`ratio` = sequential / batched time.  Each side runs once untimed first."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "eigen-lstm_amd"))
import lstm_hip  # noqa: E402


def _timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def generate_case(N, K, count, seq_calls):
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(1), N))
    rs = np.random.RandomState(K)
    u = rs.random_sample((count, K))
    h0 = (rs.randn(K, N) * 0.1).astype(np.float32)
    c0 = (rs.randn(K, N) * 0.1).astype(np.float32)
    L.generate(count=min(count, 50), u=u[:50], h0=h0, c0=c0)
    tb, (out, _, _, _) = _timed(lambda: L.generate(count=count, u=u, h0=h0, c0=c0))
    k = min(K, seq_calls)
    L.sample(h0[0], c0[0], u[:50, 0])
    ts, outs = _timed(lambda: [L.sample(h0[s], c0[s], u[:, s])[0] for s in range(k)])
    match = all(np.array_equal(outs[s], out[:, s]) for s in range(k))
    L.close()
    seq = ts * K / k
    return dict(case="generate", N=N, streams=K, count=count, batched_s=round(tb, 4), sequential_s=round(seq, 4),
                seq_measured=k, ratio=round(seq / tb, 2), batched_us_per_step=round(tb / count * 1e6, 2),
                sample_us_per_char=round(ts / (k * count) * 1e6, 2), match=match)


def score_case(N, K, n):
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(2), N))
    rs = np.random.RandomState(3)
    texts = [rs.randint(32, 127, size=n).astype(np.uint8) for _ in range(K)]
    L.generate(texts, score=True)
    tb, (_, bits, _, _) = _timed(lambda: L.generate(texts, score=True))
    L.eval_bits(texts[0][:1000])
    ts, ev = _timed(lambda: [L.eval_bits(t) for t in texts])
    L.close()
    err = max(abs(bits[s] / (n - 1) - ev[s]) for s in range(K))
    return dict(case="score", N=N, streams=K, bytes_per_text=n, batched_s=round(tb, 4), sequential_s=round(ts, 4),
                ratio=round(ts / tb, 2), batched_us_per_step=round(tb / n * 1e6, 2), max_abs_bits_per_char_diff=float(err))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=2000)
    ap.add_argument("--seq-calls", type=int, default=8)
    ap.add_argument("--only", choices=("generate", "score"), default=None)
    a = ap.parse_args()
    name, cus, mhz = lstm_hip.device_info(0)
    print(json.dumps(dict(case="device", name=name, cus=cus, clock_mhz=mhz)), flush=True)
    if a.only != "score":
        for N in (512, 1024):
            for K in (1, 64, 256, 1024):
                print(json.dumps(generate_case(N, K, a.count, a.seq_calls)), flush=True)
    if a.only != "generate":
        print(json.dumps(score_case(512, 64, 16384)), flush=True)


if __name__ == "__main__":
    main()
