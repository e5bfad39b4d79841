"""Global-norm gradient clipping (lstm_hip_set_grad_clip): its cost and its effect on training.

  python tools/grad_clip_cost.py cost    three handles per shape -- clipping off, measure only (max_norm = inf), clip 5 --
                                         at the headline shape (hidden 512, window 100, batch 64, fp32) and BASELINE
                                         configs[4] (hidden 1024, window 100, batch 16, bf16), one process, 7 interleaved
                                         rounds: per-launch HIP-event times of grad_sumsq, grad_norm and adagrad (20
                                         profiled windows) and the unprofiled window (train_windows' elapsed time over 50)
  python tools/grad_clip_cost.py train   lr 0.1 with LSTM_HIP_STABLE_SOFTMAX at the headline shape from the start of
                                         tests/test_stable_softmax.py::test_reference_learning_rate_trains_finite, 300
                                         windows without clipping and with max_norm 1 and 5: bits/char (window loss / (S-1))
                                         at windows 100 and 300, and the pre-clip norms
  python tools/grad_clip_cost.py prof    50 clipped windows of each shape and nothing else (for rocprofv3 --kernel-trace --stats)

Each mode prints one JSON line of results.
"""
import json
import math
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "eigen-lstm_amd"), ROOT, os.path.join(ROOT, "tests")]
import lstm_hip  # noqa: E402
from bench import synthetic_text  # noqa: E402

SHAPES = {"headline": (512, 100, 64, 0), "configs4_bf16": (1024, 100, 16, lstm_hip.BF16_RECURRENCE)}
SETTINGS = {"off": None, "measure": math.inf, "clip5": 5.0}


def handle(N, S, B, flags, text, clip, P=None):
    L = lstm_hip.Lstm(N, S, B, flags=flags)
    L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(1), N) if P is None else P)
    L.set_text(text)
    L.set_cursors(lstm_hip.initial_cursors(len(text), S, B))
    L.reset_window()
    if clip is not None:
        L.set_grad_clip(clip)
    return L


def cost():
    text = synthetic_text(1_000_000, seed=0)
    out = {}
    for shape, (N, S, B, flags) in SHAPES.items():
        hs = {k: handle(N, S, B, flags, text, c) for k, c in SETTINGS.items()}
        for L in hs.values():
            L.train_windows(5, 0.01)
        kern = {k: {"grad_sumsq": [], "grad_norm": [], "adagrad": []} for k in hs}
        win = {k: [] for k in hs}
        for _ in range(7):
            for k, L in hs.items():
                L.set_profiling(1)
                L.reset_kernel_stats()
                L.train_windows(20, 0.01)
                L.synchronize()
                st = L.kernel_stats()
                for name in kern[k]:
                    n, ms = st[name]
                    if n:
                        kern[k][name].append(1000.0 * ms / n)
                L.set_profiling(0)
                _, t = L.train_windows(50, 0.01, want_time=True)
                win[k].append(t / 50)
        out[shape] = {"shape": [N, S, B], "flags": flags}
        for k in hs:
            r = {"window_ms_median": statistics.median(win[k]), "window_ms_min": min(win[k])}
            for name, v in kern[k].items():
                if v:
                    r[name + "_us_median"] = statistics.median(v)
            out[shape][k] = r
        for L in hs.values():
            L.close()
    return out


def train():
    from oracle_lib import Oracle
    N, S, B, lr, windows = 512, 100, 64, 0.1, 300
    text = synthetic_text(1_000_000, seed=0)
    tr = Oracle("f32_omp").trainer(text, N, S, B, lr=lr, seed=1)
    tr.epoch_reset()
    out = {"shape": [N, S, B], "lr": lr, "flags": lstm_hip.STABLE_SOFTMAX}
    for name, clip in (("no_clip", math.inf), ("clip1", 1.0), ("clip5", 5.0)):
        L = lstm_hip.Lstm(N, S, B, flags=lstm_hip.STABLE_SOFTMAX)
        L.set_params(tr.params.copy())
        L.set_state(1, tr.h[1], tr.c[1])
        L.set_text(text)
        L.set_cursors(lstm_hip.initial_cursors(len(text), S, B))
        L.reset_window()
        L.set_grad_clip(clip)  # (inf: the unclipped trajectory, bit for bit, with its norms recorded)
        ls = L.train_windows(windows, lr)
        norms = L.grad_norms(windows)
        L.close()
        bpc = ls / (S - 1)
        out[name] = {"bits_per_char_w100": float(bpc[99]), "bits_per_char_w300": float(bpc[299]),
                     "mean_bits_per_char_w281_300": float(np.mean(bpc[280:300])), "finite": bool(np.isfinite(ls).all()),
                     "norm_w1": float(norms[0]), "norm_median": float(np.median(norms)), "norm_max": float(np.max(norms)),
                     "clipped_windows": int(np.sum(np.isfinite(norms) & (np.float32(clip / (norms + 1e-6)) < 1)))}
    return out


def prof():
    text = synthetic_text(1_000_000, seed=0)
    for N, S, B, flags in SHAPES.values():
        L = handle(N, S, B, flags, text, 5.0)
        L.train_windows(50, 0.01)
        L.close()
    return {"prof": "done"}


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "cost"
    print(json.dumps({"mode": mode, **{"cost": cost, "train": train, "prof": prof}[mode]()}))
