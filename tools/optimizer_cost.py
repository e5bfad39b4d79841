"""Adam / AdamW as the update rule (lstm_hip_set_optimizer): its cost against Adagrad and a training comparison.

  python tools/optimizer_cost.py cost    three handles per shape -- Adagrad, Adam, AdamW (weight decay 0.01) -- at the
                                         headline shape (hidden 512, window 100, batch 64, fp32) and BASELINE configs[4]
                                         (hidden 1024, window 100, batch 16, bf16), one process, 7 interleaved rounds:
                                         per-launch HIP-event time of the update launch (`adagrad` / `adam`, 20 profiled
                                         windows) and the unprofiled window (train_windows' elapsed time over 50)
  python tools/optimizer_cost.py train   the headline shape with LSTM_HIP_STABLE_SOFTMAX from the start of
                                         tools/grad_clip_cost.py train: Adagrad at lr 0.1 against Adam and AdamW at lr 2e-3,
                                         3000 windows; bits/char (window loss / (S-1)) at windows 100, 300 and 3000
  python tools/optimizer_cost.py prof    50 Adam windows of each shape and nothing else (for rocprofv3 --kernel-trace --stats)

Each mode prints one JSON line of results.
"""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "eigen-lstm_amd"), ROOT, os.path.join(ROOT, "tests")]
import lstm_hip  # noqa: E402
from bench import synthetic_text  # noqa: E402

SHAPES = {"headline": (512, 100, 64, 0), "configs4_bf16": (1024, 100, 16, lstm_hip.BF16_RECURRENCE)}
RULES = {"adagrad": (None, 0.01), "adam": (0.0, 2e-3), "adamw": (0.01, 2e-3)}  # weight decay (None: Adagrad), lr


def handle(N, S, B, flags, text, wd, P=None):
    L = lstm_hip.Lstm(N, S, B, flags=flags)
    if wd is not None:
        L.set_optimizer(lstm_hip.OPT_ADAM, weight_decay=wd)
    L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(1), N) if P is None else P)
    L.set_text(text)
    L.set_cursors(lstm_hip.initial_cursors(len(text), S, B))
    L.reset_window()
    return L


def cost():
    text = synthetic_text(1_000_000, seed=0)
    out = {}
    for shape, (N, S, B, flags) in SHAPES.items():
        hs = {k: handle(N, S, B, flags, text, wd) for k, (wd, _) in RULES.items()}
        for k, L in hs.items():
            L.train_windows(5, RULES[k][1])
        upd = {k: [] for k in hs}
        win = {k: [] for k in hs}
        for _ in range(7):
            for k, L in hs.items():
                lr = RULES[k][1]
                L.set_profiling(1)
                L.reset_kernel_stats()
                L.train_windows(20, lr)
                L.synchronize()
                n, ms = L.kernel_stats()["adagrad" if k == "adagrad" else "adam"]
                upd[k].append(1000.0 * ms / n)
                L.set_profiling(0)
                _, t = L.train_windows(50, lr, want_time=True)
                win[k].append(t / 50)
        out[shape] = {"shape": [N, S, B], "flags": flags}
        for k in hs:
            out[shape][k] = {"window_ms_median": statistics.median(win[k]), "window_ms_min": min(win[k]),
                             "update_us_median": statistics.median(upd[k])}
        base = out[shape]["adagrad"]["window_ms_median"]
        for k in ("adam", "adamw"):
            out[shape][k]["window_vs_adagrad"] = out[shape][k]["window_ms_median"] / base
        for L in hs.values():
            L.close()
    return out


def train():
    from oracle_lib import Oracle
    N, S, B, windows = 512, 100, 64, 3000
    text = synthetic_text(1_000_000, seed=0)
    tr = Oracle("f32_omp").trainer(text, N, S, B, lr=0.1, seed=1)
    tr.epoch_reset()
    out = {"shape": [N, S, B], "flags": lstm_hip.STABLE_SOFTMAX, "windows": windows}
    for name, wd, lr in (("adagrad_lr0.1", None, 0.1), ("adam_lr2e-3", 0.0, 2e-3), ("adamw_lr2e-3_wd0.01", 0.01, 2e-3)):
        L = lstm_hip.Lstm(N, S, B, flags=lstm_hip.STABLE_SOFTMAX)
        if wd is not None:
            L.set_optimizer(lstm_hip.OPT_ADAM, weight_decay=wd)
        L.set_params(tr.params.copy())
        L.set_state(1, tr.h[1], tr.c[1])
        L.set_text(text)
        L.set_cursors(lstm_hip.initial_cursors(len(text), S, B))
        L.reset_window()
        ls = np.concatenate([L.train_windows(500, lr) for _ in range(windows // 500)])
        L.close()
        bpc = ls / (S - 1)
        out[name] = {"bits_per_char_w100": float(bpc[99]), "bits_per_char_w300": float(bpc[299]),
                     "bits_per_char_w3000": float(bpc[2999]), "mean_bits_per_char_w2901_3000": float(np.mean(bpc[2900:3000])),
                     "finite": bool(np.isfinite(ls).all())}
    return out


def prof():
    text = synthetic_text(1_000_000, seed=0)
    for N, S, B, flags in SHAPES.values():
        L = handle(N, S, B, flags, text, 0.0)
        L.train_windows(50, 2e-3)
        L.close()
    return {"prof": "done"}


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "cost"
    print(json.dumps({"mode": mode, **{"cost": cost, "train": train, "prof": prof}[mode]()}))
