"""Gradient accumulation (lstm_hip_set_grad_accumulation): what a window costs with it on, and one line on what it is for.

  python tools/accumulation_cost.py window [every]   hidden 512, window 100, batch 64, fp32: the elapsed time of
                                          train_windows(200) per window, 6 repeats after 50 warm-up windows, with `every`
                                          windows per update (default 1: off; a library without the call, named by
                                          LSTM_HIP_LIB, runs the off arm only).  200 is a multiple of every, so every repeat
                                          holds whole cycles.  One JSON line per repeat, then a summary line.  Arms are
                                          compared by running this once per arm and library, alternated, in one session.
  python tools/accumulation_cost.py heldout  hidden 1024, window 100, batch 32 (the widest batch the persistent fp32 forms
                                          hold), Adam at lr 5e-4 and 2e-3 on a tools/make_text.py corpus whose last 20 000 bytes
                                          are held out, cut into 50 texts for lstm_hip_eval_texts: every in {1, 4} with the mean,
                                          the same 1200 windows (the same bytes) each; held-out bits/char every 400 windows.
"""
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "eigen-lstm_amd"), ROOT]
import lstm_hip  # noqa: E402
from bench import synthetic_text  # noqa: E402

WINDOWS, REPEATS = 200, 6


def window(every):
    N, S, B, lr = 512, 100, 64, 0.01
    text = synthetic_text(1_000_000, seed=0)
    L = lstm_hip.Lstm(N, S, B)
    L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(1), N))
    L.set_text(text)
    L.set_cursors(lstm_hip.initial_cursors(len(text), S, B))
    L.reset_window()
    if every > 1:
        L.set_grad_accumulation(every)
    L.train_windows(50 // every * every, lr)
    ms = []
    for rep in range(REPEATS):
        _, t = L.train_windows(WINDOWS, lr, want_time=True)
        ms.append(t / WINDOWS)
        print(json.dumps({"mode": "window", "lib": os.path.relpath(lstm_hip.LIB_PATH, ROOT), "shape": [N, S, B], "every": every,
                          "repeat": rep, "windows": WINDOWS, "window_ms": t / WINDOWS}), flush=True)
    L.close()
    print(json.dumps({"mode": "window_summary", "lib": os.path.relpath(lstm_hip.LIB_PATH, ROOT), "shape": [N, S, B], "every": every,
                      "window_ms_median": statistics.median(ms), "window_ms_min": min(ms), "window_ms_max": max(ms)}), flush=True)


def heldout():
    N, S, B, total, step, tail, pieces = 1024, 100, 32, 1200, 400, 20_000, 50
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "corpus.txt")
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_text.py"), path, "1000000"])
        data = np.fromfile(path, np.uint8)
    train, held = data[:-tail], data[-tail:]
    texts = [held[i * (tail // pieces):(i + 1) * (tail // pieces)] for i in range(pieces)]
    for lr, every in ((5e-4, 1), (5e-4, 4), (2e-3, 1), (2e-3, 4)):
        L = lstm_hip.Lstm(N, S, B)
        L.set_optimizer(lstm_hip.OPT_ADAM)
        L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(1), N))
        L.set_text(train)
        L.set_cursors(lstm_hip.initial_cursors(len(train), S, B))
        L.reset_window()
        L.set_grad_accumulation(every, mean=True)
        ms = 0.0
        for done in range(step, total + 1, step):
            losses, t = L.train_windows(step, lr, want_time=True)
            ms += t
            bits = L.eval_texts(texts)["bits"]  # (the first byte of a text is fed, not scored)
            print(json.dumps({"mode": "heldout", "plan": L.plan_identity(), "shape": [N, S, B], "optimizer": "adam", "lr": lr,
                              "every": every, "mean": True, "windows": done, "updates": L.optimizer_steps(),
                              "bytes_seen": done * (S - 1) * B, "train_ms": ms, "heldout_bytes": tail,
                              "train_bits_per_char_last100": float(np.mean(losses[-100:]) / (S - 1)),
                              "heldout_bits_per_char": float(bits.sum() / (tail - pieces))}), flush=True)
        L.close()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "window"
    if mode == "window":
        window(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
    else:
        heldout()
