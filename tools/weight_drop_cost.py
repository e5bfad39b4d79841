"""Weight drop (lstm_hip_set_weight_drop): what its two launches and the repack cost per window, and what it buys on held-out
text.

  python tools/weight_drop_cost.py cost     the headline shape (hidden 512, window 100, batch 64, fp32) and configs[4] (hidden
                                            1024, window 100, batch 16, LSTM_HIP_BF16_RECURRENCE): ONE handle per shape, whose
                                            weight drop is switched between three arms -- off, rate 0.25, rate 0.5 -- in 6
                                            interleaved rounds; per arm and round the elapsed time of train_windows(200).  One
                                            JSON line per measurement, then one summary line per shape: medians, the spread of the
                                            off arm's own repeats and each arm's extra time per window against the off arm.
  python tools/weight_drop_cost.py heldout  the run of tools/averaging_cost.py heldout (hidden 256, window 50, batch 32, Adam at
                                            a constant lr 2e-3, a tools/make_text.py corpus whose last 20 000 bytes are held
                                            out) at rates 0, 0.25 and 0.5: training loss and held-out bits/char every 1000
                                            windows up to 6000.  One seed.  One JSON line per rate and checkpoint.
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

ARMS = {"off": 0.0, "rate_0.25": 0.25, "rate_0.5": 0.5}
WINDOWS, ROUNDS = 200, 6
SHAPES = (("headline_fp32", 512, 100, 64, 0), ("configs4_bf16", 1024, 100, 16, lstm_hip.BF16_RECURRENCE))


def cost():
    text = synthetic_text(1_000_000, seed=0)
    for name, N, S, B, flags in SHAPES:
        lr = 0.01
        L = lstm_hip.Lstm(N, S, B, flags=flags)
        L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(1), N))
        L.set_text(text)
        L.set_cursors(lstm_hip.initial_cursors(len(text), S, B))
        L.reset_window()
        L.train_windows(50, lr)
        ms = {arm: [] for arm in ARMS}
        for rep in range(ROUNDS):
            for arm, rate in ARMS.items():
                L.set_weight_drop(rate, 1, L.weight_drop()[2])
                _, t = L.train_windows(WINDOWS, lr, want_time=True)
                ms[arm].append(t / WINDOWS)
                print(json.dumps({"mode": "cost", "shape": [N, S, B], "engine": name, "arm": arm, "round": rep,
                                  "windows": WINDOWS, "window_ms": t / WINDOWS}), flush=True)
        L.close()
        off = statistics.median(ms["off"])
        line = {"mode": "cost_summary", "shape": [N, S, B], "engine": name, "u_floats": 4 * N * N,
                "off_window_ms_median": off, "off_window_ms_spread": max(ms["off"]) - min(ms["off"])}
        for arm in ARMS:
            if arm == "off":
                continue
            med = statistics.median(ms[arm])
            line[arm] = {"window_ms_median": med, "window_ms_spread": max(ms[arm]) - min(ms[arm]),
                         "extra_us_per_window": 1000.0 * (med - off), "window_vs_off": med / off}
        print(json.dumps(line), flush=True)


def heldout():
    N, S, B, lr, total, step, tail = 256, 50, 32, 2e-3, 6000, 1000, 20_000
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "corpus.txt")
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_text.py"), path, "1000000"])
        data = np.fromfile(path, np.uint8)
    train, held = data[:-tail], data[-tail:]
    for rate in (0.0, 0.25, 0.5):
        L = lstm_hip.Lstm(N, S, B)
        L.set_optimizer(lstm_hip.OPT_ADAM)
        L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(1), N))
        L.set_text(train)
        L.set_cursors(lstm_hip.initial_cursors(len(train), S, B))
        L.reset_window()
        L.set_weight_drop(rate, 1, 0)
        for done in range(step, total + 1, step):
            losses = L.train_windows(step, lr)
            print(json.dumps({"mode": "heldout", "shape": [N, S, B], "optimizer": "adam", "lr": lr, "rate": rate, "windows": done,
                              "heldout_bytes": tail, "mask_index": L.weight_drop()[2],
                              "train_bits_per_char_last100": float(np.mean(losses[-100:]) / (S - 1)),
                              "heldout_bits_per_char": L.eval_bits(held)}), flush=True)
        L.close()


if __name__ == "__main__":
    {"cost": cost, "heldout": heldout}[sys.argv[1] if len(sys.argv) > 1 else "cost"]()
