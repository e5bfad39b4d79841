"""The running weight average (lstm_hip_set_averaging): what its launch costs, and what the average buys on held-out text.

  python tools/averaging_cost.py cost     hidden 512, window 100, batch 64, fp32 and with LSTM_HIP_BF16_RECURRENCE: ONE handle
                                          per shape, whose averaging is switched between three arms -- off, EMA every = 1, EMA
                                          every = 10 -- in 6 interleaved rounds; per arm and round the elapsed time of
                                          train_windows(200).  One JSON line per measurement, then one summary line per shape:
                                          medians, the spread of the off arm's own repeats, and each arm's cost per window and
                                          per due update against the off arm.
  python tools/averaging_cost.py heldout  hidden 256, window 50, batch 32, Adam at a constant lr 2e-3 on a tools/make_text.py
                                          corpus whose last 20 000 bytes are held out: bits/char of the last iterate, of the
                                          EMA (decay 0.999, from the first window) and of the uniform mean (from window 2000) every
                                          1000 windows up to 6000.  Two handles train identically (the average never touches
                                          training); each carries one kind.  One JSON line per checkpoint.
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

ARMS = {"off": (lstm_hip.AVG_OFF, 0.0, 1), "ema_every1": (lstm_hip.AVG_EMA, 0.999, 1), "ema_every10": (lstm_hip.AVG_EMA, 0.999, 10)}
WINDOWS, ROUNDS = 200, 6


def cost():
    text = synthetic_text(1_000_000, seed=0)
    for name, flags in (("fp32", 0), ("bf16_recurrence", lstm_hip.BF16_RECURRENCE)):
        N, S, B, lr = 512, 100, 64, 0.01
        L = lstm_hip.Lstm(N, S, B, flags=flags)
        L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(1), N))
        L.set_text(text)
        L.set_cursors(lstm_hip.initial_cursors(len(text), S, B))
        L.reset_window()
        L.train_windows(50, lr)
        ms = {arm: [] for arm in ARMS}
        for rep in range(ROUNDS):
            for arm, (kind, decay, every) in ARMS.items():
                L.set_averaging(kind, decay, every)
                _, t = L.train_windows(WINDOWS, lr, want_time=True)
                ms[arm].append(t / WINDOWS)
                print(json.dumps({"mode": "cost", "shape": [N, S, B], "engine": name, "arm": arm, "round": rep,
                                  "windows": WINDOWS, "window_ms": t / WINDOWS}), flush=True)
        L.close()
        off = statistics.median(ms["off"])
        line = {"mode": "cost_summary", "shape": [N, S, B], "engine": name, "block_floats": lstm_hip.param_count(N),
                "off_window_ms_median": off, "off_window_ms_spread": max(ms["off"]) - min(ms["off"])}
        for arm, (_, _, every) in ARMS.items():
            if arm == "off":
                continue
            med = statistics.median(ms[arm])
            line[arm] = {"window_ms_median": med, "window_ms_spread": max(ms[arm]) - min(ms[arm]),
                         "extra_us_per_window": 1000.0 * (med - off), "extra_us_per_due_update": 1000.0 * (med - off) * every,
                         "window_vs_off": med / off}
        print(json.dumps(line), flush=True)


def heldout():
    N, S, B, lr, total, step, uniform_from, tail = 256, 50, 32, 2e-3, 6000, 1000, 2000, 20_000
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "corpus.txt")
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_text.py"), path, "1000000"])
        data = np.fromfile(path, np.uint8)
    train, held = data[:-tail], data[-tail:]
    hs = {}
    for kind in ("ema", "uniform"):
        L = lstm_hip.Lstm(N, S, B)
        L.set_optimizer(lstm_hip.OPT_ADAM)
        L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(1), N))
        L.set_text(train)
        L.set_cursors(lstm_hip.initial_cursors(len(train), S, B))
        L.reset_window()
        hs[kind] = L
    hs["ema"].set_averaging(lstm_hip.AVG_EMA, 0.999, 1)
    for done in range(step, total + 1, step):
        if done - step == uniform_from:
            hs["uniform"].set_averaging(lstm_hip.AVG_UNIFORM, 0.0, 1)
        losses = {k: L.train_windows(step, lr) for k, L in hs.items()}
        line = {"mode": "heldout", "shape": [N, S, B], "optimizer": "adam", "lr": lr, "windows": done, "heldout_bytes": tail,
                "train_bits_per_char_last100": float(np.mean(losses["ema"][-100:]) / (S - 1)),
                "twins_identical": bool(hs["ema"].get_params().tobytes() == hs["uniform"].get_params().tobytes()),
                "last_iterate": hs["ema"].eval_bits(held)}
        for kind, L in hs.items():
            if kind == "uniform" and done <= uniform_from:
                line[kind] = None
                continue
            L.set_inference_source(lstm_hip.SRC_AVERAGE)
            line[kind] = L.eval_bits(held)
            L.set_inference_source(lstm_hip.SRC_PARAMS)
            line[kind + "_n"] = L.averaging_counts()[1]
        print(json.dumps(line), flush=True)
    for L in hs.values():
        L.close()


if __name__ == "__main__":
    {"cost": cost, "heldout": heldout}[sys.argv[1] if len(sys.argv) > 1 else "cost"]()
