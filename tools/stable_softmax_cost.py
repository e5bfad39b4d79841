"""Cost of LSTM_HIP_STABLE_SOFTMAX at the headline shape (hidden 512, window 100, batch 64): a default and a stable handle in
one process, timed in 7 interleaved rounds -- k_softmax_loss_dy per launch from the library's HIP-event profiling (20 windows)
and the whole window unprofiled (train_windows' elapsed time over 50 windows).  Prints one JSON line of medians and minima.

  python tools/stable_softmax_cost.py
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "eigen-lstm_amd"))
sys.path.insert(0, ROOT)
import lstm_hip  # noqa: E402
from bench import synthetic_text  # noqa: E402
N, S, B = 512, 100, 64
text = synthetic_text(1_000_000, seed=0)
g = lstm_hip.MT19937Normal(1)
P = lstm_hip.init_params(g, N)
hs = {}
for name, flags in (("default", 0), ("stable", lstm_hip.STABLE_SOFTMAX)):
    L = lstm_hip.Lstm(N, S, B, flags=flags)
    L.set_params(P)
    L.set_text(text)
    L.set_cursors(lstm_hip.initial_cursors(len(text), S, B))
    L.reset_window()
    L.train_windows(5, 0.01)
    hs[name] = L
res = {k: [] for k in hs}
win = {k: [] for k in hs}
for r in range(7):
    for k, L in hs.items():
        L.set_profiling(1)
        L.reset_kernel_stats()
        L.train_windows(20, 0.01)
        L.synchronize()
        n, ms = L.kernel_stats()["softmax_loss_dy"]
        res[k].append(1000.0 * ms / n)
        L.set_profiling(0)
        _, t = L.train_windows(50, 0.01, want_time=True)
        win[k].append(t / 50)
out = {k: {"softmax_us_median": statistics.median(v), "softmax_us_min": min(v), "window_ms_median": statistics.median(win[k]),
           "window_ms_min": min(win[k])} for k, v in res.items()}
print(json.dumps({"shape": [N, S, B], **out}))
for L in hs.values():
    L.close()
