"""The accepting sampler and the regex compiler: what they cost.

  python tools/regex_cost.py head     per-step cost of gen_head's DEADLINE instantiation against the CONSTRAIN one: ONE handle at
                                      hidden 512, the UTF-8 table, 64 and 1024 streams, 200 drawn bytes; two arms -- accept=None
                                      (lstm_hip_generate_constrained) and accept={0} (lstm_hip_generate_accepting) -- in 8
                                      interleaved rounds; per arm and round the wall time of one call over its steps.  One JSON
                                      line per measurement, then a summary line per shape: medians, the spread of the off arm's
                                      own repeats, the extra time per step.
  python tools/regex_cost.py plain    the off arm alone, 8 calls per shape: the per-step time of lstm_hip_generate_constrained
                                      without accepting states, to set beside the same line of another build (LSTM_HIP_LIB).
  python tools/regex_cost.py compile  host time of lstm_hip_dfa_regex for the largest patterns of tests/test_regex_cpu.py and for
                                      the refused blow-ups (no device needed).
"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "eigen-lstm_amd"), ROOT]
import lstm_hip  # noqa: E402

N, COUNT, ROUNDS = 512, 200, 8
SHAPES = (64, 1024)


def _setup(K):
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(1), N))
    u = np.random.RandomState(K).random_sample((COUNT, K))
    table = lstm_hip.dfa_utf8()
    accept = np.zeros(8, np.uint8)
    accept[0] = 1
    return L, u, table, accept


def _call(L, K, u, table, accept):
    t0 = time.perf_counter()
    L.generate(count=COUNT, u=u, streams=K, temperature=1.0, constraint=table, accept=accept, info=True)
    return 1e6 * (time.perf_counter() - t0) / (COUNT + 1)  # (one head launch and one recurrence step per drawn byte)


def head(arms=("off", "accept")):
    for K in SHAPES:
        L, u, table, accept = _setup(K)
        for _ in range(2):  # warm-up: both instantiations loaded, scratch grown
            for arm in arms:
                _call(L, K, u, table, accept if arm == "accept" else None)
        us = {arm: [] for arm in arms}
        for rep in range(ROUNDS):
            for arm in arms:
                t = _call(L, K, u, table, accept if arm == "accept" else None)
                us[arm].append(t)
                print(json.dumps({"mode": "head", "hidden": N, "streams": K, "count": COUNT, "arm": arm, "round": rep, "step_us": t}), flush=True)
        L.close()
        off = statistics.median(us["off"])
        line = {"mode": "head_summary", "hidden": N, "streams": K, "count": COUNT, "lib": os.path.basename(lstm_hip.LIB_PATH),
                "off_step_us_median": off, "off_step_us_min": min(us["off"]), "off_step_us_max": max(us["off"])}
        if "accept" in us:
            med = statistics.median(us["accept"])
            line.update({"accept_step_us_median": med, "accept_step_us_min": min(us["accept"]), "accept_step_us_max": max(us["accept"]),
                         "extra_us_per_step": med - off})
        print(json.dumps(line), flush=True)


def compile_times():
    cases = [b"a{4000}", b".{0,4000}", b"a{0,4095}", b"(?:[a-z]{1,8} ){1,40}[a-z]{1,8}\\.", b"(a|b)*abb(a|b){8}", b"[0-9]{3}-[0-9]{4}",
             b"(?:a{1000}){5}", b"[ab]*a[ab]{20}", b"(?:(?:(?:a{1000}){1000}){1000}){1000}", b"(.*a){30}.{30}"]
    for pat in cases:
        best, states, err = None, None, None
        for _ in range(3):
            t0 = time.perf_counter()
            try:
                states = int(lstm_hip.dfa_regex(pat)[0].shape[0])
            except lstm_hip.LstmHipError as e:
                err = str(e).split(": ", 2)[-1]
            dt = 1e3 * (time.perf_counter() - t0)
            best = dt if best is None else min(best, dt)
        print(json.dumps({"mode": "compile", "pattern": pat.decode(), "states": states, "refused": err, "best_ms_of_3": best}), flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "head"
    {"head": head, "plain": lambda: head(("off",)), "compile": compile_times}[mode]()
