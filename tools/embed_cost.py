"""What lstm_hip_embed_texts costs against lstm_hip_eval_texts on the same streams (profiles/embed/speed.jsonl; DESIGN.md
section 3.23).

  python tools/embed_cost.py arm --arm eval_texts|embed|embed_cell|embed_pick16 --N 512 --lanes 64 [--label NAME] [--out FILE]
      one arm in this process, on the library LSTM_HIP_LIB names (default: this build).  The text is 1 MiB of
      tools/make_text.py, cut into `lanes` streams by eval_split_pieces(pieces = lanes, warm = 0):
        eval_texts    Lstm.eval_texts on those streams with `lanes` lanes: the yardstick
        embed         Lstm.embed_texts, mean + max + last of h
        embed_cell    the same with cell=True: both sources
        embed_pick16  mean + max + last of h, and every 16th position picked
      Each figure is the median of five calls after one untimed call, taken twice (two JSON lines): wall time of the call,
      MB/s over the text's bytes, and the HIP-event time of the device loop per window.
  python tools/embed_cost.py all --parent-lib PATH [--out profiles/embed/speed.jsonl]
      the four arms at N = 512 with 64 lanes and at N = 256 with 32 lanes, one process each, alternately, the whole round
      twice: eval_texts on the parent commit's library (PATH, through LSTM_HIP_LIB), the embed arms on this build; then one
      `ratio` line per shape from the medians of all lines of an arm.
  python tools/embed_cost.py one --N 512 --lanes 64 [--arm embed_cell]
      a single call after an untimed one, for a `rocprofv3 --kernel-trace --stats` run of its own
      (tools/kernel_stats_from_db.py): the share of k_lane_window and k_embed_fold in the window.

The model is the seeded initialisation: speed does not depend on the weights."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "eigen-lstm_amd"))

SHAPES = ((512, 64), (256, 32))  # (N, lanes)
ARMS = ("eval_texts", "embed", "embed_cell", "embed_pick16")
TEXT_BYTES = 1 << 20
REPEATS, ROUNDS = 5, 2


def _text():
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "corpus.txt")
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_text.py"), path, str(TEXT_BYTES)])
        return np.fromfile(path, dtype=np.uint8)


def _median(call):
    call()
    times = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    return float(np.median(times))


def _emit(row, out):
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def _call(L, name, streams, lanes, total):
    if name == "eval_texts":
        return lambda: L.eval_texts(streams, lanes=lanes, want_time=True)["ms"]
    kw = dict(lanes=lanes, want_time=True, cell=name == "embed_cell")
    if name == "embed_pick16":
        kw["pick"] = np.arange(15, total, 16, dtype=np.uint64)
    return lambda: L.embed_texts(streams, **kw)["ms"]


def _setup(N, lanes):
    import lstm_hip
    text = _text()
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(1), N))
    streams = [text[s:e] for s, e, _ in lstm_hip.eval_split_pieces(text.size, lanes)]
    return L, streams, sum(len(s) for s in streams)


def arm(a):
    L, streams, total = _setup(a.N, a.lanes)
    short = 1 if a.arm == "eval_texts" else 0  # eval_texts has ceil((L - 1) / 128) windows per stream, embed_texts ceil(L / 128)
    windows = max(-(-(len(s) - short) // 128) for s in streams)
    loop_ms = []
    inner = _call(L, a.arm, streams, a.lanes, total)

    def call():
        loop_ms.append(inner())
    for rnd in range(ROUNDS):
        del loop_ms[:]
        t = _median(call)
        ms = float(np.median(loop_ms[1:]))
        _emit(dict(case=a.arm, label=a.label, lib=os.environ.get("LSTM_HIP_LIB", "this build"), N=a.N, lanes=a.lanes, round=rnd,
                   text_bytes=total, repeats=REPEATS, seconds_median=round(t, 6), MB_per_s=round(total / t / 1e6, 3),
                   device_loop_ms_median=round(ms, 3), windows=windows, us_per_window=round(1e3 * ms / windows, 2)), a.out)
    L.close()


def everything(a):
    rows = []
    for N, lanes in SHAPES:
        for _ in range(2):
            for name in ARMS:
                lib = a.parent_lib if name == "eval_texts" else None
                env = dict(os.environ)
                env.pop("LSTM_HIP_LIB", None)
                if lib:
                    env["LSTM_HIP_LIB"] = os.path.abspath(lib)
                cmd = [sys.executable, os.path.abspath(__file__), "arm", "--arm", name, "--N", str(N), "--lanes", str(lanes),
                       "--label", "parent" if lib else "branch"]
                done = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
                if done.returncode != 0:   # nothing more is started on the device after a failed arm
                    sys.stderr.write(done.stdout + done.stderr)
                    sys.exit(done.returncode)
                for line in done.stdout.splitlines():
                    if line.startswith("{"):
                        row = json.loads(line)
                        if lib:
                            row["lib"] = "parent commit"
                        rows.append(row)
                        _emit(row, a.out)
        here = [r for r in rows if r["N"] == N]
        mbs = {name: float(np.median([r["MB_per_s"] for r in here if r["case"] == name])) for name in ARMS}
        usw = {name: float(np.median([r["us_per_window"] for r in here if r["case"] == name])) for name in ARMS}
        _emit(dict(case="ratio", N=N, lanes=lanes, MB_per_s=mbs, us_per_window=usw,
                   window_us_over_eval_texts={k: round(usw[k] - usw["eval_texts"], 2) for k in ARMS[1:]}), a.out)


def one(a):
    L, streams, total = _setup(a.N, a.lanes)
    call = _call(L, a.arm, streams, a.lanes, total)
    call()
    print(json.dumps(dict(case="one", arm=a.arm, N=a.N, lanes=a.lanes, ms=call())))
    L.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("arm", "all", "one"))
    ap.add_argument("--arm", choices=ARMS, default="embed")
    ap.add_argument("--N", type=int, default=512)
    ap.add_argument("--lanes", type=int, default=64)
    ap.add_argument("--label", default="")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.mode == "all" and not a.parent_lib:
        ap.error("all needs --parent-lib")
    {"arm": arm, "all": everything, "one": one}[a.mode](a)


if __name__ == "__main__":
    main()
