"""What lstm_hip_eval_texts costs against the two older ways to score a held-out text (profiles/eval/speed.jsonl; DESIGN.md
section 3.17).

  python tools/eval_cost.py arm --arm eval_texts|score|eval_bits --N 512 --lanes 64 [--label NAME] [--out FILE]
      one arm in this process, on the library LSTM_HIP_LIB names (default: this build).  The text is 1 MiB of
      tools/make_text.py, cut by eval_split_pieces(pieces = lanes, warm = 0):
        eval_texts  Lstm.eval_texts on those streams with `lanes` lanes (wall time of the call, and the HIP-event time of its
                    device loop)
        score       lstm_hip_score asked for surprisal only, on the same streams
        eval_bits   lstm_hip_eval_bits on the first 64 KiB (one stream; MB/s does not depend on the length)
      Each figure is the median of five calls after one untimed call, taken twice (two JSON lines).
  python tools/eval_cost.py all --parent-lib PATH [--out profiles/eval/speed.jsonl]
      the three arms at N = 512 with 64 lanes and at N = 256 with 32 lanes, one process each, alternately, the whole round
      twice: eval_texts on this build, score and eval_bits on the parent commit's library (PATH, through LSTM_HIP_LIB); then
      one `ratio` line per shape from the medians of all lines of an arm.
  python tools/eval_cost.py one --N 512 --lanes 64
      a single eval_texts call after an untimed one, for a `rocprofv3 --kernel-trace --stats` run of its own
      (tools/kernel_stats_from_db.py): the share of k_lane_window and k_eval_fold in the window.

MB/s counts the scored bytes (1 MiB - 1, or 64 KiB - 1) over the wall time of the call, which ends in a stream synchronise and
includes the uploads.  The model is the seeded initialisation: speed does not depend on the weights."""
import argparse
import ctypes as C
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
TEXT_BYTES = 1 << 20
EVAL_BITS_BYTES = 1 << 16
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


def arm(a):
    import lstm_hip
    N, lanes = a.N, a.lanes
    text = _text()
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(1), N))
    streams = [text[s:e] for s, e, _ in lstm_hip.eval_split_pieces(text.size, lanes)]
    loop_ms = []
    if a.arm == "eval_texts":
        scored = text.size - 1

        def call():
            loop_ms.append(L.eval_texts(streams, lanes=lanes, want_time=True)["ms"])
    elif a.arm == "score":
        scored = text.size - 1
        data, off = lstm_hip._offsets(lstm_hip._bytes_list(streams))
        sur = np.zeros(data.size, np.float32)
        opt = lstm_hip._Scoring(C.sizeof(lstm_hip._Scoring), 0, 0, None)
        out = lstm_hip._Scores(C.sizeof(lstm_hip._Scores), lstm_hip._ptr(sur), None, None, None, None, None, None)

        def call():
            lstm_hip._chk(L.lib.lstm_hip_score(L._h, C.c_int32(len(streams)), lstm_hip._ptr(data, C.c_uint8),
                                               lstm_hip._ptr(off, C.c_uint64), None, None, C.byref(opt), None, C.byref(out), None, None))
    else:
        scored = EVAL_BITS_BYTES - 1
        short = np.ascontiguousarray(text[:EVAL_BITS_BYTES])

        def call():
            L.eval_bits(short)
    for rnd in range(ROUNDS):
        del loop_ms[:]
        t = _median(call)
        row = dict(case=a.arm, label=a.label, lib=os.environ.get("LSTM_HIP_LIB", "this build"), N=N, lanes=lanes, round=rnd,
                   scored_bytes=scored, repeats=REPEATS, seconds_median=round(t, 6), MB_per_s=round(scored / t / 1e6, 3))
        if loop_ms:
            row["device_loop_ms_median"] = round(float(np.median(loop_ms[1:])), 3)
        _emit(row, a.out)
    L.close()


def everything(a):
    rows = []
    for N, lanes in SHAPES:
        for _ in range(2):
            for name, lib in (("eval_texts", None), ("score", a.parent_lib), ("eval_bits", a.parent_lib)):
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
        med = {name: float(np.median([r["MB_per_s"] for r in rows if r["case"] == name and r["N"] == N]))
               for name in ("eval_texts", "score", "eval_bits")}
        _emit(dict(case="ratio", N=N, lanes=lanes, MB_per_s=med, eval_texts_over_score=round(med["eval_texts"] / med["score"], 2),
                   eval_texts_over_eval_bits=round(med["eval_texts"] / med["eval_bits"], 2)), a.out)


def one(a):
    import lstm_hip
    text = _text()
    L = lstm_hip.Lstm(a.N, 2, 1)
    L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(1), a.N))
    streams = [text[s:e] for s, e, _ in lstm_hip.eval_split_pieces(text.size, a.lanes)]
    L.eval_texts(streams, lanes=a.lanes)
    print(json.dumps(dict(case="one", N=a.N, lanes=a.lanes, ms=L.eval_texts(streams, lanes=a.lanes, want_time=True)["ms"])))
    L.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("arm", "all", "one"))
    ap.add_argument("--arm", choices=("eval_texts", "score", "eval_bits"), default="eval_texts")
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
