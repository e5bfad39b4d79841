"""What training on separate texts costs, how full its windows are, and what it buys (profiles/train_texts/; DESIGN.md
section 3.18).

  python tools/train_texts_cost.py arm --arm text|flat --N 512 --S 100 --B 64 [--label NAME] [--out FILE]
      one arm in this process, on the library LSTM_HIP_LIB names (default: this build); ms per window from the HIP-event time
      of the device loop, 20 windows per call, the median of seven calls after one untimed call.
        text   lstm_hip_train_text_windows on 3B texts of exactly 2 (S - 1) + 1 bytes: two whole windows each, no padded row
        flat   lstm_hip_train_windows on the same bytes as one flat text
  python tools/train_texts_cost.py all --parent-lib PATH [--out profiles/train_texts/cost.jsonl]
      at (512, 100, 64) and (128, 26, 8): flat on the parent commit's library (PATH, through LSTM_HIP_LIB), text and flat on
      this build, one process each, alternately, three rounds; then one `ratio` line per shape from the medians.
  python tools/train_texts_cost.py fill [--out profiles/train_texts/fill.jsonl]
      the share of rows filled on a line corpus: 1 MiB of tools/make_text.py with a seeded share of its spaces turned into
      newlines (lines of 40 bytes on average), cut after every newline, placed by lstm_hip_text_plan in corpus order and in a
      shuffled order.  Host only: needs no device.
  python tools/train_texts_cost.py heldout [--out profiles/train_texts/heldout.jsonl]
      the point of the feature: short records (the lines above, 256 KiB to train on, the next 64 KiB held out), one shape,
      the same number of scored bytes per arm; `lstm --records` against the flat `lstm`, each saved and loaded again, the
      held-out records scored each from the zero state by Lstm.eval_texts.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "eigen-lstm_amd"))

SHAPES = ((512, 100, 64), (128, 26, 8))
WINDOWS, REPEATS, ROUNDS = 20, 7, 3
HEAD = 8   # heldout: the bytes at a record's start are reported on their own


def _emit(row, out):
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def _corpus(n):
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "corpus.txt")
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_text.py"), path, str(n)])
        return np.fromfile(path, dtype=np.uint8)


def line_corpus(n, mean=40, seed=3):
    """make_text.py's words with a seeded share of the spaces turned into newlines: lines of `mean` bytes on average"""
    text = _corpus(n).copy()
    spaces = np.flatnonzero(text == 32)
    words_per_line = mean * spaces.size / text.size
    rs = np.random.RandomState(seed)
    text[spaces[rs.random_sample(spaces.size) < 1.0 / words_per_line]] = 10
    return text


def records(text, delim=10):
    cuts = np.flatnonzero(text[:-1] == delim) + 1
    return np.split(text, cuts)


def arm(a):
    import lstm_hip
    N, S, B = a.N, a.S, a.B
    per = 2 * (S - 1) + 1
    text = _corpus(3 * B * per + S + 1)
    L = lstm_hip.Lstm(N, S, B)
    L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(1), N))
    times = []
    if a.arm == "text":
        texts = [text[i * per:(i + 1) * per] for i in range(3 * B)]
        assert L.set_train_texts(texts) == 6 and lstm_hip.text_plan(S - 1, B, [per] * 3 * B)[0] == 6

        def call():
            done = 0
            ms = 0.0
            while done < WINDOWS:   # the plan has 6 windows: set again, outside the timed loop
                L.set_train_texts(texts)
                k = min(6, WINDOWS - done)
                ms += L.train_text_windows(k, 0.0, want_losses=False, want_time=True)[1]
                done += k
            return ms / WINDOWS
    else:
        L.set_text(text)
        L.set_cursors(lstm_hip.initial_cursors(text.size, S, B))
        L.set_stride(S - 1, S - 1)   # the stride of a text window: every byte is a target once

        def call():
            return L.train_windows(WINDOWS, 0.0, want_losses=False, want_time=True)[1] / WINDOWS
    call()
    for _ in range(REPEATS):
        times.append(call())
    _emit(dict(case=a.arm, label=a.label, lib=os.environ.get("LSTM_HIP_LIB", "this build"), N=N, S=S, B=B, windows=WINDOWS,
               repeats=REPEATS, ms_per_window_median=round(float(np.median(times)), 4), ms_per_window_min=round(min(times), 4),
               ms_per_window_max=round(max(times), 4)), a.out)
    L.close()


def everything(a):
    rows = []
    for N, S, B in SHAPES:
        for _ in range(ROUNDS):
            for name, lib in (("flat", a.parent_lib), ("text", None), ("flat", None)):
                env = dict(os.environ)
                env.pop("LSTM_HIP_LIB", None)
                if lib:
                    env["LSTM_HIP_LIB"] = os.path.abspath(lib)
                label = "parent" if lib else "branch"
                cmd = [sys.executable, os.path.abspath(__file__), "arm", "--arm", name, "--N", str(N), "--S", str(S), "--B", str(B),
                       "--label", label]
                done = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
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

        def med(case, label):
            return float(np.median([r["ms_per_window_median"] for r in rows
                                    if (r["case"], r["label"], r["N"], r["S"], r["B"]) == (case, label, N, S, B)]))
        parent, flat, text = med("flat", "parent"), med("flat", "branch"), med("text", "branch")
        _emit(dict(case="ratio", N=N, S=S, B=B, parent_flat_ms=round(parent, 4), branch_flat_ms=round(flat, 4),
                   branch_text_ms=round(text, 4), text_minus_parent_flat_ms=round(text - parent, 4),
                   text_over_parent_flat=round(text / parent, 3), branch_flat_over_parent_flat=round(flat / parent, 3)), a.out)


def fill(a):
    import lstm_hip
    text = line_corpus(1 << 20)
    recs = records(text)
    lens = np.array([r.size for r in recs])
    steps = int(np.maximum(lens - 1, 0).sum())
    _emit(dict(case="corpus", bytes=int(text.size), records=len(recs), mean_bytes=round(float(lens.mean()), 2),
               median_bytes=int(np.median(lens)), max_bytes=int(lens.max())), a.out)
    for S, B in ((26, 8), (50, 32), (100, 64), (100, 256)):
        for order in ("corpus", "shuffled"):
            use = lens if order == "corpus" else np.random.RandomState(5).permutation(lens)
            windows = lstm_hip.text_plan(S - 1, B, use)[0]
            _emit(dict(case="fill", S=S, B=B, order=order, windows=windows, rows=windows * (S - 1) * B, steps=steps,
                       filled=round(steps / (windows * (S - 1) * B), 4)), a.out)


def _load(prefix, N, S, B):
    import lstm_hip
    # the host program's checkpoint: five matrices, one row per line (tests/test_host_driver.py reads them the same way)
    blocks = [np.loadtxt(f"{prefix}_{name}.txt", ndmin=2).astype(np.float32).flatten(order="F") for name in ("W", "U", "b", "Why", "by")]
    L = lstm_hip.Lstm(N, S, B)
    L.set_params(np.concatenate(blocks).astype(np.float32))
    return L


def heldout(a):
    N, S, B = a.N, a.S, a.B
    lstm = os.path.join(ROOT, "eigen-lstm_amd", "lstm")
    text = line_corpus((256 + 64) << 10)
    cut = int(np.flatnonzero(text[:256 << 10] == 10)[-1]) + 1
    train, held = text[:cut], records(text[cut:])[:-1]     # (the last piece may lack its newline)
    held_steps = int(sum(r.size - 1 for r in held))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "train.txt")
        train.tofile(path)
        lens = np.array([r.size for r in records(train)])
        steps = int(np.maximum(lens - 1, 0).sum())
        flat_windows = -(-steps // ((S - 1) * B))          # the same number of scored bytes per epoch
        for arm_name, extra in (("records", ["--records"]),
                                ("flat", ["--stride", str(S - 1), "--windows", str(flat_windows)])):
            ck = os.path.join(d, arm_name)
            cmd = [lstm, path, str(N), str(S), str(B), str(a.lr), "--epochs", str(a.epochs), "--seed", "1", "--sample", "0",
                   "--quiet", "--save", ck] + extra
            out = subprocess.run(cmd, capture_output=True, text=True, errors="replace", timeout=1500)
            if out.returncode != 0:
                sys.stderr.write(out.stdout + out.stderr)
                sys.exit(out.returncode)
            L = _load(ck, N, S, B)
            got = L.eval_texts(held, surprisal=True)
            bits = got["bits"]
            head = [s[1:HEAD + 1] for s in got["surprisal"]]       # the first scored bytes of every record
            whole = L.eval_bits(text[cut:])
            L.close()
            _emit(dict(case="heldout", arm=arm_name, N=N, S=S, B=B, lr=a.lr, epochs=a.epochs, train_bytes=int(train.size),
                       train_records=int(lens.size), scored_bytes_per_epoch=steps, heldout_records=len(held),
                       heldout_scored_bytes=held_steps, heldout_bits_per_char_from_zero=round(float(bits.sum()) / held_steps, 5),
                       heldout_bits_per_char_one_stream=round(float(whole), 5),
                       **{f"heldout_bits_per_char_first_{HEAD}": round(float(np.concatenate(head).sum()) / sum(h.size for h in head), 5)}),
                  a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("arm", "all", "fill", "heldout"))
    ap.add_argument("--arm", choices=("text", "flat"), default="text")
    ap.add_argument("--N", type=int, default=128)
    ap.add_argument("--S", type=int, default=26)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--label", default="")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.mode == "all" and not a.parent_lib:
        ap.error("all needs --parent-lib")
    {"arm": arm, "all": everything, "fill": fill, "heldout": heldout}[a.mode](a)


if __name__ == "__main__":
    main()
