"""What a weight per target byte costs on the text windows, and what completion-only training buys
(profiles/train_texts_weighted/).  The sibling of tools/train_texts_cost.py.

  python tools/train_texts_weighted_cost.py arm --arm text|weighted --N 512 --S 100 --B 64 [--label NAME] [--out FILE]
      one arm in this process, on the library LSTM_HIP_LIB names (default: this build); ms per window from the HIP-event time
      of the device loop, 20 windows per call, the median of seven calls after one untimed call.  Both arms run
      lstm_hip_train_text_windows on 3B texts of exactly 2 (S - 1) + 1 bytes (two whole windows each, no padded row):
        text       set without weights (the only arm a library without lstm_hip_set_train_texts_weighted can run)
        weighted   set with weights: 0 on the first half of every text, 1 on the second
  python tools/train_texts_weighted_cost.py all --parent-lib PATH [--out profiles/train_texts_weighted/cost.jsonl]
      at (512, 100, 64) and (128, 26, 8): text on the parent commit's library (PATH, through LSTM_HIP_LIB), text and weighted
      on this build, one process each, alternately, three rounds; then one `difference` line per shape: the medians, the
      differences in microseconds and the spread of the parent's own three rounds.
  python tools/train_texts_weighted_cost.py pairs FILE RECORDS [--seed K]
      the synthetic records of `heldout`: "key TAB value NEWLINE", the key four seeded lower-case letters, the value the key
      reversed and shifted three letters on, each of its letters replaced by a seeded random one with probability 0.1.
  python tools/train_texts_weighted_cost.py heldout [--out profiles/train_texts_weighted/heldout.jsonl]
      the point of the feature: `lstm --records` with and without `--train-after 9` on the same records in the same number of
      windows, each saved and loaded again; held-out records scored by Lstm.eval_texts with skip set to the byte after the
      TAB: bits per completion byte, and for comparison bits per prompt byte.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import train_texts_cost as ttc  # noqa: E402  (the corpus, the shapes and the timing constants are its own)

SEP = 9


def pairs(records, seed):
    """`records` byte strings "key\\tvalue\\n" (the module text has the rule)"""
    rs = np.random.RandomState(seed)
    keys = rs.randint(0, 26, size=(records, 4))
    values = (keys[:, ::-1] + 3) % 26
    noise = rs.random_sample(values.shape) < 0.1
    values = np.where(noise, rs.randint(0, 26, size=values.shape), values)
    return [bytes((97 + k).astype(np.uint8)) + b"\t" + bytes((97 + v).astype(np.uint8)) + b"\n" for k, v in zip(keys, values)]


def arm(a):
    import lstm_hip
    N, S, B = a.N, a.S, a.B
    per = 2 * (S - 1) + 1
    text = ttc._corpus(3 * B * per + S + 1)
    L = lstm_hip.Lstm(N, S, B)
    L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(1), N))
    texts = [text[i * per:(i + 1) * per] for i in range(3 * B)]
    weights = None
    if a.arm == "weighted":
        weights = [np.concatenate([np.zeros(per // 2, np.float32), np.ones(per - per // 2, np.float32)]) for _ in texts]
    set_texts = (lambda: L.set_train_texts(texts)) if weights is None else (lambda: L.set_train_texts(texts, weights))
    assert set_texts() == 6

    def call():
        done, ms = 0, 0.0
        while done < ttc.WINDOWS:   # the plan has 6 windows: set again, outside the timed loop
            set_texts()
            k = min(6, ttc.WINDOWS - done)
            ms += L.train_text_windows(k, 0.0, want_losses=False, want_time=True)[1]
            done += k
        return ms / ttc.WINDOWS
    call()
    times = [call() for _ in range(ttc.REPEATS)]
    ttc._emit(dict(case=a.arm, label=a.label, lib=os.environ.get("LSTM_HIP_LIB", "this build"), N=N, S=S, B=B, windows=ttc.WINDOWS,
                   repeats=ttc.REPEATS, ms_per_window_median=round(float(np.median(times)), 4), ms_per_window_min=round(min(times), 4),
                   ms_per_window_max=round(max(times), 4)), a.out)
    L.close()


def everything(a):
    rows = []
    for N, S, B in ttc.SHAPES:
        for _ in range(ttc.ROUNDS):
            for name, lib in (("text", a.parent_lib), ("text", None), ("weighted", None)):
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
                        ttc._emit(row, a.out)

        def rounds(case, label):
            return [r["ms_per_window_median"] for r in rows if (r["case"], r["label"], r["N"], r["S"], r["B"]) == (case, label, N, S, B)]
        parent, text, weighted = rounds("text", "parent"), rounds("text", "branch"), rounds("weighted", "branch")
        pm, tm, wm = float(np.median(parent)), float(np.median(text)), float(np.median(weighted))
        spread = max(parent) - min(parent)
        ttc._emit(dict(case="difference", N=N, S=S, B=B, parent_text_ms=round(pm, 4), branch_text_ms=round(tm, 4),
                       branch_weighted_ms=round(wm, 4), parent_spread_us=round(1e3 * spread, 2),
                       weighted_minus_parent_text_us=round(1e3 * (wm - pm), 2), branch_text_minus_parent_text_us=round(1e3 * (tm - pm), 2),
                       allowance_us=round(1e3 * (spread + 0.01 * pm), 2)), a.out)


def heldout(a):
    N, S, B = a.N, a.S, a.B
    lstm = os.path.join(ROOT, "eigen-lstm_amd", "lstm")
    train, held = pairs(a.records, 11), pairs(a.held, 12)
    skip = [r.index(b"\t") + 1 for r in held]
    completion = sum(len(r) - k for r, k in zip(held, skip))
    prompt = sum(k - 1 for k in skip)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "train.txt")
        with open(path, "wb") as f:
            f.write(b"".join(train))
        for arm_name, extra in (("every byte", []), ("train-after", ["--train-after", str(SEP)])):
            ck = os.path.join(d, "ck_" + arm_name.replace(" ", "_"))
            cmd = [lstm, path, str(N), str(S), str(B), str(a.lr), "--epochs", str(a.epochs), "--seed", "1", "--sample", "0",
                   "--quiet", "--records", "--save", ck] + extra
            out = subprocess.run(cmd, capture_output=True, text=True, errors="replace", timeout=1500)
            if out.returncode != 0:   # nothing more is started on the device after a failed arm
                sys.stderr.write(out.stdout + out.stderr)
                sys.exit(out.returncode)
            lines = [ln for ln in out.stdout.splitlines() if ln.startswith("records:")]
            L = ttc._load(ck, N, S, B)
            whole = L.eval_texts(held)["bits"]
            behind = L.eval_texts(held, skip=skip)["bits"]
            L.close()
            ttc._emit(dict(case="heldout", arm=arm_name, N=N, S=S, B=B, lr=a.lr, epochs=a.epochs, train_records=len(train),
                           heldout_records=len(held), completion_bytes=completion, prompt_bytes=prompt,
                           bits_per_completion_byte=round(float(behind.sum()) / completion, 5),
                           bits_per_prompt_byte=round(float((whole - behind).sum()) / prompt, 5),
                           last_epoch_line=lines[-1] if lines else ""), a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("arm", "all", "pairs", "heldout"))
    ap.add_argument("rest", nargs="*")
    ap.add_argument("--arm", choices=("text", "weighted"), default="weighted")
    ap.add_argument("--N", type=int, default=128)
    ap.add_argument("--S", type=int, default=11)
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--records", type=int, default=20000)
    ap.add_argument("--held", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--label", default="")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.mode == "all" and not a.parent_lib:
        ap.error("all needs --parent-lib")
    if a.mode == "pairs":
        if len(a.rest) != 2:
            ap.error("pairs needs FILE RECORDS")
        with open(a.rest[0], "wb") as f:
            f.write(b"".join(pairs(int(a.rest[1]), a.seed)))
        return
    {"arm": arm, "all": everything, "heldout": heldout}[a.mode](a)


if __name__ == "__main__":
    main()
