"""What lstm_hip_embed_texts buys a user who wants a feature vector per record (the line goes to
profiles/embed/probe.jsonl).  Nothing asserts the figures.

  python tools/embed_probe.py [--out FILE] [--windows 2000] [--seed 1]

Synthetic two-class records: a record is 8 to 20 two-letter tokens separated by spaces and ended by a newline.  Class 0
draws its tokens from ab cd ef gh, class 1 from the same letters in the other order, ba dc fe hg; one token in five comes
from the other class.  Both classes have the same byte histogram in expectation: what tells them apart is the order of
bytes.  A hidden-128 model is trained on the unlabelled records as one text (Adagrad, `--windows` windows of 64 x 16), then
a NumPy logistic probe is fitted on 600 labelled records and scored on 300 held-out ones, once on the `concat` embedding
(last, max, mean of h: 384 floats) of Lstm.embed_texts and once on the records' byte histograms (256 floats)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "eigen-lstm_amd"))

TOKENS = (("ab", "cd", "ef", "gh"), ("ba", "dc", "fe", "hg"))
N, S, B, LR = 128, 65, 16, 0.1
TRAIN, TEST, UNLABELLED = 600, 300, 3000


def records(rs, count):
    labels = rs.randint(0, 2, size=count)
    out = []
    for y in labels:
        toks = [TOKENS[y if rs.rand() >= 0.2 else 1 - y][rs.randint(4)] for _ in range(rs.randint(8, 21))]
        out.append((" ".join(toks) + "\n").encode())
    return out, labels


def probe(xtr, ytr, xte, yte, steps=500, lr=0.5, l2=1e-3):
    """logistic regression by full-batch gradient descent on standardised features; held-out accuracy"""
    mu, sd = xtr.mean(0), xtr.std(0) + 1e-6
    xtr, xte = (xtr - mu) / sd, (xte - mu) / sd
    w, b = np.zeros(xtr.shape[1]), 0.0
    for _ in range(steps):
        p = 1.0 / (1.0 + np.exp(-(xtr @ w + b)))
        g = p - ytr
        w -= lr * (xtr.T @ g / len(ytr) + l2 * w)
        b -= lr * g.mean()
    return float((((xte @ w + b) > 0) == (yte > 0)).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--windows", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    import lstm_hip
    rs = np.random.RandomState(a.seed)
    corpus, _ = records(rs, UNLABELLED)
    labelled, y = records(rs, TRAIN + TEST)
    text = np.frombuffer(b"".join(corpus), np.uint8)
    L = lstm_hip.Lstm(N, S, B)
    L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(a.seed), N))
    L.set_text(text)
    L.set_cursors(lstm_hip.initial_cursors(len(text), S, B))
    losses = L.train_windows(a.windows, LR)
    r = L.embed_texts(labelled, lanes=64, want_time=True)
    L.close()
    emb = np.concatenate([r["last_h"], r["max_h"], r["mean_h"]], axis=1).astype(np.float64)
    hist = np.stack([np.bincount(np.frombuffer(t, np.uint8), minlength=256) / len(t) for t in labelled]).astype(np.float64)
    yf = y.astype(np.float64)
    row = dict(case="probe", N=N, windows=a.windows, seed=a.seed, train=TRAIN, test=TEST,
               bits_per_char_last_window=round(float(losses[-1]) / (S - 1), 4), embed_ms=round(r["ms"], 3),
               accuracy_embedding=probe(emb[:TRAIN], yf[:TRAIN], emb[TRAIN:], yf[TRAIN:]),
               accuracy_last_only=probe(emb[:TRAIN, :N], yf[:TRAIN], emb[TRAIN:, :N], yf[TRAIN:]),
               accuracy_byte_histogram=probe(hist[:TRAIN], yf[:TRAIN], hist[TRAIN:], yf[TRAIN:]))
    line = json.dumps(row)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
