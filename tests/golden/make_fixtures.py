#!/usr/bin/env python3
"""Regenerates tests/golden/fixture_{A,B}.npz from the reference's own saved artefacts.

Runs only where /root/reference is mounted (the build container); the .npz files it writes are
committed, so nothing under tests/ reads /root/reference at test time.

The fixtures are DATA the reference produced, not reference source:
  * the five weight matrices its Parameters::save_to_disk wrote as text
    (OV/lstm_eigen_class_CUDA/lstm.h:83-101, io.h:16-32; one matrix row per line, 6 sig. digits),
  * the held-out slice of the corpus its main() evaluates on (last 1 %: lstm.cc:78-86),
  * the bits/char its results log recorded for exactly those weights (column 4 of the 5-column
    log, lstm.cc:205-211).

Fixture A: models/enwik5_test_*  (N=32), R/enwik5.txt bytes [99000,100000), logged 3.24396
Fixture B: models/test4_*        (N=16), R/alice29.txt bytes [150480,152089), logged 2.75851
Flat parameter layout written: [W (4N x M) | U (4N x N) | b | Why (M x N) | by], column-major.

`make_fixtures.py coder [OUT]` writes tests/golden/coder_v1.npz (or OUT) instead: the pinned code of
lstm_hip_coder_version() 1.  It needs an MI355X and the built library, not the reference: four texts
(the first 512 bytes of fixture A's text, an empty one, a one-byte one, 64 random bytes) and the codes and the trace the
device makes of them on fixture A's model.  The fixture is written only if every traced frequency lies in the interval
tests/code_table_ref.py allows for the model's float64 table on the state the byte was coded in.
"""
import os
import sys
import numpy as np

R = "/root/reference"
MODELS = R + "/optimized-obsfuscated_versions/lstm_eigen_class_CUDA/models"
HERE = os.path.dirname(os.path.abspath(__file__))


def load_params(prefix):
    mats = {k: np.loadtxt(f"{MODELS}/{prefix}_{k}.txt", dtype=np.float64, ndmin=2) for k in ("W", "U", "b", "Why", "by")}
    n4, m = mats["W"].shape
    n = n4 // 4
    assert mats["U"].shape == (n4, n) and mats["Why"].shape == (m, n)
    flat = np.concatenate([mats[k].astype(np.float32).flatten(order="F") for k in ("W", "U", "b", "Why", "by")])
    return n, m, flat


def held_out(path):
    data = np.fromfile(path, dtype=np.uint8)
    pct = data.size // 100  # lstm.cc:79
    return data[99 * pct:]  # lstm.cc:84-86 with test_fraction = 1


def logged(path, row):
    return float(np.loadtxt(path, ndmin=2)[row, 3])


def main():
    for name, prefix, corpus, log, row in (
        ("A", "enwik5_test", R + "/enwik5.txt", MODELS + "/enwik5_test.txt", 0),
        ("B", "test4", R + "/alice29.txt", MODELS + "/test4.txt", -1),
    ):
        n, m, flat = load_params(prefix)
        text = held_out(corpus)
        exp = logged(log, row)
        np.savez_compressed(f"{HERE}/fixture_{name}.npz", N=n, M=m, params=flat, text=text, expected_bits=exp)
        print(name, "N", n, "M", m, "params", flat.size, "text", text.size, "expected", exp)


def coder(out):
    root = os.path.dirname(os.path.dirname(HERE))
    sys.path[:0] = [os.path.join(root, "eigen-lstm_amd"), os.path.join(root, "tests")]
    import code_table_ref as ct
    import lstm_hip
    from logits_ref import logits32
    from oracle_lib import split_params
    fx = np.load(f"{HERE}/fixture_A.npz")
    N, P = int(fx["N"]), fx["params"].astype(np.float32)
    texts = [fx["text"][:512].tobytes(), b"", b"\x7f", np.random.RandomState(1).randint(0, 256, size=64).astype(np.uint8).tobytes()]
    L = lstm_hip.Lstm(N, 2, 1)  # (no LSTM_HIP_FAST_MATH)
    L.set_params(P)
    codes, bits, trace = L.encode(texts, trace=True)
    assert L.decode(codes, [len(t) for t in texts]) == texts
    # the interval test on the fixture's own trace: the state before byte j of a text is the generator's after its first j bytes
    where = [(s, j) for s, t in enumerate(texts) for j in range(len(t))]
    prompts = [texts[s][:j] for s, j in where if j]
    H = iter(L.generate(prompts, count=0)[2])
    L.close()
    sp = split_params(P, N)
    Why, by = np.asarray(sp["Why"], np.float32), np.asarray(sp["by"], np.float32).reshape(256)
    for (s, j), (cum, freq, total) in zip(where, trace):
        z = logits32(Why, by, next(H) if j else np.zeros(N, np.float32))
        lo, hi = ct.interval64(z)
        x = texts[s][j]
        assert lo[x] <= int(freq) - 1 <= hi[x], (s, j, x, int(freq), int(lo[x]), int(hi[x]))
    text_off = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.uint64)
    code_off = np.concatenate([[0], np.cumsum([len(c) for c in codes])]).astype(np.uint64)
    np.savez_compressed(out, coder_version=lstm_hip.coder_version(), texts=np.frombuffer(b"".join(texts), np.uint8), text_off=text_off,
                        codes=np.frombuffer(b"".join(codes), np.uint8), code_off=code_off, trace=trace, bits=bits)
    print("coder version", lstm_hip.coder_version(), "texts", [len(t) for t in texts], "codes", [len(c) for c in codes],
          "every traced frequency inside its interval")


if __name__ == "__main__":
    if sys.argv[1:2] == ["coder"]:
        coder(sys.argv[2] if len(sys.argv) > 2 else f"{HERE}/coder_v1.npz")
    else:
        main()
