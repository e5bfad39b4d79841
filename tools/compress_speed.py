"""Speed and compression ratio of the model-driven range coder (lstm_hip_encode / lstm_hip_decode).

  python tools/compress_speed.py [--only speed|ratio|one] [--out DIR]

  speed  N in (512, 1024), K in (1, 64, 1024, 4096) streams of `count` bytes (random-init weights): one encode call, one
         decode call (which must give the text back) and, beside them, one lstm_hip_generate scoring call of the same
         texts (the generator's step loop).  Each call runs once untimed first, then three times: the fastest counts.
         us/step = wall time / count.
  ratio  a 1 MB corpus from tools/make_text.py; `lstm` trains N = 512 on the first 900 KB for a fixed number of windows
         (Adagrad lr 0.05 with --stable-softmax and --clip-norm 5, which keep it finite at that rate);
         `lstm_compress` codes the held-out last 100 KB with K = 1 .. 4096 streams and decodes it back (cmp); Python's
         lzma and zlib sizes of the same bytes beside it.
  one    one encode call at N = 512, 64 streams x 500 bytes (for a rocprofv3 --kernel-trace --stats run).
One JSON line per case on stdout and in DIR/speed.jsonl / DIR/ratio.jsonl (DIR default profiles/compress)."""
import argparse
import json
import lzma
import os
import re
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "eigen-lstm_amd")
sys.path.insert(0, PKG)
import lstm_hip  # noqa: E402


def _timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def _best(fn, n=3):
    """the fastest of n runs (and the last result)"""
    runs = [_timed(fn) for _ in range(n)]
    return min(t for t, _ in runs), runs[-1][1]


def speed_case(N, K, count):
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(1), N))
    rs = np.random.RandomState(K)
    texts = [rs.randint(32, 127, size=count).astype(np.uint8) for _ in range(K)]
    warm = [t[:20] for t in texts]
    L.encode(warm)
    te, (codes, bits) = _best(lambda: L.encode(texts))
    L.decode([c[:64] for c in codes], [20] * K)
    td, back = _best(lambda: L.decode(codes, [count] * K))
    L.generate(warm, score=True)
    tg, _ = _best(lambda: L.generate(texts, score=True))
    L.close()
    ok = all(back[s] == texts[s].tobytes() for s in range(K))
    mb = K * count / 1e6
    return dict(case="speed", N=N, streams=K, count=count, encode_s=round(te, 4), decode_s=round(td, 4),
                encode_us_per_step=round(te / count * 1e6, 2), decode_us_per_step=round(td / count * 1e6, 2),
                generate_us_per_step=round(tg / count * 1e6, 2), encode_vs_generate=round(te / tg, 2),
                encode_MB_per_s=round(mb / te, 4), decode_MB_per_s=round(mb / td, 4),
                code_bits_per_char=round(8 * sum(len(c) for c in codes) / (K * count), 4), round_trip=ok)


def ratio_cases(windows, N=512, S=100, B=64, lr=0.05):
    out = []
    with tempfile.TemporaryDirectory() as d:
        corpus = os.path.join(d, "corpus.txt")
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_text.py"), corpus, "1000000"])
        data = open(corpus, "rb").read()
        train, held = data[:900000], data[900000:]
        open(os.path.join(d, "train.txt"), "wb").write(train)
        src = os.path.join(d, "held.txt")
        open(src, "wb").write(held)
        t, r = _timed(lambda: subprocess.run([os.path.join(PKG, "lstm"), os.path.join(d, "train.txt"), str(N), str(S), str(B),
                                              str(lr), "--epochs", "1", "--windows", str(windows), "--seed", "1", "--sample",
                                              "0", "--stable-softmax", "--clip-norm", "5", "--save", os.path.join(d, "ck"),
                                              "--quiet"], capture_output=True, text=True))
        if r.returncode != 0:
            raise RuntimeError(r.stderr)
        out.append(dict(case="model", N=N, S=S, B=B, lr=lr, windows=windows, flags="--stable-softmax --clip-norm 5", train_bytes=len(train), held_out_bytes=len(held),
                        train_s=round(t, 2)))
        out.append(dict(case="baseline", held_out_bytes=len(held), lzma_bytes=len(lzma.compress(held, preset=9)),
                        zlib_bytes=len(zlib.compress(held, 9)),
                        lzma_bits_per_char=round(8 * len(lzma.compress(held, preset=9)) / len(held), 4),
                        zlib_bits_per_char=round(8 * len(zlib.compress(held, 9)) / len(held), 4)))
        exe = os.path.join(PKG, "lstm_compress")
        packed, back = os.path.join(d, "x.lhac"), os.path.join(d, "x.out")
        for K in (None, 1, 4, 16, 64, 256, 1024, 4096):
            extra = [] if K is None else ["--streams", str(K)]
            tc, r = _timed(lambda: subprocess.run([exe, "--load", os.path.join(d, "ck"), "-c", src, packed] + extra,
                                                  capture_output=True, text=True))
            if r.returncode != 0:
                raise RuntimeError(r.stderr)
            m = re.fullmatch(r"in (\d+) bytes, out (\d+) bytes, code (\d+) bytes in (\d+) streams: ([\d.]+) bits/char "
                             r"\(model ([\d.]+) bits/char\)\n", r.stdout)
            tx, r2 = _timed(lambda: subprocess.run([exe, "--load", os.path.join(d, "ck"), "-d", packed, back],
                                                   capture_output=True, text=True))
            same = r2.returncode == 0 and open(back, "rb").read() == held
            out.append(dict(case="ratio", streams=int(m.group(4)), default=K is None, out_bytes=int(m.group(2)),
                            code_bytes=int(m.group(3)), code_bits_per_char=float(m.group(5)),
                            file_bits_per_char=round(8 * int(m.group(2)) / len(held), 5),
                            model_bits_per_char=float(m.group(6)), compress_wall_s=round(tc, 3),
                            decompress_wall_s=round(tx, 3), round_trip=same))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["speed", "ratio", "one"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compress"))
    ap.add_argument("--count", type=int, default=500)
    ap.add_argument("--windows", type=int, default=6000)
    a = ap.parse_args()
    if a.only == "one":
        L = lstm_hip.Lstm(512, 2, 1)
        L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(1), 512))
        rs = np.random.RandomState(1)
        L.encode([rs.randint(32, 127, size=500).astype(np.uint8) for _ in range(64)])
        L.close()
        return
    os.makedirs(a.out, exist_ok=True)
    if a.only in (None, "speed"):
        name, cus, mhz = lstm_hip.device_info(0)
        rows = [dict(case="device", name=name, cus=cus, clock_mhz=mhz)]
        print(json.dumps(rows[0]), flush=True)
        for N in (512, 1024):
            for K in (1, 64, 1024, 4096):
                rows.append(speed_case(N, K, a.count))
                print(json.dumps(rows[-1]), flush=True)
        with open(os.path.join(a.out, "speed.jsonl"), "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)
    if a.only in (None, "ratio"):
        rows = ratio_cases(a.windows)
        for r in rows:
            print(json.dumps(r), flush=True)
        with open(os.path.join(a.out, "ratio.jsonl"), "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)


if __name__ == "__main__":
    main()
