"""Measures adaptive coding (lstm_hip_encode_adaptive / lstm_hip_decode_adaptive) on one GPU:

  split   how a block's device time divides between the code pass (code_head + fwd_step), the repack (pack_U), the window
          builder (block_window) and the train pass (everything else), from the handle's own kernel stats (HIP-event
          profiling: every launch timed on its own), beside the unprofiled wall time and MB/s of encode and decode
  ratio   the word corpus of tools/make_text.py coded adaptively: total bits/char and by quarter of the blocks, against the
          static coder with the initial parameters, zlib -9 and lzma -9

usage: python tools/adaptive_profile.py OUT_DIR [split|ratio]   (writes OUT_DIR/split.jsonl, OUT_DIR/ratio.jsonl)
"""
import json
import lzma
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "eigen-lstm_amd"))
import lstm_hip  # noqa: E402

STABLE = lstm_hip.STABLE_SOFTMAX
CODE = ("code_head", "fwd_step")
REPACK = ("pack_U",)
WINDOW = ("block_window",)


def word_text(n, seed=11):
    rs = np.random.RandomState(seed)
    words = [bytes(rs.randint(97, 123, size=rs.randint(2, 9)).astype(np.uint8)) for _ in range(400)]
    p = 1.0 / np.arange(1, 401)
    p /= p.sum()
    return b" ".join(words[i] for i in rs.choice(400, size=n // 4 + 1, p=p))[:n]


def handle(N, S, B, flags, clip):
    L = lstm_hip.Lstm(N, S, B, flags=flags)
    L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(1), N))
    if clip:
        L.set_grad_clip(clip)
    return L


def texts_for(S, B, blocks, seed=11):
    n = blocks * (S - 1)
    t = word_text(n * B, seed)
    return [t[s * n:(s + 1) * n] for s in range(B)]


def split(out):
    name, cus, mhz = lstm_hip.device_info(0)
    out.write(json.dumps({"case": "device", "name": name, "cus": cus, "clock_mhz": mhz}) + "\n")
    for N, S, B, blocks in ((512, 100, 64, 30), (128, 26, 8, 200)):
        lr, clip, flags = 0.05, 5.0, STABLE
        texts = texts_for(S, B, blocks)
        nbytes = sum(len(t) for t in texts)
        warm = handle(N, S, B, flags, clip)  # first-use costs (module load, scratch growth) stay out of the timed calls
        warm.encode_adaptive(texts_for(S, B, 2), lr)
        warm.close()
        best = {}
        codes = None
        for _ in range(3):
            E, D = handle(N, S, B, flags, clip), handle(N, S, B, flags, clip)
            t0 = time.perf_counter()
            codes, bits, _ = E.encode_adaptive(texts, lr)
            t1 = time.perf_counter()
            back = D.decode_adaptive(codes, [len(t) for t in texts], lr)
            t2 = time.perf_counter()
            assert back == texts
            plan = E.plan_identity()
            E.close()
            D.close()
            best["encode_s"] = min(best.get("encode_s", 1e9), t1 - t0)
            best["decode_s"] = min(best.get("decode_s", 1e9), t2 - t1)
        P = handle(N, S, B, flags, clip)
        P.set_profiling(True)
        P.reset_kernel_stats()
        P.encode_adaptive(texts, lr)
        stats = P.kernel_stats()
        P.close()
        group = {"code_pass": 0.0, "repack": 0.0, "block_window": 0.0, "train_pass": 0.0}
        for k, (n, ms) in stats.items():
            key = "code_pass" if k in CODE else "repack" if k in REPACK else "block_window" if k in WINDOW else "train_pass"
            group[key] += ms
        total = sum(group.values())
        row = {"case": "split", "N": N, "S": S, "B": B, "blocks": blocks, "bytes": nbytes, "lr": lr, "clip": clip,
               "flags": flags, "plan": plan,
               "encode_s": round(best["encode_s"], 4), "decode_s": round(best["decode_s"], 4),
               "encode_MB_per_s": round(nbytes / best["encode_s"] / 1e6, 4),
               "decode_MB_per_s": round(nbytes / best["decode_s"] / 1e6, 4),
               "encode_ms_per_block": round(1e3 * best["encode_s"] / blocks, 4),
               "profiled_ms_per_block": {k: round(v / blocks, 4) for k, v in group.items()},
               "profiled_share": {k: round(v / total, 4) for k, v in group.items()},
               "kernels": {k: {"launches": n, "us_per_launch": round(1e3 * ms / n, 3)} for k, (n, ms) in stats.items() if n},
               "code_bits_per_char": round(8.0 * sum(len(c) for c in codes) / nbytes, 4)}
        out.write(json.dumps(row) + "\n")
        out.flush()


def ratio(out):
    for N, S, B, blocks, lr, clip in ((128, 26, 8, 240, 0.05, 5.0), (128, 26, 8, 2000, 0.05, 5.0), (512, 100, 64, 160, 0.05, 5.0)):
        texts = texts_for(S, B, blocks)
        raw = b"".join(texts)
        A, T = handle(N, S, B, STABLE, clip), handle(N, S, B, STABLE, clip)
        codes, bits, block_bits = A.encode_adaptive(texts, lr)
        norms = A.grad_norms(blocks)
        s_codes, s_bits = T.encode(texts)
        A.close()
        T.close()
        q = blocks // 4
        per = (S - 1) * B
        row = {"case": "ratio", "N": N, "S": S, "B": B, "blocks": blocks, "bytes": len(raw), "optimizer": "adagrad", "lr": lr,
               "clip": clip, "flags": STABLE, "finite": bool(np.all(np.isfinite(block_bits)) and np.all(np.isfinite(norms))),
               "adaptive_bytes": sum(len(c) for c in codes), "static_initial_bytes": sum(len(c) for c in s_codes),
               "zlib9_bytes": len(zlib.compress(raw, 9)), "lzma9_bytes": len(lzma.compress(raw, preset=9)),
               "bits_per_char_by_quarter": [round(block_bits[i * q:(i + 1) * q].sum() / (q * per), 4) for i in range(4)],
               "max_norm": round(float(norms.max()), 3), "clipped_blocks": int((norms > clip).sum())}
        for k in ("adaptive", "static_initial", "zlib9", "lzma9"):
            row[k + "_bits_per_char"] = round(8.0 * row[k + "_bytes"] / len(raw), 4)
        out.write(json.dumps(row) + "\n")
        out.flush()


if __name__ == "__main__":
    out_dir = sys.argv[1]
    which = sys.argv[2] if len(sys.argv) > 2 else "all"
    os.makedirs(out_dir, exist_ok=True)
    if which in ("split", "all"):
        with open(os.path.join(out_dir, "split.jsonl"), "w") as f:
            split(f)
    if which in ("ratio", "all"):
        with open(os.path.join(out_dir, "ratio.jsonl"), "w") as f:
            ratio(f)
