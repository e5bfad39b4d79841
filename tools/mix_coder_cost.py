"""What mixed coding costs, and what it buys, one JSON line per figure.

    python tools/mix_coder_cost.py off LABEL    lstm_hip_encode and lstm_hip_decode at hidden 512: 64 streams of 512 bytes, five
                                                repeats
    python tools/mix_coder_cost.py on LABEL     the encoder at hidden 512 with one hidden-128 guide and with one hidden-512
                                                guide, at rate 0 and at rate 0.01, against the unmixed call, three repeats
    python tools/mix_coder_cost.py buys LABEL   trains a hidden-128 and a hidden-512 model as tools/guided_cost.py buys does (1 MB
                                                of tools/make_text.py, the last 20 000 bytes held out), then codes the held-out
                                                bytes with lstm_compress: each model alone, the fixed (0.5, 0.5) mix, and learned
                                                weights from (1, 0) and (0.5, 0.5) at four rates, in one stream and in four

`off` calls nothing the parent commit's library lacks, so LSTM_HIP_LIB=<that library> gives the other arm of the comparison;
alternate the two, a process each.  Per repeat: the wall time of one call with profiling off, then the rows of
Lstm.kernel_stats() from a second call with profiling on.  The lines go to standard output and to DIR/LABEL.jsonl (DIR:
$MIX_CODER_OUT, default the working directory)."""
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "eigen-lstm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

N, NG, K, LEN = 512, (128, 512), 64, 512
ROWS = ("code_head", "code_head_mixed", "guide_logits", "fwd_step", "pack_U")


def _emit(out, line):
    print(json.dumps(line), flush=True)
    out.write(json.dumps(line) + "\n")


def _measure(out, label, case, reps, L, call):
    call()  # warm-up: scratch, LDS grants, code objects
    for r in range(reps):
        L.set_profiling(False)
        L.synchronize()
        t0 = time.perf_counter()
        call()
        wall = (time.perf_counter() - t0) * 1e3
        L.set_profiling(True)
        L.reset_kernel_stats()
        call()
        L.synchronize()
        st = L.kernel_stats()
        L.set_profiling(False)
        line = dict(label=label, case=case, streams=K, steps=LEN, rep=r, wall_ms=round(wall, 3), wall_us_per_step=round(1e3 * wall / LEN, 3))
        for row in ROWS:
            n, ms = st.get(row, (0, 0.0))
            if n:
                line[row + "_launches"] = n
                line[row + "_us_per_launch"] = round(1e3 * ms / n, 3)
        _emit(out, line)


def costs(mode, label, out):
    import lstm_hip
    import sampling_ref as sr
    rs = np.random.RandomState(4)
    texts = [bytes(rs.randint(97, 123, size=LEN).astype(np.uint8)) for _ in range(K)]
    lengths = [LEN] * K
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(sr.peaked_params(N, seed=3, scale=0.1))
    codes = L.encode(texts)[0]
    if mode == "off":
        _measure(out, label, "encode_512", 5, L, lambda: L.encode(texts))
        _measure(out, label, "decode_512", 5, L, lambda: L.decode(codes, lengths))
    else:
        _measure(out, label, "encode_512", 3, L, lambda: L.encode(texts))
        for ng in NG:
            G = lstm_hip.Lstm(ng, 2, 1)
            G.set_params(sr.peaked_params(ng, seed=5, scale=0.1))
            _measure(out, label, f"encode_{ng}_alone", 3, G, lambda: G.encode(texts))
            for rate in (0.0, 0.01):
                _measure(out, label, f"encode_512_guide_{ng}_rate_{rate}", 3, L,
                         lambda: L.encode_mixed(texts, guides=[(G, 0.5)], main_weight=0.5, rate=rate))
            mixed = L.encode_mixed(texts, guides=[(G, 0.5)], main_weight=0.5, rate=0.01)[0]
            _measure(out, label, f"decode_512_guide_{ng}_rate_0.01", 3, L,
                     lambda: L.decode_mixed(mixed, lengths, guides=[(G, 0.5)], main_weight=0.5, rate=0.01))
            G.close()
    L.close()


def buys(label, out):
    lstm, cmp_ = os.path.join(ROOT, "eigen-lstm_amd", "lstm"), os.path.join(ROOT, "eigen-lstm_amd", "lstm_compress")
    with tempfile.TemporaryDirectory() as d:
        whole = os.path.join(d, "whole.txt")
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_text.py"), whole, "1000000"])
        data = open(whole, "rb").read()
        train, held = os.path.join(d, "train.txt"), os.path.join(d, "held.txt")
        open(train, "wb").write(data[:-20000])
        open(held, "wb").write(data[-20000:])
        ck = {}
        for hidden, windows in ((128, 3000), (512, 3000)):
            ck[hidden] = os.path.join(d, f"ck{hidden}")
            t0 = time.perf_counter()
            subprocess.check_call([lstm, "--data", train, "--hidden", str(hidden), "--seq", "50", "--batch", "32", "--lr", "2e-3",
                                   "--optimizer", "adam", "--epochs", "1", "--windows", str(windows), "--sample", "0", "--save",
                                   ck[hidden], "--quiet"], stdout=subprocess.DEVNULL, timeout=900)
            _emit(out, dict(label=label, case="train", hidden=hidden, windows=windows, seconds=round(time.perf_counter() - t0, 1)))

        def code(streams, *args):
            packed, back = os.path.join(d, "x.bin"), os.path.join(d, "x.out")
            res = subprocess.run([cmp_, *args, "--streams", str(streams), "-c", held, packed], capture_output=True, text=True, timeout=600)
            assert res.returncode == 0, res.stderr
            m = re.search(r"code (\d+) bytes in (\d+) streams.*: ([\d.]+) bits/char \(model ([\d.]+) bits/char\)", res.stdout)
            line = dict(code_bytes=int(m.group(1)), streams=int(m.group(2)), bits_per_char=float(m.group(3)), model_bits_per_char=float(m.group(4)))
            finals = re.findall(r"model (\d): weight (\S+), final (\S+) \.\. (\S+)", res.stdout)
            if finals:
                line["final_weights"] = [[float(lo), float(hi)] for _, _, lo, hi in finals]
            keep, skip = [], False
            for a in args:  # -d takes the models only
                if skip:
                    skip = False
                elif a in ("--guide-weight", "--main-weight", "--mix-rate"):
                    skip = True
                else:
                    keep.append(a)
            res = subprocess.run([cmp_, *keep, "-d", packed, back], capture_output=True, text=True, timeout=600)
            assert res.returncode == 0 and open(back, "rb").read() == data[-20000:], res.stderr
            return line

        for streams in (1, 4):
            for hidden in (128, 512):
                _emit(out, dict(label=label, case="alone", hidden=hidden, **code(streams, "--load", ck[hidden])))
            mix = ["--load", ck[512], "--guide", ck[128]]
            _emit(out, dict(label=label, case="fixed", main_weight=0.5, guide_weight=0.5,
                            **code(streams, *mix, "--main-weight", "0.5", "--guide-weight", "0.5")))
            for a, b in ((1.0, 0.0), (0.5, 0.5)):
                for rate in (0.0005, 0.002, 0.008, 0.03):
                    _emit(out, dict(label=label, case="learned", main_weight=a, guide_weight=b, rate=rate,
                                    **code(streams, *mix, "--main-weight", repr(a), "--guide-weight", repr(b), "--mix-rate", repr(rate))))


def main():
    mode, label = sys.argv[1], sys.argv[2]
    where = os.environ.get("MIX_CODER_OUT", ".")
    os.makedirs(where, exist_ok=True)
    with open(os.path.join(where, label + ".jsonl"), "w") as out:
        if mode == "buys":
            buys(label, out)
        else:
            costs(mode, label, out)


if __name__ == "__main__":
    main()
