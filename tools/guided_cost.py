"""What guided generation and scoring cost, and what they buy, one JSON line per figure.

    python tools/guided_cost.py off LABEL     the unguided generator and scorer at hidden 512: 64 streams, 512 drawn bytes at
                                              temperature 0.8 / 64 texts of 512 bytes, five repeats
    python tools/guided_cost.py on LABEL      the generator at hidden 512 with one hidden-512 guide and with one hidden-128
                                              guide, weights (1.5, -0.5), against the unguided call of the main model and of
                                              each guide alone, three repeats
    python tools/guided_cost.py buys LABEL    trains a hidden-128 and a hidden-512 model on a 1 MB tools/make_text.py corpus
                                              (window 50, batch 32, Adam at 2e-3, the last 20 000 bytes held out), then through
                                              lstm_generate: held-out bits/char of each alone and of their mixes, and the
                                              4-gram repetition rate of greedy samples with and without --guidance 0.5

`off` calls nothing the parent commit's library lacks, so LSTM_HIP_LIB=<that library> gives the other arm of the comparison;
alternate the two, a process each.  Per repeat: the wall time of one call with profiling off (the call ends in a stream
synchronise), then the rows of Lstm.kernel_stats() from a second call with profiling on.  The lines go to standard output and
to DIR/LABEL.jsonl (DIR: $GUIDED_OUT, default the working directory)."""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "eigen-lstm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

N, NG, K, DRAWS = 512, (512, 128), 64, 512
ROWS = ("gen_head", "score_head", "fwd_step", "guide_logits", "pack_U")


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
        line = dict(label=label, case=case, streams=K, steps=DRAWS, rep=r, wall_ms=round(wall, 3), wall_us_per_step=round(1e3 * wall / DRAWS, 3))
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
    u = rs.random_sample((DRAWS, K))
    texts = [rs.randint(97, 123, size=DRAWS).astype(np.uint8) for _ in range(K)]
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(sr.peaked_params(N, seed=3, scale=0.1))
    if mode == "off":
        _measure(out, label, "generate_512", 5, L, lambda: L.generate(count=DRAWS, u=u, temperature=0.8, streams=K))
        _measure(out, label, "score_512", 5, L, lambda: L.score(texts))
    else:
        _measure(out, label, "generate_512", 3, L, lambda: L.generate(count=DRAWS, u=u, temperature=0.8, streams=K))
        _measure(out, label, "generate_512_processed", 3, L,
                 lambda: L.generate(count=DRAWS, u=u, temperature=0.8, streams=K, logit_bias=np.zeros(256, np.float32)))
        for ng in NG:
            G = lstm_hip.Lstm(ng, 2, 1)
            G.set_params(sr.peaked_params(ng, seed=5, scale=0.1))
            _measure(out, label, f"generate_{ng}_alone", 3, G, lambda: G.generate(count=DRAWS, u=u, temperature=0.8, streams=K))
            _measure(out, label, f"generate_512_guide_{ng}", 3, L,
                     lambda: L.generate(count=DRAWS, u=u, temperature=0.8, streams=K, guides=[(G, -0.5)], main_weight=1.5))
            _measure(out, label, f"score_512_guide_{ng}", 3, L, lambda: L.score_guided(texts, [(G, 0.5)], 0.5))
            G.close()
        _measure(out, label, "score_512", 3, L, lambda: L.score(texts))
    L.close()


def _repeat_rate(text, n=4):
    """the share of the text's n-grams that the text already held"""
    seen, again = set(), 0
    for j in range(len(text) - n + 1):
        g = text[j:j + n]
        again += g in seen
        seen.add(g)
    return again / max(len(text) - n + 1, 1)


def buys(label, out):
    lstm, gen = os.path.join(ROOT, "eigen-lstm_amd", "lstm"), os.path.join(ROOT, "eigen-lstm_amd", "lstm_generate")
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

        def score(*args):
            res = subprocess.run([gen, *args, "--score", held], capture_output=True, text=True, timeout=600)
            assert res.returncode == 0, res.stderr
            return float(res.stdout.split("\n")[0].split(": ")[1].split(" ")[0])

        for hidden in (128, 512):
            _emit(out, dict(label=label, case="heldout_alone", hidden=hidden, bits_per_char=score("--load", ck[hidden])))
        for a in (0.5, 0.6, 0.7, 0.8, 0.9, 1.2, 1.5):  # the hidden-512 model's weight; the hidden-128 guide takes 1 - a
            bits = score("--load", ck[512], "--guide", ck[128], "--guide-weight", repr(round(1.0 - a, 3)), "--main-weight", repr(a))
            _emit(out, dict(label=label, case="heldout_mix", main=512, guide=128, main_weight=a, guide_weight=round(1.0 - a, 3),
                            bits_per_char=bits))

        def samples(*args):  # greedy: one stream per prime, eight primes from the held-out text
            got = []
            for i in range(8):
                prime = data[-20000 + 2000 * i:][:40].decode()
                res = subprocess.run([gen, "--load", ck[512], "--count", "400", "--prime", prime, "--temperature", "0", *args],
                                     capture_output=True, timeout=600)
                assert res.returncode == 0, res.stderr
                got.append(res.stdout.split(b" ==\n", 1)[1][40:-1])
            return got

        for case, args in (("greedy", []), ("greedy_guidance_0.5", ["--guidance", "0.5"]), ("greedy_guidance_1.5", ["--guidance", "1.5"])):
            got = samples(*args)
            _emit(out, dict(label=label, case=case, hidden=512, streams=len(got), drawn=len(got[0]),
                            repeat_rate_4gram=round(float(np.mean([_repeat_rate(t) for t in got])), 4),
                            distinct_samples=len(set(got))))


def main():
    mode, label = sys.argv[1], sys.argv[2]
    where = os.environ.get("GUIDED_OUT", ".")
    os.makedirs(where, exist_ok=True)
    with open(os.path.join(where, label + ".jsonl"), "w") as out:
        if mode == "buys":
            buys(label, out)
        else:
            costs(mode, label, out)


if __name__ == "__main__":
    main()
