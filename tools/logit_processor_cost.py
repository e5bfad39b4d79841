"""What the logit processors cost: hidden 512, 1024 streams of an 8-byte prompt, tempered draws under
top-k 40 and nucleus 0.9 (gen_head's FILTER instantiation), one JSON line per repeat.

    python tools/logit_processor_cost.py off LABEL    the filtered call with processors off, 256 draws, three repeats
    python tools/logit_processor_cost.py on LABEL     then bias alone, min-p alone, no_repeat_ngram = 8 at 256 and at 4096 draws
                                                      against the same call with processors off, and 256 draws behind histories
                                                      of 1024, 4096 and 16384 bytes

`off` calls nothing the parent commit's library lacks, so LSTM_HIP_LIB=<that library> gives the other arm of the comparison;
alternate the two, a process each.  Per repeat: the wall time of one Lstm.generate call with profiling off (the call ends in a
stream synchronise), then the gen_head and fwd_step rows of Lstm.kernel_stats() from a second call with profiling on.  The
lines go to standard output and to DIR/LABEL.jsonl (DIR: $LOGIT_PROCESSOR_OUT, default the working directory)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "eigen-lstm_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import lstm_hip
import sampling_ref as sr

N, K = 512, 1024
FILT = dict(temperature=0.8, top_k=40, top_p=0.9)


def main():
    mode, label = sys.argv[1], sys.argv[2]
    P = sr.peaked_params(N, seed=3, scale=0.1)
    rs = np.random.RandomState(4)
    prompts = [rs.randint(97, 123, size=8).astype(np.uint8) for _ in range(K)]
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(P)
    where = os.environ.get("LOGIT_PROCESSOR_OUT", ".")
    os.makedirs(where, exist_ok=True)
    out = open(os.path.join(where, label + ".jsonl"), "w")

    def measure(name, count, u, reps, **kw):
        L.generate(prompts, count=count, u=u, info=True, **FILT, **kw)  # warm-up: scratch, LDS grants, code objects
        for r in range(reps):
            L.set_profiling(False)
            L.synchronize()
            t0 = time.perf_counter()
            L.generate(prompts, count=count, u=u, info=True, **FILT, **kw)
            wall = (time.perf_counter() - t0) * 1e3
            L.set_profiling(True)
            L.reset_kernel_stats()
            L.generate(prompts, count=count, u=u, info=True, **FILT, **kw)
            L.synchronize()
            st = L.kernel_stats()
            n, ms = st["gen_head"]
            line = dict(label=label, case=name, hidden=N, streams=K, draws=count, rep=r, wall_ms=round(wall, 3),
                        gen_head_launches=n, gen_head_ms=round(ms, 4), gen_head_us_per_step=round(1e3 * ms / n, 3),
                        fwd_step_ms=round(st.get("fwd_step", (0, 0.0))[1], 4))
            print(json.dumps(line), flush=True)
            out.write(json.dumps(line) + "\n")
        L.set_profiling(False)

    u256 = rs.random_sample((256, K))
    if mode == "off":
        measure("filtered_off", 256, u256, 3)
    else:
        bias = (rs.randn(256) * 0.5).astype(np.float32)
        u4096 = rs.random_sample((4096, K))
        measure("filtered_off", 256, u256, 2)
        measure("bias", 256, u256, 2, logit_bias=bias)
        measure("min_p_0.05", 256, u256, 2, min_p=0.05)
        measure("no_repeat_8", 256, u256, 2, no_repeat_ngram=8)
        measure("filtered_off", 4096, u4096, 1)
        measure("no_repeat_8", 4096, u4096, 1, no_repeat_ngram=8)
        for hist in (1024, 4096, 16384):  # how gen_head grows with the text: the same 256 draws behind longer histories
            histories = [rs.randint(97, 123, size=hist).astype(np.uint8) for _ in range(K)]
            measure(f"no_repeat_8_history_{hist}", 256, u256, 1, no_repeat_ngram=8, history=histories)
    L.close()


if __name__ == "__main__":
    main()
