#!/usr/bin/env python3
"""bench.py -- chars/sec through forward + BPTT + Adagrad on the BASELINE headline workload.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A "step" is one training window: slide, forward over S-1 timesteps, loss, BPTT, [RCCL all-reduce of
the flat gradient block], Adagrad -- everything the reference's i-loop does per iteration
(OV/lstm_eigen_opt/lstm.cc:186-318).  Workload = BASELINE.json configs[2] (the config the metric is
quoted on): hidden 512, window 100, batch 64 per GPU, fp32.  The corpus is synthetic (1e6 bytes drawn
with enwik6's order-0 byte statistics): the reference's corpora are not part of this repository and the
throughput is content-independent.  For N > 1 the driver launches one rank per GPU with
torch.distributed.run (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_PORT from the env).  The ranks exchange only
the RCCL id, barriers and a few doubles, over dp.Rendezvous (plain sockets): the GPU processes do not import
torch, so the library's HIP runtime and RCCL are the only copies mapped.  The data path is the C-ABI library
and RCCL inside it.

A plain run does what the headline figure needs: set-up, --sustained-seconds of windows to bring the GPU to its
operating clocks, the W warm-up and the K timed windows from the seeded initial state, and ONE JSON line on rank 0
(see the task contract).  --dump-outputs DIR writes what the last timed window left behind (see dump_outputs).
--full adds the measurements that take runs of their own:
  sustained    : the clock warm-up leg timed as a measurement of its own (at least K windows)
  roofline     : the dominant kernel's algorithmic FLOP per launch / its HIP-event-timed duration
  kernels_us   : every kernel's HIP-event time, in a profiling pass after the timed windows
  cpu_baseline : the CPU oracle (oracle/, a port of the reference's loop) timed on this host
"""
import argparse
import json
import os
import sys
import time

import numpy as np

# multi-process GPU work on this pool needs dmabuf IPC (RCCL's hipIpcGetMemHandle fails otherwise); set before HIP loads
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "eigen-lstm_amd"))
if os.environ.get("LSTM_BENCH_FAKE_GPU") == "1":  # CPU test of the multi-rank plumbing only (tests/fake_gpu)
    sys.path.insert(0, os.path.join(ROOT, "tests", "fake_gpu"))

METRIC = "chars/sec fwd+BPTT, enwik6 H=512 S=100 B=64, 1/2/4/8 GPU"
PEAK_FP32_MFMA_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 / 16x16x4_f32 dense peak

# BASELINE.json `configs`, by index.  The corpora are synthetic stand-ins of the named file's length (enwik6's order-0
# byte statistics): the reference's corpora are not part of this repository, enwik7 is absent even from the reference
# (SURVEY 8d), and the throughput does not depend on the content.  configs[3] is configs[2] under `--gpus 8` (the
# driver's run).
CONFIGS = {
    0: dict(label="configs[0]: alice29.txt, hidden=128 seq=25 batch=1, fp32 (the `lstm.cc as-is` row)", N=128, S=25, B=1,
            nbytes=152_089, corpus="alice29"),
    1: dict(label="configs[1]: enwik5.txt, hidden=256 seq=50 batch=32, fp32", N=256, S=50, B=32, nbytes=100_000,
            corpus="enwik5"),
    2: dict(label="configs[2] (headline): enwik6.txt, hidden=512 seq=100 batch=64, fp32", N=512, S=100, B=64,
            nbytes=1_000_000, corpus="enwik6"),
    3: dict(label="configs[3]: enwik6.txt, hidden=512 seq=100 batch=512 sharded 8 ways (64/GPU), fp32", N=512, S=100, B=64,
            nbytes=1_000_000, corpus="enwik6"),
    4: dict(label="configs[4]: enwik7.txt, hidden=1024 seq=100 batch=128 over 8 GPUs (16/GPU), bf16 MFMA path", N=1024,
            S=100, B=16, nbytes=10_000_000, corpus="enwik7", bf16=True),
}


def synthetic_text(n_bytes, seed=0):
    hist = json.load(open(os.path.join(ROOT, "bench_data", "enwik6_byte_hist.json")))["counts"]
    p = np.asarray(hist, np.float64)
    p /= p.sum()
    return np.random.RandomState(seed).choice(256, size=n_bytes, p=p).astype(np.uint8)


def kernel_flops(N, S, B, M=256, fused=True):
    """algorithmic FLOP per launch of each MFMA kernel (one-hot structure exploited).
    fused: the backward recurrence also computes Why^T*dy and dy*h^T (R/lstm.cc:226,228) itself."""
    T = (S - 1) * B
    return {
        "fwd_step": 2.0 * 4 * N * N * B,                       # U * h_prev           R/lstm.cc:176
        "bwd_step": 2.0 * 4 * N * N * B * (S - 2) / (S - 1),   # U^T * dg (none at t = S-1)  :255
        "gemm_Y": 2.0 * M * N * T,                             # Why * h              :195
        "gemm_DHy": 2.0 * M * N * T,                           # Why^T * dy           :228
        "gemm_dWhy": 2.0 * M * N * T,                          # dy * h^T             :226
        "gemm_dU": 2.0 * 4 * N * N * T,                        # dg * h_prev^T        :250
        "fwd_persistent": 2.0 * 4 * N * N * B * (S - 1),
        "bwd_persistent": 2.0 * 4 * N * N * B * (S - 2) + (4.0 * M * N * T if fused else 0.0),
    }


def pmc_traffic(kernel, N, S, B, dtype):
    """HBM bytes per launch of `kernel` at THIS shape from the committed rocprofv3 PMC passes (separate --pmc FETCH_SIZE /
    WRITE_SIZE runs of this bench, gfx950 x2 read correction applied; tools/pmc_traffic.py).  PMC collection cannot run
    inside this process, so the figure is the recorded one; None for a shape (or kernel) that was not collected."""
    key = f"{N}x{S}x{B}_{dtype}"
    try:
        d = json.load(open(os.path.join(ROOT, "profiles", "r3_pmc_traffic.json")))
        return d["shapes"][key]["kernels"][kernel]["hbm_bytes_per_launch"]
    except Exception:
        pass
    if key == "512x100x64_f32":  # earlier rounds collected the headline shape only (same recurrence kernels)
        for name in ("r2_pmc_traffic.json", "r1_pmc_traffic.json"):
            try:
                d = json.load(open(os.path.join(ROOT, "profiles", name)))
                return d["kernels"][kernel]["hbm_bytes_per_launch"]
            except Exception:
                continue
    return None


def _time_oracle(kind, N, S, B, text, lr, budget_s):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle_lib import Oracle
    tr = Oracle(kind).trainer(text, N, S, B, lr=lr, seed=1)
    tr.epoch_reset()
    tr.window()  # warm caches / page in
    n, t0 = 0, time.perf_counter()
    while True:
        tr.window()
        n += 1
        dt = time.perf_counter() - t0
        if dt > budget_s or n >= 50:
            break
    return (S - 1) * B * n / dt, n, dt


def cpu_baseline(N, S, B, text, lr, budget_s=20.0):
    """The oracle's trainer (a port of the reference loop) on this host: 1 thread (the reference Makefile has no
    -fopenmp, R/Makefile:10) on a bounded sample, plus the same code with OpenMP over the GEMM loops on all cores as the
    generous figure."""
    v1, n1, dt1 = _time_oracle("f32", N, S, B, text, lr, budget_s)
    out = {"value": v1, "unit": "chars/s", "cores": 1, "kind": "port",
           "sample": f"{n1} window(s) of the same workload (N={N} S={S} B={B}) in {dt1:.1f} s, "
                     "oracle/lstm_ref.c -O3 -march=native, single thread like the reference build"}
    try:
        vo, no, dto = _time_oracle("f32_omp", N, S, B, text, lr, budget_s / 2)  # OMP_NUM_THREADS = this process's CPU share
        out["all_cores"] = {"value": vo, "cores": int(os.environ["OMP_NUM_THREADS"]),
                            "sample": f"{no} window(s) in {dto:.1f} s, same source with -fopenmp"}
    except Exception as e:  # the generous figure is optional; the single-thread one above is the baseline
        out["all_cores"] = {"error": str(e)}
    return out


MAX_DUMP_BYTES = 60 << 20  # the files of --dump-outputs stay under 64 MB


def dump_outputs(d, arrays):
    """--dump-outputs: each array as DIR/<name>.npy (float32 / float64).  If together they exceed MAX_DUMP_BYTES, each is
    cut to a fixed, seeded sample of its flat elements: one element from every run of `step`, in index order."""
    os.makedirs(d, exist_ok=True)
    step = -(-sum(a.nbytes for a in arrays.values()) // MAX_DUMP_BYTES)
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        if step > 1:
            k = max(1, a.size // step)
            a = a.ravel()[np.arange(k) * step + np.random.RandomState(0).randint(0, min(step, a.size), k)]
        np.save(os.path.join(d, name + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--config", type=int, default=2, choices=sorted(CONFIGS),
                    help="BASELINE.json configs[i]; 2 (default) is the configuration the metric is quoted on")
    ap.add_argument("--hidden", type=int, default=None, help="override the config's hidden size")
    ap.add_argument("--seq", type=int, default=None, help="override the config's window length")
    ap.add_argument("--batch", type=int, default=None, help="override: streams per GPU (weak scaling)")
    ap.add_argument("--sustained-seconds", type=float, default=2.0,
                    help="before the warm-up, this many seconds of windows to bring the GPU to its operating clocks; with "
                         "--full also timed as the `sustained` figure, over at least K windows (0 = skip)")
    ap.add_argument("--cpu-budget", type=float, default=20.0, help="seconds of CPU work for the cpu_baseline leg (--full)")
    ap.add_argument("--lr", type=float, default=0.01,
                    help="Adagrad step; 0.1 (R/lstm.cc:59) overflows the unshifted softmax at hidden=512 batch=64 "
                         "within ~100 windows unless the class_CUDA warm-up (lr=0 for 50*S windows) is used")
    ap.add_argument("--flags", type=int, default=0)
    ap.add_argument("--bf16", action="store_true", help="bf16 MFMA in the recurrent products (not the headline dtype)")
    ap.add_argument("--fp32", action="store_true", help="force the fp32 path on a config whose named dtype is bf16 (configs[4]: the "
                                                         "fp32 line beside the bf16 one)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the cpu_baseline leg")
    ap.add_argument("--profile-windows", type=int, default=3, help="windows of the --full per-kernel profiling pass")
    ap.add_argument("--full", action="store_true",
                    help="also measure the `sustained` figure, per-kernel times, the roofline and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed to DIR/<name>.npy (see dump_outputs)")
    args = ap.parse_args()

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            sys.exit("bench.py --gpus N>1 must be launched with torch.distributed.run (one rank per GPU)")
        args.gpus = world

    import dp
    import lstm_hip

    cfg = CONFIGS[args.config]
    if cfg.get("bf16") and not args.fp32:
        args.bf16 = True
    if args.bf16:
        args.flags |= 128  # LSTM_HIP_BF16_RECURRENCE
    N = args.hidden or cfg["N"]
    S = args.seq or cfg["S"]
    B = args.batch or cfg["B"]
    lr = args.lr
    rdzv = dp.Rendezvous(rank, world, tag=os.environ.get("MASTER_PORT", "0") + "_" + os.environ.get("TORCHELASTIC_RUN_ID", "0"))

    text = synthetic_text(cfg["nbytes"], seed=0)
    bf16_refused = None
    try:
        L = lstm_hip.Lstm(N, S, B, device=local_rank, flags=args.flags)
    except lstm_hip.LstmHipError as e:
        if not args.bf16:
            raise
        # the bf16 path refuses shapes whose persistent grids are not co-resident (e.g. hidden 1024 with 128 streams per
        # GPU): measure the fp32 path instead and say so in the line
        bf16_refused = str(e)
        args.bf16 = False
        args.flags &= ~128
        L = lstm_hip.Lstm(N, S, B, device=local_rank, flags=args.flags)
    P0 = lstm_hip.init_params(lstm_hip.MT19937Normal(1), N)  # identical on every rank
    srng = lstm_hip.MT19937Normal(1000 + rank)
    h1, c1 = srng.randn(N, B, 0.0, 0.1), srng.randn(N, B, 0.0, 0.1)  # column 1: becomes column 0 after the first slide
    L.set_text(text)
    # Steady state from the first timed window on, whatever --warmup is: the window is uploaded FULL, as S slides from the
    # start cursors c0 would have left it (OV/lstm_eigen_opt/lstm.cc:190-213: target[t] = text[c0+t], x[t] = target[t-1]),
    # and the cursors continue from c0 + S.  (The reference starts from an empty window and fills it over S iterations.)
    c0 = dp.cursors(len(text), S, rank, world, world * B).astype(np.int64)  # rank r owns streams [r*B, (r+1)*B)
    tt = np.arange(S, dtype=np.int64)[:, None]
    ti0 = text[(c0[None, :] + tt) % len(text)].astype(np.int32)
    xi0 = text[(c0[None, :] + tt - 1) % len(text)].astype(np.int32)

    def initial_state():
        """the seeded start of every window sequence: parameters, zero Adagrad memory (as a new handle has it), carry,
        full window (ring head 0), cursors.  The timed windows start here whatever the clock warm-up ran before them,
        so the same arguments give the same inputs and outputs on every run."""
        L.set_params(P0)
        L.set_params(np.zeros_like(P0), lstm_hip.P_MEM)
        L.set_state(1, h1, c1)
        L.set_window(xi0, ti0)
        L.set_cursors(((c0 + S) % len(text)).astype(np.uint64))

    initial_state()
    L.set_global_batch(world * B)
    if world > 1:
        L.comm_init(rdzv.broadcast(lstm_hip.comm_unique_id() if rank == 0 else None), world, rank)

    def barrier():
        L.synchronize()
        rdzv.barrier()

    # ---- clock warm-up FIRST: >= 2 s of windows.  It leaves the GPU at its operating clocks for the contract's
    # region below: W warm-up windows, then exactly K timed ones, from the initial state again.  (Timed cold, 25 windows =
    # 20 ms of work run on ramping clocks: 0.83 ms per window against 0.77 sustained.)  With --full the leg runs at least K
    # windows and is a measurement of its own (the `sustained` key).
    sustained = None
    if args.sustained_seconds > 0:
        barrier()
        tp = time.perf_counter()
        L.train_windows(20, lr, want_losses=False)  # probe: how many windows make up the requested seconds
        L.synchronize()
        probe = (time.perf_counter() - tp) / 20
        n_sus = int(np.ceil(args.sustained_seconds / probe))
        if args.full:
            n_sus = max(args.steps, n_sus)
        n_sus = int(rdzv.allgather(n_sus)[0]) if world > 1 else n_sus  # every rank runs rank 0's count
        barrier()
        t1 = time.perf_counter()
        sl = L.train_windows(n_sus, lr, want_losses=args.full)
        L.synchronize()
        barrier()
        wall_s = time.perf_counter() - t1
        if args.full:
            if world > 1:
                wall_s = max(rdzv.allgather(wall_s))
            sustained = {"steps": n_sus, "seconds": round(wall_s, 3), "ms_per_step": round(wall_s / n_sus * 1e3, 4),
                         "value": round((S - 1) * B * n_sus * world / wall_s, 1),
                         "loss_finite": bool(np.all(np.isfinite(sl))), "order": "before the warm-up and the timed steps"}
        initial_state()

    L.train_windows(args.warmup, lr, want_losses=False)
    barrier()
    t0 = time.perf_counter()
    losses, dev_ms = L.train_windows(args.steps, lr, want_losses=True, want_time=True)
    L.synchronize()
    barrier()
    wall = time.perf_counter() - t0
    if world > 1:
        gathered = rdzv.allgather((wall, losses))
        wall = max(g[0] for g in gathered)                      # MAX over ranks
        losses = np.sum([g[1] for g in gathered], axis=0)       # each rank's share of the global-batch loss
    if not np.all(np.isfinite(losses)):
        sys.exit(f"non-finite loss in the timed region: {losses[:5]}")

    chars = (S - 1) * B * args.steps * world
    value = chars / wall

    # ---- what the last timed window left: its loss (summed over ranks), the parameters and Adagrad memory after its update
    # (identical on every rank), rank 0's h and c at its last timestep
    if args.dump_outputs and rank == 0:
        h_last, c_last = L.get_state(S - 1)
        dump_outputs(args.dump_outputs, {"loss": np.asarray(losses[-1:], np.float64), "params": L.get_params(),
                                         "adagrad_mem": L.get_params(lstm_hip.P_MEM), "h": h_last, "c": c_last})

    # ---- per-kernel durations, HIP events on the library's own stream (separate short pass) ----
    roofline = None
    kstats = {}
    if args.full and (rank == 0 or world > 1):
        L.reset_kernel_stats()
        L.set_profiling(True)
        L.train_windows(args.profile_windows, lr, want_losses=False)
        L.set_profiling(False)
        kstats = {k: v for k, v in L.kernel_stats().items() if v[0] > 0}
    if rank == 0:
        # the library fuses DHy / dWhy into the backward recurrence when it runs on 8-column groups (one workgroup per CU on
        # the 256 CUs of an MI355X) and hidden <= 512
        # (wider batches at hidden 256 / 512: the same kernels, several launches over column ranges; one stream at hidden
        # <= 128: single-CU recurrences, unfused)
        fl = kernel_flops(N, S, B, fused=not (args.flags & (64 | 128)) and N <= 512 and N % 64 == 0 and
                          ((N // 16) * ((B + 7) // 8) <= 256 or N in (256, 512)) and not (B == 1 and N in (64, 128)))
        mf = {k: v for k, v in kstats.items() if k in fl}
        if mf:
            dom = max(mf, key=lambda k: mf[k][1])
            calls, ms = mf[dom]
            avg_s = ms / calls * 1e-3
            lpw = max(1, round(calls / max(args.profile_windows, 1)))  # launches per window (column ranges of a wide batch)
            ach = fl[dom] / lpw / avg_s / 1e12
            # bf16 recurrence mode: the two recurrences run on the bf16 pipe (dense peak 2500 TFLOP/s); the PMC traffic
            # file was collected for the fp32 kernels only
            bf16_kernel = bool(args.flags & 128)  # every MFMA kernel of the bf16 path runs on the bf16 pipe
            peak = 2500.0 if bf16_kernel else PEAK_FP32_MFMA_TFLOPS
            roofline = {"bound": "mfma", "kernel": dom, "achieved": round(ach, 3), "peak": peak,
                        "unit": "TFLOP/s", "frac": round(ach / peak, 4), "traffic": pmc_traffic(dom, N, S, B, "bf16" if bf16_kernel else "f32"),
                        "avg_launch_us": round(avg_s * 1e6, 2), "flop_per_launch": fl[dom] / lpw, "launches_per_window": lpw,
                        "window_frac": round((24.0 * N * N + 6.0 * 256 * N) * (value / world) / 1e12 / peak, 4)}

    if rank == 0:
        out = {
            "metric": METRIC if args.config in (2, 3) and (N, S, B) == (512, 100, 64) and not args.bf16
            else f"chars/sec fwd+BPTT, hidden={N} seq={S} batch={B}/GPU",
            "value": round(value, 1), "unit": "chars/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(wall / args.steps * 1e3, 4), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None,
            "dtype": "bf16" if args.flags & 128 else "f32",
            "dtype_note": ("bf16 MFMA operands in the two recurrent and the four time-batched products, f32 accumulate, f32 master "
                           "weights / elementwise / Adagrad" if args.flags & 128 else
                           ("bf16 path refused for this shape, measured in f32: " + bf16_refused if bf16_refused else None)),
            "data": ("FAKE GPU (plumbing test, not a measurement) " if getattr(lstm_hip, "FAKE", False) else "")
                    + f"synthetic ({len(text)} bytes, enwik6 order-0 byte statistics; random-init weights, seed 1)",
            "config": {"workload": f"{cfg['label']}; run as hidden={N} seq={S} batch={B}/GPU (global {B * world}), "
                                   f"{'bf16 MFMA path' if args.bf16 else 'fp32'}, {cfg['corpus']}-sized synthetic text "
                                   f"({len(text)} bytes), stride-1 windows from a full window, Adagrad lr=%g" % lr,
                       "parallelism": f"dp{world}" if world > 1 else "single",
                       "engine": "step-kernels" if (args.flags & lstm_hip.STEP_KERNELS) else "default",
                       # every product of the window is one of the library's own kernels (csrc/gemm.hip for the time-batched
                       # ones); it links and loads no BLAS
                       "gemm": "native"},
            "device_ms_per_step": round(dev_ms / args.steps, 4),
            "loss_first_last": [round(float(losses[0]), 4), round(float(losses[-1]), 4)],
        }
        if args.full:
            out["sustained"] = sustained
            out["roofline"] = roofline
            out["kernels_us"] = {k: [v[0] // max(args.profile_windows, 1), round(v[1] / v[0] * 1e3, 2)] for k, v in kstats.items()}
            if world == 1 and not args.no_cpu_baseline:
                out["cpu_baseline"] = cpu_baseline(N, S, B, text, lr, budget_s=args.cpu_budget)
        print(json.dumps(out), flush=True)
    L.close()
    rdzv.barrier()
    rdzv.close()


if __name__ == "__main__":
    main()
