"""What soft targets cost per window and what distillation buys on held-out text (profiles/distill/).

  python tools/distill_cost.py side --side plain|smooth|distill|teacher --N 512 --S 100 --B 64 [--label NAME] [--out FILE]
      one side in this process, on the library LSTM_HIP_LIB names (default: this build); ms per window from the HIP-event time
      of the device loop, 20 windows per call, the median of seven calls after one untimed call.
        plain    lstm_hip_train_windows, soft targets never set
        smooth   ... with label smoothing 0.1 and no teacher
        distill  ... from a teacher at (alpha, tau) = (0.5, 2): student 512 from a hidden-1024 bf16 teacher, student 128 from a
                 hidden-512 fp32 teacher
        teacher  a forward-only window of that teacher alone: the summed HIP-event times of the launches of lstm_hip_forward on
                 a profiling handle, 20 forward passes per call, with and without its softmax launch (which a borrowed teacher
                 does not make)
  python tools/distill_cost.py all --parent-lib PATH [--out profiles/distill/cost.jsonl]
      at (512, 100, 64) and (128, 26, 8): plain on the parent commit's library (PATH, through LSTM_HIP_LIB) and the four sides
      on this build, one process each, alternately, three rounds; then one `summary` line per shape from the medians, with
      whether this build's plain median lies inside the spread (min to max) of the parent's own lines.
  python tools/distill_cost.py heldout [--windows 6000] [--out profiles/distill/heldout.jsonl]
      the point of the feature: 1 MiB of tools/make_text.py, the last 64 KiB held out and scored with Lstm.eval_texts; a
      hidden-512 teacher, a hidden-128 student alone, the same student from the teacher at (alpha, tau) = (0.5, 1) and
      (0.5, 2), and a hidden-128 model with label smoothing 0.1 alone, each trained the same number of windows.
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
TEACHERS = {512: (1024, True), 128: (512, False)}     # student hidden -> (teacher hidden, bf16 recurrence)
WINDOWS, REPEATS, ROUNDS = 20, 7, 3
SIDES = ("plain", "smooth", "distill", "teacher")
HELD = 64 << 10


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


def _teacher(lstm_hip, N, S, B):
    Nt, bf16 = TEACHERS[N]
    T = lstm_hip.Lstm(Nt, S, B, flags=lstm_hip.BF16_RECURRENCE if bf16 else 0)
    T.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(2), Nt))
    return T, Nt, bf16


def side(a):
    import lstm_hip
    N, S, B = a.N, a.S, a.B
    text = _corpus(64 * S * B + S + 1)
    extra = {}
    L = T = None
    if a.side == "teacher":
        T, Nt, bf16 = _teacher(lstm_hip, N, S, B)
        extra = dict(teacher_N=Nt, teacher_bf16=bf16)
        rs = np.random.RandomState(1)
        T.set_window(rs.randint(0, 256, size=(S, B)).astype(np.int32), rs.randint(0, 256, size=(S, B)).astype(np.int32))
        T.set_profiling(True)
        without = []

        def call():
            T.reset_kernel_stats()
            for _ in range(WINDOWS):
                T.forward()
            T.synchronize()
            stats = T.kernel_stats()
            total = sum(ms for _, ms in stats.values())
            without.append((total - stats["softmax_loss_dy"][1]) / WINDOWS)
            return total / WINDOWS
    else:
        L = lstm_hip.Lstm(N, S, B)
        L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(1), N))
        L.set_text(text)
        L.set_cursors(lstm_hip.initial_cursors(text.size, S, B))
        if a.side == "smooth":
            L.set_soft_targets(smoothing=0.1)
        elif a.side == "distill":
            T, Nt, bf16 = _teacher(lstm_hip, N, S, B)
            extra = dict(teacher_N=Nt, teacher_bf16=bf16, alpha=0.5, temperature=2.0)
            L.set_soft_targets(T, 0.5, 2.0, 0.0)

        def call():
            return L.train_windows(WINDOWS, 0.0, want_losses=False, want_time=True)[1] / WINDOWS
    call()
    if a.side == "teacher":
        del without[:]
    times = [call() for _ in range(REPEATS)]
    row = dict(case=a.side, label=a.label, lib=os.environ.get("LSTM_HIP_LIB", "this build"), N=N, S=S, B=B, windows=WINDOWS,
               repeats=REPEATS, ms_per_window_median=round(float(np.median(times)), 4), ms_per_window_min=round(min(times), 4),
               ms_per_window_max=round(max(times), 4), **extra)
    if a.side == "teacher":
        row["ms_per_window_without_softmax_median"] = round(float(np.median(without)), 4)
    _emit(row, a.out)
    for H in (L, T):
        if H is not None:
            H.close()


def everything(a):
    rows = []
    for N, S, B in SHAPES:
        for _ in range(ROUNDS):
            for name, lib in (("plain", a.parent_lib),) + tuple((s, None) for s in SIDES):
                env = dict(os.environ)
                env.pop("LSTM_HIP_LIB", None)
                if lib:
                    env["LSTM_HIP_LIB"] = os.path.abspath(lib)
                label = "parent" if lib else "branch"
                cmd = [sys.executable, os.path.abspath(__file__), "side", "--side", name, "--N", str(N), "--S", str(S), "--B", str(B),
                       "--label", label]
                done = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
                if done.returncode != 0:   # nothing more is started on the device after a failed side
                    sys.stderr.write(done.stdout + done.stderr)
                    sys.exit(done.returncode)
                for line in done.stdout.splitlines():
                    if line.startswith("{"):
                        row = json.loads(line)
                        if lib:
                            row["lib"] = "parent commit"
                        rows.append(row)
                        _emit(row, a.out)

        def of(case, label, key="ms_per_window_median"):
            return [r[key] for r in rows if (r["case"], r["label"], r["N"], r["S"], r["B"]) == (case, label, N, S, B)]
        parent, plain = float(np.median(of("plain", "parent"))), float(np.median(of("plain", "branch")))
        smooth, distill = float(np.median(of("smooth", "branch"))), float(np.median(of("distill", "branch")))
        teacher = float(np.median(of("teacher", "branch", "ms_per_window_without_softmax_median")))
        lo = min(of("plain", "parent", "ms_per_window_min"))
        hi = max(of("plain", "parent", "ms_per_window_max"))
        _emit(dict(case="summary", N=N, S=S, B=B, parent_plain_ms=round(parent, 4), branch_plain_ms=round(plain, 4),
                   parent_spread_ms=[lo, hi], branch_plain_inside_parent_spread=bool(lo <= plain <= hi),
                   branch_smooth_ms=round(smooth, 4), smooth_minus_plain_ms=round(smooth - plain, 4),
                   branch_distill_ms=round(distill, 4), teacher_forward_ms=round(teacher, 4),
                   distill_minus_plain_plus_teacher_ms=round(distill - (plain + teacher), 4),
                   distill_over_plain=round(distill / plain, 3)), a.out)


def heldout(a):
    import lstm_hip
    S, B, lr = a.S, a.B, a.lr
    text = _corpus(1 << 20)
    train, held = text[:-HELD], text[-HELD:]

    def model(N, seed, soft=None):
        L = lstm_hip.Lstm(N, S, B)
        L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(seed), N))
        L.set_text(train)
        L.set_cursors(lstm_hip.initial_cursors(train.size, S, B))
        L.set_stride(S - 1, S - 1)
        if soft:
            L.set_soft_targets(*soft)
        return L

    def run(name, L, **more):
        done, last, kl = 0, 0.0, None
        while done < a.windows:
            k = min(500, a.windows - done)
            last = float(np.mean(L.train_windows(k, lr))) / (S - 1)
            if more.get("teacher_N"):
                kl = float(np.mean(L.teacher_kl())) / (S - 1)
            done += k
        bits = float(L.eval_texts([held])["bits"][0]) / (held.size - 1)
        row = dict(case="heldout", run=name, N=L.N, S=S, B=B, lr=lr, windows=a.windows, train_bytes=int(train.size),
                   heldout_bytes=int(held.size), train_bits_per_char_last_500=round(last, 5), heldout_bits_per_char=round(bits, 5), **more)
        if kl is not None:
            row["teacher_kl_bits_per_char_last_500"] = round(kl, 5)
        _emit(row, a.out)

    T = model(512, 2)
    run("teacher", T)
    Pt = T.get_params()
    T.close()
    for name, setting in (("student_alone", None), ("student_distilled", (0.5, 1.0, 0.0)), ("student_distilled", (0.5, 2.0, 0.0)),
                          ("student_smoothed", (1.0, 1.0, 0.1))):
        teacher = None
        more = {}
        if name == "student_distilled":
            teacher = lstm_hip.Lstm(512, S, B)
            teacher.set_params(Pt)
            more = dict(teacher_N=512, alpha=setting[0], temperature=setting[1])
        elif setting:
            more = dict(smoothing=setting[2])
        L = model(128, 1, (teacher,) + setting if setting else None)
        run(name, L, **more)
        L.close()
        if teacher is not None:
            teacher.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("side", "all", "heldout"))
    ap.add_argument("--side", choices=SIDES, default="plain")
    ap.add_argument("--N", type=int, default=128)
    ap.add_argument("--S", type=int, default=26)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--windows", type=int, default=6000)
    ap.add_argument("--label", default="")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.mode == "all" and not a.parent_lib:
        ap.error("all needs --parent-lib")
    {"side": side, "all": everything, "heldout": heldout}[a.mode](a)


if __name__ == "__main__":
    main()
