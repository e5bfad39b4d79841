"""Bit-for-bit A/B of two builds of the library over every recurrence instantiation the launchers can pick.

Every kernel of a training window is deterministic, so two builds whose device code is the same must agree
in every bit.  One case list runs in a child process per library (LSTM_HIP_LIB), each child under a time limit of its own;
a child that fails, aborts or hangs ends the script.  Per case: one forward / loss / backward through the step API, then
three train_windows; the line written holds the plan, the losses and SHA-256 digests of the gradients and the parameters.

  python tools/ab_windows.py OUTDIR parent=/path/liblstm_hip.so branch=/path/liblstm_hip.so [--timeout SECONDS]

writes OUTDIR/bits_parent.jsonl and OUTDIR/bits_branch.jsonl and exits 0 only if they are identical.
"""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 5
FAST, STAMPS, UNFUSED, BF16 = 1, 16, 64, 128  # LSTM_HIP_FAST_MATH, _DEBUG_STAMPS, _NO_FUSED_GRADS, _BF16_RECURRENCE
ONE = {"LSTM_HIP_FWD_HALVES": "0", "LSTM_HIP_BWD_HALVES": "0"}  # the one-recurrence forms where the shape has them


def cases():
    """(N, B, flags, env).  Every form with a FAST parameter runs with and without LSTM_HIP_FAST_MATH."""
    base = [(64, 1, 0, {}), (128, 1, 0, {})]                                            # single-CU forms
    base += [(64, 5, 0, {}), (128, 3, 0, {}), (1024, 8, 0, {}), (1024, 136, 0, {})]     # first / second forward form
    base += [(1024, 16, 0, {}), (64, 8, UNFUSED, {}), (128, 8, UNFUSED, {})]            # 8-column forms
    base += [(64, 520, 0, {}), (128, 264, 0, {})]                                       # 16-column backward groups
    for N in (256, 512):
        for B in (1, 5, 64, 136):                                                       # two-half / scatter; 136: several launches
            base += [(N, B, 0, {}), (N, B, UNFUSED, {})]
        base += [(N, 16, 0, ONE), (N, 16, UNFUSED, ONE)]
    base += [(128, 8, BF16, {}), (128, 136, BF16, {}), (128, 800, BF16, {}), (1024, 24, BF16, ONE)]  # 4, 8, 16 columns; 16-column forward
    for N in (256, 512, 1024):
        for B in (8, 16, 40, 136):
            base += [(N, B, BF16, {}), (N, B, BF16, ONE)]
    out = base + [(N, B, flags | FAST, env) for N, B, flags, env in base]
    stamped = [(512, 64, STAMPS, {}), (512, 64, STAMPS | UNFUSED, {}), (512, 16, STAMPS, ONE), (512, 16, STAMPS | UNFUSED, ONE)]
    return out + stamped + [(N, B, STAMPS | BF16, {}) for N, B in ((256, 16), (512, 64), (1024, 16))]


def digest(a):
    return hashlib.sha256(a.tobytes()).hexdigest()[:32]


def run_case(lstm_hip, np, N, B, flags, env):
    for k in ONE:
        os.environ.pop(k, None)
    os.environ.update(env)
    L = lstm_hip.Lstm(N, S, B, flags=flags)
    for k in ONE:
        os.environ.pop(k, None)
    rs = np.random.RandomState(1000 * N + B)
    L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(N + B), N))
    L.set_state(0, (rs.randn(B, N) * 0.1).astype(np.float32), (rs.randn(B, N) * 0.1).astype(np.float32))
    L.set_window(rs.randint(0, 256, size=(S, B)), rs.randint(0, 256, size=(S, B)))
    L.forward()
    loss = L.loss()
    L.backward()
    rec = {"N": N, "B": B, "flags": flags, "env": env, "plan": L.plan_identity(), "step_loss": loss.hex(),
           "step_grads": digest(L.get_grads())}
    text = rs.randint(0, 256, size=65536).astype(np.uint8)
    L.set_text(text)
    L.set_cursors(lstm_hip.initial_cursors(len(text), S, B))
    rec["losses"] = [float(x).hex() for x in L.train_windows(3, 0.05)]
    rec["grads"] = digest(L.get_grads())
    rec["params"] = digest(L.get_params())
    rec["memory"] = digest(L.get_params(lstm_hip.P_MEM))
    L.close()
    return rec


def child(out):
    sys.path.insert(0, os.path.join(ROOT, "eigen-lstm_amd"))
    import numpy as np
    import lstm_hip
    with open(out, "w") as f:
        for N, B, flags, env in cases():
            f.write(json.dumps(run_case(lstm_hip, np, N, B, flags, env), sort_keys=True) + "\n")
            f.flush()


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2])
    outdir, libs, timeout = sys.argv[1], {}, 300
    args = sys.argv[2:]
    while args:
        a = args.pop(0)
        if a == "--timeout":
            timeout = int(args.pop(0))
        else:
            name, path = a.split("=", 1)
            libs[name] = os.path.abspath(path)
    os.makedirs(outdir, exist_ok=True)
    files = []
    for name, lib in libs.items():
        files.append(os.path.join(outdir, f"bits_{name}.jsonl"))
        env = dict(os.environ, LSTM_HIP_LIB=lib)
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", files[-1]], env=env, timeout=timeout).returncode
        if rc != 0:  # (a time-out raises: nothing more is started on the device either way)
            sys.exit(f"{name}: the child ended with status {rc}; stopping")
    texts = [open(f).read() for f in files]
    same = all(t == texts[0] for t in texts[1:])
    print(f"{len(texts[0].splitlines())} cases; " + ("every bit agrees" if same else "THE FILES DIFFER"))
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
