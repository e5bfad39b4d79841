"""-m gpu: weight drop, DropConnect on the hidden-to-hidden matrix U with one mask per training window
(lstm_hip_set_weight_drop, lstm_hip_get_weight_drop, lstm_hip_weight_drop_mask in include/lstm_hip.h).

A window trained with weight drop is a window of the unchanged engine on Ue = where(keep, U * s, +0), followed by the same
mask and scale on dU.  Both are single fp32 operations, so NumPy's float32 arithmetic with the reference mask of
tests/weight_drop_ref.py reproduces them bit for bit and everything here is compared by bytes: the zero pattern of dU, a twin
handle that holds Ue as its parameters, the update against a handle that is handed the gradient, the window loop in chunks
and by hand, switching, inference, resuming, the refusals and the training program.  The shapes are the rows of
handle_sequence_cases.SHAPES (one per pair of recurrence forms) and two small padded handles."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import handle_replay as hr
import handle_sequence_cases as hsc
import weight_drop_ref as wd
from test_pad_hidden import same_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSTM = os.path.join(ROOT, "eigen-lstm_amd", "lstm")

# ... and two small padded handles; at 30 of 32 the gate blocks start at e = 30, 60, 90, so a float4 of the internal matrix
# spans two Philox quads
SHAPES = list(hsc.SHAPES) + [hsc.Shape("padded, 100 of 128", 100, 6, 4, ("PAD_HIDDEN",), {}, {}),
                             hsc.Shape("padded, 30 of 32", 30, 6, 4, ("PAD_HIDDEN",), {}, {})]
IDS = [hsc.shape_id(sh) for sh in SHAPES]
assert len(set(IDS)) == len(IDS)
shapes = pytest.mark.parametrize("sh", SHAPES, ids=IDS)

RATE = 0.25
SEED = 0x243F6A8800000007       # a non-zero high word
T0 = 2 ** 32 + 3                # ... and a mask index past 32 bits
TEXT = np.random.RandomState(11).randint(32, 127, size=hsc.LONG).astype(np.uint8)
M = 256


def _u(block, N):
    """the U range of a logical flat block [W | U | b | Why | by]: element e = r + 4N k at index e"""
    return block[4 * N * M:4 * N * M + 4 * N * N]


def _rest(block, N):
    return np.concatenate([block[:4 * N * M], block[4 * N * M + 4 * N * N:]])


def _start(sh, on=True, adam=False, clip=False, seed=SEED, t=T0):
    import lstm_hip
    L = hr.start(sh, TEXT)
    if adam:
        hr.apply_setting(L, "optimizer", lstm_hip.OPT_ADAM)
    if clip:
        hr.apply_setting(L, "clip", hr.CLIP_ON)
    if on:
        L.set_weight_drop(RATE, seed, t)
    L.set_state(0, *L.get_state(1))  # (the by-hand passes start from column 0)
    return L


def _state(L):
    """the observable state and the weight-drop numbers, as comparable arrays"""
    snap = hr.snapshot(L, TEXT)
    rate, seed, t = L.weight_drop()
    snap["weight_drop"] = np.array([np.float64(rate).view(np.uint64), seed, t], np.uint64)
    return snap


def _restore(sh, snap, weight_drop=None):
    L = hr.restore(sh, snap)
    if weight_drop is not None:
        L.set_weight_drop(*weight_drop)
    return L


# ---- 1. the mask shows -------------------------------------------------------------------------------------------------------
# An fp32 sum of a few hundred products of either sign is exactly 0 about once in 10^8 elements (the sum's last bit is some
# 2^-23 of its spread), so among the up to 4 * 10^6 elements of a matrix here a kept element or two can hold a true 0.0 that
# the product itself gave: measured once, at hidden 512 with 64 streams, element 862289, on the handle without weight drop too.
# The pattern is therefore compared where the twin's product (test 2: the unmasked engine on Ue) is not zero itself, and at
# most CHANCE_ZEROS elements may be excused that way -- a mask that is wrong in one quad of one column shows as more.
CHANCE_ZEROS = 4


def _masked_pattern(dU, keep):
    """(dropped elements that are not +0.0f bit for bit, kept elements that are 0)"""
    return int(np.count_nonzero(dU[~keep].view(np.uint32))), int(np.count_nonzero(dU[keep] == 0))


@shapes
def test_mask_shows_in_the_gradient(sh):
    A = _start(sh)
    B = _start(sh, on=False)  # the twin of test 2, for the product's own zeros
    pattern = []
    for k in range(2):
        keep = wd.flat_mask(sh.N, RATE, SEED, T0 + k)
        Pe = A.get_params()
        _u(Pe, sh.N)[:] = wd.apply(_u(Pe, sh.N), keep, RATE)
        B.set_params(Pe)
        for L in (A, B):
            L.forward()
            L.backward()
        dU, own = _u(A.get_grads(), sh.N), _u(B.get_grads(), sh.N) != 0
        dropped_set, kept_zero = _masked_pattern(dU, keep)
        print(f"mask t+{k}: dropped {int((~keep).sum())}, of them not +0.0f {dropped_set}; kept but zero {kept_zero}, "
              f"zero in the unmasked product itself {int(np.count_nonzero(keep & ~own))}")
        assert dropped_set == 0                                   # dropped: +0.0f, every bit
        assert np.array_equal(dU != 0, keep & own), (k, int(((dU != 0) != (keep & own)).sum()))
        assert np.count_nonzero(keep & ~own) <= CHANCE_ZEROS
        assert A.weight_drop() == (RATE, SEED, T0 + k)
        pattern.append(keep)
        A.adagrad(hr.LR)
    assert A.weight_drop() == (RATE, SEED, T0 + 2)
    assert not np.array_equal(pattern[0], pattern[1])
    frac = 1.0 - pattern[0].mean()
    assert abs(frac - RATE) < 4 * math.sqrt(RATE * (1 - RATE) / pattern[0].size) + 1e-9, frac  # (four sigma of a fair mask)
    A.close()
    B.close()


# ---- 2. the twin: a handle that holds Ue as its parameters ---------------------------------------------------------------------
@shapes
def test_window_equals_the_twin_that_holds_the_masked_matrix(sh):
    N = sh.N
    A = _start(sh)
    B = _start(sh, on=False)
    P = A.get_params()
    keep = wd.flat_mask(N, RATE, SEED, T0)
    Pe = P.copy()
    _u(Pe, N)[:] = wd.apply(_u(P, N), keep, RATE)
    B.set_params(Pe)
    for L in (A, B):
        L.forward()
        L.backward()
    assert same_bytes(np.array([A.loss()]), np.array([B.loss()]))
    for t in range(sh.S):
        for x, y in zip(A.get_state(t), B.get_state(t)):
            assert same_bytes(x, y), t
        if t >= 1:
            for x, y in zip(A.get_activations(t), B.get_activations(t)):
                assert same_bytes(x, y), t
    da, db = A.get_grads(), B.get_grads()
    assert same_bytes(_rest(da, N), _rest(db, N))                      # dW, db, dWhy, dby
    assert same_bytes(_u(da, N), wd.apply(_u(db, N), keep, RATE))      # dU = where(keep, dUe * s, 0)
    assert same_bytes(A.get_params(), P)                               # the parameters themselves are not masked
    A.close()
    B.close()


# ---- 3. the update is the plain update on the masked gradient -----------------------------------------------------------------
@pytest.mark.parametrize("adam", [False, True], ids=["adagrad", "adamw"])
@shapes
def test_update_equals_a_handle_given_the_gradient(sh, adam):
    import lstm_hip
    blocks = [lstm_hip.P_PARAMS, lstm_hip.P_MEM] + ([lstm_hip.P_ADAM_V] if adam else [])
    A = _start(sh, adam=adam)
    for _ in range(2):  # (the second update starts from a non-zero optimizer state)
        A.forward()
        A.backward()
        before = {w: A.get_params(w) for w in blocks}
        grad, steps = A.get_grads(), A.optimizer_steps()
        A.adagrad(hr.LR)
    Z = hr.create(sh)
    if adam:
        hr.apply_setting(Z, "optimizer", lstm_hip.OPT_ADAM)
    for w in blocks:
        Z.set_params(before[w], w)
    Z.set_params(grad, lstm_hip.P_GRADS)
    Z.set_optimizer_steps(steps)
    Z.adagrad(hr.LR)
    for w in blocks:
        assert same_bytes(A.get_params(w), Z.get_params(w)), w
    assert not same_bytes(A.get_params(), before[lstm_hip.P_PARAMS])
    A.close()
    Z.close()


# ---- 4. the loop: one call, chunks, and single windows by hand ------------------------------------------------------------------
@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@shapes
def test_loop_chunks_and_single_windows_agree(sh, clip):
    runs = []
    for ops in ([("T", 5)], [("T", 1), ("T", 2), ("T", 2)], [("W",)] * 5):
        L = _start(sh, clip=clip)
        losses, norms, out = [], [], {}
        for op in ops:
            out = hr.run_op(L, op)
            losses.append(out["losses"] if op[0] == "T" else out["loss"])
            if clip:
                norms.append(out["norms"])
        res = dict(_state(L), losses=np.concatenate(losses), grads=out["grads"])
        if clip:
            res["norms"] = np.concatenate(norms)
        runs.append(res)
        assert L.weight_drop() == (RATE, SEED, T0 + 5)
        L.close()
    hr.assert_same(runs[0], runs[1], "one call against chunks (1, 2, 2)")
    hr.assert_same(runs[0], runs[2], "one call against five single windows")
    assert np.all(np.isfinite(runs[0]["losses"])) and runs[0]["losses"].size == 5
    if clip:  # the norm is taken on the masked gradient: the tolerance of tests/test_grad_clip.py
        want = float(np.sqrt(np.sum(runs[0]["grads"].astype(np.float64) ** 2)))
        rec = float(runs[0]["norms"][-1])
        assert abs(rec - want) <= 1e-9 * want, (rec, want)
    keep = wd.flat_mask(sh.N, RATE, SEED, T0 + 4)  # the last window's mask
    dropped_set, kept_zero = _masked_pattern(_u(runs[0]["grads"], sh.N), keep)
    assert dropped_set == 0 and kept_zero <= CHANCE_ZEROS, (dropped_set, kept_zero)


# ---- 5. off is off, and switching is clean ----------------------------------------------------------------------------------------
FOUR = [("T", 2), ("W",), ("T", 1)]


def _run(L, ops):
    outs = [hr.run_op(L, op) for op in ops]
    res = _state(L)
    for i, o in enumerate(outs):
        for k, v in o.items():
            res[f"op{i}.{k}"] = v
    return res


@shapes
def test_rate_zero_equals_a_handle_that_never_heard_of_it(sh):
    A = _start(sh, on=False)
    A.set_weight_drop(0.0, SEED, 9)
    Z = _start(sh, on=False)
    a, z = _run(A, FOUR), _run(Z, FOUR)
    a.pop("weight_drop"), z.pop("weight_drop")  # (rate 0 keeps the numbers it was given; nothing advances them)
    hr.assert_same(a, z, "rate 0 against never set")
    assert A.weight_drop() == (0.0, SEED, 9)
    A.close()
    Z.close()


SWITCHES = {
    "off": lambda rate, seed, t: (0.0, 0, 0),
    "seed": lambda rate, seed, t: (rate, seed ^ 0x55, t),
    "resume": lambda rate, seed, t: (rate, seed, t),      # 7. a fresh handle given the state and (rate, seed, t) from get
}


@pytest.mark.parametrize("switch", sorted(SWITCHES))
@shapes
def test_switching_equals_a_fresh_handle_with_the_state(sh, switch):
    A = _start(sh)
    _run(A, [("T", 1), ("W",)])
    assert A.weight_drop() == (RATE, SEED, T0 + 2)
    new = SWITCHES[switch](*A.weight_drop())
    if switch != "resume":
        A.set_weight_drop(*new)
    Z = _restore(sh, hr.snapshot(A, TEXT), None if switch == "off" else new)
    a, z = _run(A, [("T", 2)]), _run(Z, [("T", 2)])
    if switch == "off":
        a.pop("weight_drop"), z.pop("weight_drop")
        assert np.count_nonzero(_u(a["op0.grads"], sh.N) == 0) <= CHANCE_ZEROS  # no mask any more
    else:
        assert A.weight_drop() == (new[0], new[1], new[2] + 2)
    hr.assert_same(a, z, f"switch {switch}")
    A.close()
    Z.close()


@shapes
def test_new_parameters_between_windows_are_picked_up(sh):
    A = _start(sh)
    A.forward()
    first = A.loss()
    P = A.get_params()
    P2 = P + (np.random.RandomState(4).randn(P.size) * 1e-2).astype(np.float32)
    A.set_params(P2)
    Z = _start(sh)
    Z.set_params(P2)
    a, z = _run(A, [("FB",), ("T", 1)]), _run(Z, [("FB",), ("T", 1)])
    hr.assert_same(a, z, "after set_params(0)")
    assert a["op0.loss"][0] != first
    A.close()
    Z.close()


# ---- 6. inference does not see it ----------------------------------------------------------------------------------------------
def _infer(L):
    rs = np.random.RandomState(5)
    out = {"eval_bits": np.array([L.eval_bits(rs.randint(32, 127, size=60).astype(np.uint8))])}
    prompts = [rs.randint(32, 127, size=k).astype(np.uint8) for k in (3, 5)]
    g, bits, gh, gc = L.generate(prompts, count=6, u=rs.random_sample((6, 2)), score=True)
    out["generate"], out["generate_bits"], out["generate_h"], out["generate_c"] = g, bits, gh, gc
    sc = L.score(prompts, top_n=2)
    for key in ("surprisal", "entropy", "rank", "top_byte", "top_bits"):
        out["score_" + key] = np.concatenate([np.asarray(a).ravel() for a in sc[key]])
    codes, cbits = L.encode([rs.randint(32, 127, size=12).astype(np.uint8) for _ in range(2)])
    out["code"], out["code_bits"] = np.frombuffer(b"".join(codes), np.uint8), cbits
    return out


@shapes
def test_inference_reads_the_unmasked_parameters(sh):
    import lstm_hip
    A = _start(sh, t=0)
    A.set_averaging(lstm_hip.AVG_UNIFORM)
    hr.run_op(A, ("T", 2))
    A.forward()  # (the window's images are the masked ones when inference is called)
    P = A.get_params()
    assert np.count_nonzero(_u(P, sh.N) == 0) < 8  # get_params(0): nothing dropped
    on = _infer(A)
    A.set_weight_drop(0.0)
    off = _infer(A)
    Z = hr.create(sh)
    Z.set_params(P)
    fresh = _infer(Z)
    hr.assert_same(on, off, "inference with weight drop on against off")
    hr.assert_same(on, fresh, "inference against a handle that only holds the parameters")
    # the average takes the unmasked parameters: after one more update (n = 3) it follows the rule on get_params
    avg = A.get_average()
    A.set_weight_drop(RATE, SEED, 5)
    hr.run_op(A, ("T", 1))
    p = A.get_params()
    assert same_bytes(A.get_average(), avg + np.float32(1.0 / 3.0) * (p - avg))
    A.close()
    Z.close()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------
SMALL = hsc.Shape("refusals", 64, 6, 4, (), {}, {})


def test_refusals_leave_the_handle_usable():
    import lstm_hip
    L = _start(SMALL)
    lib, h = L.lib, L._h
    EINVAL, ESTATE = lstm_hip.EINVAL, lstm_hip.ESTATE
    err = lambda: lib.lstm_hip_last_error().decode()
    for bad in (-0.25, 1.0, 1.5, math.nan, math.inf, -math.inf):
        assert lib.lstm_hip_set_weight_drop(h, C.c_double(bad), C.c_uint64(1), C.c_uint64(1)) == EINVAL, bad
        assert ("%g" % bad) in err(), (bad, err())
        assert L.weight_drop() == (RATE, SEED, T0)
    rate, seed, t = C.c_double(), C.c_uint64(), C.c_uint64()
    assert lib.lstm_hip_get_weight_drop(h, None, C.byref(seed), C.byref(t)) == EINVAL
    assert lib.lstm_hip_get_weight_drop(None, C.byref(rate), C.byref(seed), C.byref(t)) == EINVAL
    # set drops the forward pass
    L.forward()
    L.backward()
    L.forward()
    L.set_weight_drop(RATE, SEED, T0)
    assert lib.lstm_hip_backward(h) == ESTATE
    L.forward()
    L.backward()
    # the adaptive coders refuse while it is on, and change nothing
    before = _state(L)
    texts = [np.full(12, 97, np.uint8)] * SMALL.B
    off = np.arange(SMALL.B + 1, dtype=np.uint64) * 12
    code, code_off, data = np.zeros(SMALL.B * 40, np.uint8), np.zeros(SMALL.B + 1, np.uint64), np.concatenate(texts)
    p8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    assert lib.lstm_hip_encode_adaptive(h, p8(data), p64(off), C.c_double(0.05), p8(code), C.c_uint64(code.size), p64(code_off),
                                        None, None, None) == ESTATE
    assert "weight drop" in err()
    assert lib.lstm_hip_decode_adaptive(h, p8(code), p64(code_off), p64(off), C.c_double(0.05), p8(data)) == ESTATE
    assert "weight drop" in err()
    hr.assert_same(before, _state(L), "after the refused adaptive calls")
    hr.run_op(L, ("T", 1))
    assert L.weight_drop() == (RATE, SEED, T0 + 1)
    L.set_weight_drop(0.0)
    codes, _, _ = L.encode_adaptive(texts, 0.05)  # off again: the adaptive coder runs
    assert len(codes) == SMALL.B
    L.close()


def test_split_dU_plan_refuses_weight_drop():
    import lstm_hip
    L = hr.create(hsc.Shape("dU in halves", 256, 6, 16, (), {"LSTM_HIP_DU_SPLIT": "1"}, {}))
    assert L.lib.lstm_hip_set_weight_drop(L._h, C.c_double(RATE), C.c_uint64(0), C.c_uint64(0)) == lstm_hip.ESTATE
    assert "LSTM_HIP_DU_SPLIT" in L.lib.lstm_hip_last_error().decode()
    assert L.weight_drop() == (0.0, 0, 0)
    L.close()


# ---- 9. the program -----------------------------------------------------------------------------------------------------------------
def test_program_saves_and_resumes_weight_drop(tmp_path):
    """The program draws fresh states for every run and keeps its parameter checkpoints at 6 digits, so (as in
    tests/test_weight_averaging.py) a cut run can equal the uninterrupted one only from a saved checkpoint and at lr = 0; what
    is compared is then what the cut must carry: the parameters and the three weight-drop numbers, t advanced over the cut."""
    text = np.random.RandomState(11).randint(97, 110, size=3000).astype(np.uint8)
    f = tmp_path / "corpus.txt"
    text.tofile(f)
    run = lambda args: subprocess.run(args, capture_output=True, text=True, errors="replace", timeout=300)
    base = [LSTM, str(f), "32", "8", "4", "--epochs", "1", "--seed", "1", "--sample", "0", "--quiet"]
    opt = ["--weight-drop", "0.5", "--weight-drop-seed", "77"]
    p0, plain, a, b, c, d = (str(tmp_path / k) for k in ("p0", "plain", "a", "b", "c", "d"))
    out = run(base + ["--lr", "0.05", "--windows", "9", "--save", p0] + opt)
    assert out.returncode == 0, out.stderr
    assert open(p0 + "_weight_drop.txt").read().split() == "rate 0.5 seed 77 t 9".split()
    out = run(base + ["--lr", "0.05", "--windows", "9", "--save", plain])
    assert out.returncode == 0 and not os.path.exists(plain + "_weight_drop.txt"), out.stderr
    assert open(plain + "_U.txt").read() != open(p0 + "_U.txt").read()  # the option trains another model
    read = lambda path: np.loadtxt(path, dtype=np.float64, ndmin=1)
    assert np.count_nonzero(read(p0 + "_U.txt") == 0) < 8  # ... whose saved matrix is the unmasked one
    lr0 = ["--lr", "0"]
    out = run(base + lr0 + opt[:2] + ["--load", p0, "--windows", "13", "--save", a])  # (the seed comes from the checkpoint)
    assert out.returncode == 0, out.stderr
    assert "Loaded weight drop (seed = 77, t = 9)" in out.stdout, out.stdout
    out = run(base + lr0 + opt[:2] + ["--load", a, "--windows", "8", "--save", b])
    assert out.returncode == 0, out.stderr
    assert "Loaded weight drop (seed = 77, t = 22)" in out.stdout, out.stdout
    out = run(base + lr0 + opt + ["--load", p0, "--windows", "21", "--save", c])
    assert out.returncode == 0, out.stderr
    for k in ("W", "U", "Why", "b", "by"):
        assert open(f"{b}_{k}.txt").read() == open(f"{c}_{k}.txt").read(), k
    assert open(b + "_weight_drop.txt").read() == open(c + "_weight_drop.txt").read()
    assert open(c + "_weight_drop.txt").read().split() == "rate 0.5 seed 77 t 30".split()
    # a seed on the command line wins over the checkpoint's; without the option the file is ignored
    out = run(base + lr0 + ["--weight-drop", "0.25", "--weight-drop-seed", "5", "--load", p0, "--windows", "3", "--save", d])
    assert out.returncode == 0, out.stderr
    assert open(d + "_weight_drop.txt").read().split() == "rate 0.25 seed 5 t 12".split()
    out = run(base + lr0 + ["--load", p0, "--windows", "3"])
    assert out.returncode == 0 and "weight drop" not in out.stdout, out.stdout
