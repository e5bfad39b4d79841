"""-m gpu: the running weight average and inference from it (lstm_hip_set_averaging, lstm_hip_get_average, lstm_hip_set_average,
lstm_hip_get_averaging_counts, lstm_hip_set_averaging_counts, lstm_hip_set_inference_source in include/lstm_hip.h).

Every update the handle launches counts (seen += 1); the update is due when seen % every == 0; at a due update n += 1 and the
average takes the parameters p the update has just written: a = p at n == 1 (a copy), a = a + w * (p - a) after it, in fp32 with
three separately rounded operations, w = float(1 - decay) for the EMA and float(1 / n) for the uniform mean.  NumPy's float32
a + w * (p - a) is that rule bit for bit, so everything here is compared by bytes: the rule on every engine form, chunking,
that training does not notice the average, inference from the average against a second handle that holds it as its
parameters, resuming through the public calls, padding, the refusals, and the training program's checkpoints."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import gpu_util as gu
from test_grad_clip import _flags, _text
from test_pad_hidden import pad_params, padded_width, same_bytes, unpad_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSTM = os.path.join(ROOT, "eigen-lstm_amd", "lstm")
GENERATE = os.path.join(ROOT, "eigen-lstm_amd", "lstm_generate")

# the smallest shapes that reach each engine form: per-step, persistent fp32, bf16 recurrence, padded hidden width
SHAPES = [(64, 6, 4, ("STEP_KERNELS",)), (256, 10, 16, ()), (512, 10, 16, ("BF16_RECURRENCE",)), (100, 6, 4, ("PAD_HIDDEN",))]
IDS = ["step64", "fp32_256", "bf16_512", "pad100"]
DECAY = 0.9  # (far from 1, so that the average is visibly not the last iterate after a few windows)


def _kind(name):
    import lstm_hip
    return lstm_hip.AVG_EMA if name == "ema" else lstm_hip.AVG_UNIFORM


def _handle(N, S, B, names, adam, seed=3, text=None, P=None):
    import lstm_hip
    text = _text() if text is None else text
    L = lstm_hip.Lstm(N, S, B, flags=_flags(names))
    if adam:
        L.set_optimizer(lstm_hip.OPT_ADAM, 0.9, 0.999, 1e-8, 0.01)
    L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(seed), N) if P is None else P)
    L.set_text(text)
    L.set_cursors(lstm_hip.initial_cursors(len(text), S, B))
    return L


def _lr(adam):
    return 2e-3 if adam else 0.05


def _weight(name, n):
    """w as the library narrows it (include/lstm_hip.h)"""
    return np.float32(1.0 - DECAY) if name == "ema" else np.float32(1.0 / float(n))


def _step(a, p, name, n):
    """the rule at a due update, in NumPy float32"""
    if n == 1:
        return p.copy()
    w = _weight(name, n)
    out = a + w * (p - a)
    assert out.dtype == np.float32
    return out


class _Replay:
    def __init__(self, name, every, size):
        self.name, self.every, self.seen, self.n, self.a = name, every, 0, 0, np.zeros(size, np.float32)

    def update(self, p):
        self.seen += 1
        if self.seen % self.every == 0:
            self.n += 1
            self.a = _step(self.a, p, self.name, self.n)


def _averaging(L, name, every):
    L.set_averaging(_kind(name), DECAY if name == "ema" else 0.0, every)


# ---- 1. the rule, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("adam", [False, True], ids=["adagrad", "adam"])
@pytest.mark.parametrize("name", ["ema", "uniform"])
@pytest.mark.parametrize("N,S,B,names", SHAPES, ids=IDS)
def test_average_follows_the_rule_bit_for_bit(N, S, B, names, name, adam, every):
    L = _handle(N, S, B, names, adam)
    _averaging(L, name, every)
    assert L.averaging_counts() == (0, 0) and not np.any(L.get_average())
    ref = _Replay(name, every, L.np)
    for k in range(7):
        L.train_windows(1, _lr(adam))
        p = L.get_params()
        assert np.all(np.isfinite(p))
        ref.update(p)
        assert same_bytes(L.get_average(), ref.a), (k, ref.seen, ref.n)
        assert L.averaging_counts() == (ref.seen, ref.n)
    assert ref.n == 7 // every and not same_bytes(ref.a, p)  # (the average is not simply the last iterate)
    L.close()


# ---- 2. chunking is invisible; the stand-alone update advances the average like a window of the loop --------------------------
@pytest.mark.parametrize("name,every", [("ema", 3), ("uniform", 2)])
@pytest.mark.parametrize("N,S,B,names", SHAPES, ids=IDS)
def test_chunking_is_invisible(N, S, B, names, name, every):
    got = []
    for chunks in ((7,), (1, 3, 3)):
        L = _handle(N, S, B, names, adam=True)
        _averaging(L, name, every)
        for k in chunks:
            L.train_windows(k, _lr(True))
        got.append((L.get_average(), L.averaging_counts(), L.get_params()))
        L.close()
    assert got[0][1] == got[1][1] == (7, 7 // every)
    assert same_bytes(got[0][0], got[1][0]) and same_bytes(got[0][2], got[1][2])
    assert np.any(got[0][0] != 0)


@pytest.mark.parametrize("N,S,B,names", SHAPES, ids=IDS)
def test_update_by_hand_advances_the_average(N, S, B, names):
    import lstm_hip
    P, xi, ti, h0, c0 = gu.random_case(N, S, B, seed=N + B)
    L = lstm_hip.Lstm(N, S, B, flags=_flags(names))
    L.set_params(P)
    _averaging(L, "uniform", 2)
    ref = _Replay("uniform", 2, L.np)
    for k in range(4):
        L.set_state(0, h0, c0)
        L.set_window(xi, ti)
        L.forward()
        L.backward()
        L.adagrad(0.05 if k != 1 else 0.0)  # (an lr = 0 update counts too)
        ref.update(L.get_params())
        assert same_bytes(L.get_average(), ref.a) and L.averaging_counts() == (ref.seen, ref.n), k
    assert ref.n == 2
    L.close()


# ---- 3. training is untouched ----------------------------------------------------------------------------------------------
def _train_state(L, adam):
    import lstm_hip
    out = [L.get_params(), L.get_params(lstm_hip.P_MEM)]
    if adam:
        out.append(L.get_params(lstm_hip.P_ADAM_V))
    out.append(np.array([L.optimizer_steps()]))
    return out


@pytest.mark.parametrize("adam", [False, True], ids=["adagrad", "adam"])
@pytest.mark.parametrize("N,S,B,names", SHAPES, ids=IDS)
def test_training_is_untouched(N, S, B, names, adam):
    import lstm_hip
    A = _handle(N, S, B, names, adam)
    T = _handle(N, S, B, names, adam)  # the twin: never hears of averaging
    _averaging(A, "ema", 1)
    la, lt = [A.train_windows(2, _lr(adam))], [T.train_windows(2, _lr(adam))]
    A.set_inference_source(lstm_hip.SRC_AVERAGE)  # training never reads the source
    la.append(A.train_windows(5, _lr(adam)))
    lt.append(T.train_windows(5, _lr(adam)))
    assert same_bytes(np.concatenate(la), np.concatenate(lt))
    for x, y in zip(_train_state(A, adam), _train_state(T, adam)):
        assert same_bytes(x, y)
    assert same_bytes(A.get_grads(), T.get_grads())
    assert A.averaging_counts() == (7, 7)
    A.close()
    T.close()


# ---- 4. inference from the average -------------------------------------------------------------------------------------------
def _outputs(L, N):
    """every call the inference source reaches, on fixed inputs; a dict of comparable values"""
    rs = np.random.RandomState(5)
    text = rs.randint(32, 127, size=300).astype(np.uint8)
    out = {"eval_bits": np.array([L.eval_bits(text)])}
    h0, c0 = (rs.randn(N) * 0.1).astype(np.float32), (rs.randn(N) * 0.1).astype(np.float32)
    s, hs, cs = L.sample(h0, c0, rs.random_sample(16))
    out["sample"] = np.concatenate([s.astype(np.float32), hs, cs])
    prompts = [rs.randint(32, 127, size=k).astype(np.uint8) for k in (5, 6, 8, 9)]
    g, bits, gh, gc = L.generate(prompts, count=16, u=rs.random_sample((16, 4)), temperature=0.8, score=True)
    out["generate"], out["generate_bits"], out["generate_h"], out["generate_c"] = g, bits, gh, gc
    hyp = L.beam_search(prompts, count=8, beams=3)
    out["beam_bytes"] = np.frombuffer(b"|".join(b for per in hyp for b, _ in per), np.uint8)
    out["beam_bits"] = np.array([c for per in hyp for _, c in per])
    sc = L.score(prompts, top_n=2)
    for key in ("surprisal", "entropy", "rank", "top_byte", "top_bits"):
        out["score_" + key] = np.concatenate([np.asarray(a).ravel() for a in sc[key]])
    out["score_bits"], out["score_h"] = sc["bits"], sc["h"]
    texts = [rs.randint(32, 127, size=40).astype(np.uint8) for _ in range(4)]
    codes, cbits = L.encode(texts)
    out["code"] = np.frombuffer(b"".join(codes), np.uint8)
    out["code_len"], out["code_bits"] = np.array([len(c) for c in codes]), cbits
    back = L.decode(codes, [40] * 4)
    assert [bytes(b) for b in back] == [t.tobytes() for t in texts]
    out["decode"] = np.frombuffer(b"".join(back), np.uint8)
    return out


@pytest.mark.parametrize("N,S,B,names", [SHAPES[1], SHAPES[0]], ids=[IDS[1], IDS[0]])
def test_inference_from_the_average(N, S, B, names):
    import lstm_hip
    X = _handle(N, S, B, names, adam=False)
    _averaging(X, "ema", 1)
    X.train_windows(5, 0.05)
    avg, p = X.get_average(), X.get_params()
    assert not same_bytes(avg, p)
    Y = lstm_hip.Lstm(N, S, B, flags=_flags(names))
    Y.set_params(avg)
    before, want = _outputs(X, N), _outputs(Y, N)
    X.set_inference_source(lstm_hip.SRC_AVERAGE)
    got = _outputs(X, N)
    assert sorted(got) == sorted(want)
    for key in want:
        assert same_bytes(got[key], want[key]), key
    assert not same_bytes(got["eval_bits"], before["eval_bits"])  # (the two models do differ)
    X.set_inference_source(lstm_hip.SRC_PARAMS)
    again = _outputs(X, N)
    for key in before:
        assert same_bytes(again[key], before[key]), key
    assert same_bytes(X.get_params(), p) and same_bytes(X.get_average(), avg)  # inference changed neither block
    X.close()
    Y.close()


# ---- 5. resume through the public calls ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,every", [("ema", 2), ("uniform", 3)])
@pytest.mark.parametrize("N,S,B,names", SHAPES, ids=IDS)
def test_resume_through_the_public_calls(N, S, B, names, name, every):
    import lstm_hip
    lr = _lr(True)
    X = _handle(N, S, B, names, adam=True)
    _averaging(X, name, every)
    X.train_windows(5, lr)
    R = lstm_hip.Lstm(N, S, B, flags=_flags(names))
    R.set_optimizer(lstm_hip.OPT_ADAM, 0.9, 0.999, 1e-8, 0.01)
    R.set_text(_text())
    _averaging(R, name, every)                      # the order the header gives: set_averaging, set_average, counts
    R.set_average(X.get_average())
    R.set_averaging_counts(*X.averaging_counts())
    for which in (lstm_hip.P_PARAMS, lstm_hip.P_MEM, lstm_hip.P_ADAM_V):
        R.set_params(X.get_params(which), which)
    R.set_optimizer_steps(X.optimizer_steps())
    R.set_cursors(X.get_cursors())
    R.set_window(*X.get_window())
    R.set_state(1, *X.get_state(1))  # the carry column of the next slide
    assert same_bytes(R.get_average(), X.get_average())
    X.train_windows(4, lr)
    R.train_windows(4, lr)
    assert same_bytes(R.get_params(), X.get_params())
    assert same_bytes(R.get_average(), X.get_average())
    assert R.averaging_counts() == X.averaging_counts() == (9, 9 // every)
    X.close()
    R.close()


# ---- 6. padded against explicit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ema", "uniform"])
def test_padded_average_matches_an_explicit_wide_handle(name):
    import lstm_hip
    N, S, B = 100, 6, 4
    Np = padded_width(N, lstm_hip.PAD_HIDDEN)
    assert Np == 128
    P = lstm_hip.init_params(lstm_hip.MT19937Normal(7), N)
    A = _handle(N, S, B, ("PAD_HIDDEN",), adam=False, P=P)
    E = _handle(Np, S, B, (), adam=False, P=pad_params(P, N, Np))  # the explicit handle: the extra units are zero
    for L in (A, E):
        _averaging(L, name, 2)
        L.train_windows(7, 0.05)
    a, e = A.get_average(), E.get_average()
    assert same_bytes(a, unpad_params(e, N, Np))
    assert same_bytes(pad_params(a, N, Np), e)  # ... and the explicit handle's padding entries are 0
    assert A.averaging_counts() == E.averaging_counts() == (7, 3)
    # set_average writes the padding as 0, as set_params does: the round trip is exact
    A.set_average(a)
    assert same_bytes(A.get_average(), a)
    A.close()
    E.close()


# ---- 7. boundary codes -------------------------------------------------------------------------------------------------------
def test_boundary_codes():
    import lstm_hip
    N, S, B = 64, 6, 4
    L = _handle(N, S, B, (), adam=False)
    lib, h = L.lib, L._h
    lib.lstm_hip_set_averaging.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_int32]
    lib.lstm_hip_get_average.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    lib.lstm_hip_set_average.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    lib.lstm_hip_get_averaging_counts.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.lstm_hip_set_averaging_counts.argtypes = [C.c_void_p, C.c_int64, C.c_int64]
    lib.lstm_hip_set_inference_source.argtypes = [C.c_void_p, C.c_int32]
    OFF, EMA, UNI = lstm_hip.AVG_OFF, lstm_hip.AVG_EMA, lstm_hip.AVG_UNIFORM
    EINVAL, ESTATE = lstm_hip.EINVAL, lstm_hip.ESTATE
    buf = np.zeros(L.np, np.float32)
    bp = buf.ctypes.data_as(C.POINTER(C.c_float))
    seen, n = C.c_int64(-1), C.c_int64(-1)
    err = lambda: lib.lstm_hip_last_error().decode()

    def off_answers():  # a handle without averaging
        assert lib.lstm_hip_get_average(h, bp) == ESTATE
        assert lib.lstm_hip_set_average(h, bp) == ESTATE
        assert lib.lstm_hip_get_averaging_counts(h, C.byref(seen), C.byref(n)) == ESTATE
        assert lib.lstm_hip_set_averaging_counts(h, 1, 1) == ESTATE
        assert lib.lstm_hip_set_inference_source(h, lstm_hip.SRC_AVERAGE) == ESTATE

    off_answers()
    nan, inf = math.nan, math.inf
    for args, word in [((3, 0.0, 1), "kind"), ((-1, 0.0, 1), "kind"), ((EMA, nan, 1), "decay"), ((EMA, 1.0, 1), "decay"),
                       ((EMA, -0.1, 1), "decay"), ((EMA, inf, 1), "decay"), ((UNI, 0.5, 1), "decay"), ((UNI, nan, 1), "decay"),
                       ((OFF, 0.5, 1), "decay"), ((EMA, 0.9, 0), "every"), ((UNI, 0.0, -2), "every"), ((OFF, 0.0, 0), "every")]:
        assert lib.lstm_hip_set_averaging(h, *args) == EINVAL, args
        assert word in err(), (args, err())
    off_answers()  # (nothing was accepted)
    assert lib.lstm_hip_set_inference_source(h, 2) == EINVAL and lib.lstm_hip_set_inference_source(h, -1) == EINVAL
    assert lib.lstm_hip_set_inference_source(h, lstm_hip.SRC_PARAMS) == 0
    assert lib.lstm_hip_set_averaging(h, OFF, 0.0, 1) == 0  # off on an off handle: nothing happens
    assert lib.lstm_hip_get_params(h, 4, bp) == EINVAL  # the average is no fifth block

    assert lib.lstm_hip_set_averaging(h, EMA, 0.0, 1) == 0  # the edge of the range is accepted
    assert lib.lstm_hip_get_averaging_counts(h, C.byref(seen), C.byref(n)) == 0 and (seen.value, n.value) == (0, 0)
    buf[:] = 1.0
    assert lib.lstm_hip_get_average(h, bp) == 0 and not np.any(buf)  # n == 0: the zero block
    assert lib.lstm_hip_set_inference_source(h, lstm_hip.SRC_AVERAGE) == ESTATE  # n == 0: a zero model is never meant
    assert lib.lstm_hip_get_average(h, None) == EINVAL and lib.lstm_hip_set_average(h, None) == EINVAL
    assert lib.lstm_hip_get_averaging_counts(h, None, C.byref(n)) == EINVAL
    assert lib.lstm_hip_get_averaging_counts(h, C.byref(seen), None) == EINVAL
    for bad in [(1, 2), (-1, -1), (3, -1)]:
        assert lib.lstm_hip_set_averaging_counts(h, *bad) == EINVAL, bad
    assert lib.lstm_hip_get_averaging_counts(h, C.byref(seen), C.byref(n)) == 0 and (seen.value, n.value) == (0, 0)

    L.train_windows(3, 0.05)  # the handle is still usable, and now has an average
    assert L.averaging_counts() == (3, 3)
    avg = L.get_average()
    assert same_bytes(avg, L.get_params())  # decay 0: the average is the last iterate
    L.set_averaging(EMA, 0.5, 2)  # the same kind again keeps the block and both counters and takes the new numbers
    assert L.averaging_counts() == (3, 3) and same_bytes(L.get_average(), avg)
    L.train_windows(1, 0.05)  # seen = 4: due under every = 2
    assert L.averaging_counts() == (4, 4)
    want = avg + np.float32(0.5) * (L.get_params() - avg)
    assert same_bytes(L.get_average(), want)

    L.set_inference_source(lstm_hip.SRC_AVERAGE)
    texts = [np.full(12, 97, np.uint8)] * B
    off = np.arange(B + 1, dtype=np.uint64) * 12
    code = np.zeros(B * 40, np.uint8)
    code_off = np.zeros(B + 1, np.uint64)
    p8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    data = np.concatenate(texts)
    assert lib.lstm_hip_encode_adaptive(h, p8(data), p64(off), C.c_double(0.05), p8(code), C.c_uint64(code.size), p64(code_off),
                                        None, None, None) == ESTATE
    assert "LSTM_HIP_SRC_AVERAGE" in err()
    assert lib.lstm_hip_decode_adaptive(h, p8(code), p64(code_off), p64(off), C.c_double(0.05), p8(data)) == ESTATE
    assert L.averaging_counts() == (4, 4) and L.optimizer_steps() == 4  # (neither call trained)
    assert lib.lstm_hip_set_averaging_counts(h, 4, 0) == ESTATE  # n = 0 under the average source
    L.set_inference_source(lstm_hip.SRC_PARAMS)
    codes, _, _ = L.encode_adaptive(texts, 0.05)  # back on the parameters the adaptive coder runs, and its train passes count
    assert 12 // (S - 1) == 2 and L.averaging_counts() == (6, 5)  # two train passes; every = 2: the second one is due

    L.set_inference_source(lstm_hip.SRC_AVERAGE)
    L.set_averaging(UNI, 0.0, 1)  # a new kind zeroes the block and the counters; the source goes back to the parameters
    assert L.averaging_counts() == (0, 0) and not np.any(L.get_average())
    assert lib.lstm_hip_set_inference_source(h, lstm_hip.SRC_AVERAGE) == ESTATE
    L.set_averaging_counts(5, 2)
    assert L.averaging_counts() == (5, 2)
    L.train_windows(1, 0.05)
    assert L.averaging_counts() == (6, 3)
    L.set_inference_source(lstm_hip.SRC_AVERAGE)
    b1 = L.eval_bits(np.frombuffer(b"the quick brown fox jumps over the lazy dog", np.uint8))
    L.set_averaging(OFF)  # off: no average, and the source is the parameters again
    off_answers()
    b2 = L.eval_bits(np.frombuffer(b"the quick brown fox jumps over the lazy dog", np.uint8))
    assert np.isfinite(b1) and np.isfinite(b2) and b1 != b2
    L.train_windows(1, 0.05)  # and nothing counts any more
    L.set_averaging(UNI)
    assert L.averaging_counts() == (0, 0)
    L.close()


# ---- 8. the program ---------------------------------------------------------------------------------------------------------
def _read(path):
    return np.loadtxt(path, dtype=np.float64, ndmin=1)


BLOCKS = ("W", "U", "Why", "b", "by")


def test_program_saves_and_resumes_the_average(tmp_path):
    """The program starts every run from freshly drawn states and keeps its parameter checkpoints at 6 digits, so a resumed run
    can equal the uninterrupted one only where neither matters: all three runs start from one saved checkpoint (6-digit
    parameters survive their own round trip) and train at lr = 0, so that what is compared is the average's own resume --
    the block, kept at 9 digits, and both counters across the cut."""
    text = np.random.RandomState(11).randint(97, 110, size=3000).astype(np.uint8)
    f = tmp_path / "corpus.txt"
    text.tofile(f)
    run = lambda args: subprocess.run(args, capture_output=True, text=True, errors="replace", timeout=300)
    base = [LSTM, str(f), "32", "8", "4", "--epochs", "1", "--seed", "1", "--sample", "0", "--quiet"]
    avg = ["--average", "uniform", "--average-every", "2"]
    p0, a, b, c, d = (str(tmp_path / k) for k in ("p0", "a", "b", "c", "d"))
    # a trained run: the average is a checkpoint of its own and differs from the last iterate
    out = run(base + ["--lr", "0.05", "--windows", "21", "--save", p0, "--test-percent", "10"] + avg + ["--average-start", "4"])
    assert out.returncode == 0, out.stderr
    names = sorted(p.name for p in tmp_path.iterdir() if p.name.startswith("p0_avg"))
    assert names == sorted([f"p0_avg_{k}.txt" for k in BLOCKS] + ["p0_avg_state.txt"]), names
    state = dict(line.split() for line in open(p0 + "_avg_state.txt").read().splitlines())
    assert state == {"kind": "uniform", "decay": "0", "every": "2", "seen": "17", "n": "8"}, state  # (on after 4 windows)
    assert np.any(_read(p0 + "_avg_U.txt") != _read(p0 + "_U.txt"))
    assert "Test error of the uniform average (n = 8):" in out.stdout, out.stdout
    assert out.stdout.count("Test error:") == 2  # the report's own two lines are as they were
    # the cut run against the uninterrupted one
    lr0 = ["--lr", "0"]
    out = run(base + lr0 + avg + ["--load", p0, "--windows", "13", "--save", a])
    assert out.returncode == 0, out.stderr
    assert "Loaded the uniform average (seen = 17, n = 8)" in out.stdout, out.stdout
    out = run(base + lr0 + avg + ["--load", a, "--windows", "8", "--save", b])
    assert out.returncode == 0, out.stderr
    assert "Loaded the uniform average (seen = 30, n = 15)" in out.stdout, out.stdout
    out = run(base + lr0 + avg + ["--load", p0, "--windows", "21", "--save", c])
    assert out.returncode == 0, out.stderr
    for k in BLOCKS:
        assert open(f"{b}_avg_{k}.txt").read() == open(f"{c}_avg_{k}.txt").read(), k
    assert open(b + "_avg_state.txt").read() == open(c + "_avg_state.txt").read()
    assert open(c + "_avg_state.txt").read().split() == "kind uniform decay 0 every 2 seen 38 n 19".split()
    # another kind, or no --average, ignores the saved average
    out = run(base + lr0 + ["--average", "ema", "--load", p0, "--windows", "3", "--save", d])
    assert out.returncode == 0 and "Loaded the" not in out.stdout, (out.stdout, out.stderr)
    assert open(d + "_avg_state.txt").read().split() == "kind ema decay 0.999 every 1 seen 3 n 3".split()
    out = run(base + lr0 + ["--load", p0, "--windows", "3"])
    assert out.returncode == 0 and "average" not in out.stdout, out.stdout
    # PREFIX_avg is a parameter checkpoint: the generator loads it
    out = run([GENERATE, "--load", p0 + "_avg", "--prime", "abc", "--count", "8", "--seed", "3"])
    assert out.returncode == 0, (out.stdout, out.stderr)
    last = run([GENERATE, "--load", p0, "--score", str(f)])
    mean = run([GENERATE, "--load", p0 + "_avg", "--score", str(f)])
    assert last.returncode == 0 and mean.returncode == 0 and last.stdout != mean.stdout  # (two different models)
