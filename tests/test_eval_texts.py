"""-m gpu: lstm_hip_eval_texts -- held-out bits of many texts on the training window's forward path (include/lstm_hip.h,
DESIGN.md section 3.17).

Against the float64 statement of tests/eval_texts_ref.py on every pair of recurrence forms (the rows of
handle_sequence_cases.SHAPES, a padded N = 100 handle, a per-step handle and a bf16 parent): per-stream bits within 2e-5 per
scored byte, per-byte surprisal within 8 x D32 (the float32 statement's own distance from float64, pinned in
tests/test_eval_texts_cpu.py, where the comparison's mutants are).  The reference's fixtures, the call's own arithmetic by
bytes, placement, chaining, skip, the untouched parent, the inference source, the refusals and the program."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import eval_texts_ref as er
import gpu_util as gu
import handle_replay as hr
import handle_sequence_cases as hsc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSTM = os.path.join(ROOT, "eigen-lstm_amd", "lstm")
ACT_TOL = 2e-5      # tests/test_hip_parity.py
FIXTURE_TOL = 1e-4  # bits/char: tests/test_hip_parity.py against expected_bits

EXTRA = [hsc.Shape("padded N = 100", 100, 5, 8, ("PAD_HIDDEN",), {}, {}),
         hsc.Shape("per-step engine", 64, 5, 4, ("STEP_KERNELS",), {}, {}),
         hsc.Shape("bf16 parent", 128, 5, 8, ("BF16_RECURRENCE",), {}, {})]
SHAPES = hsc.SHAPES + EXTRA

_reference = {}


def reference(N, orc64):
    """the float64 statement of er.case(N), computed once per width and shared"""
    if N not in _reference:
        P, txts, h0, c0 = er.case(N)
        _reference[N] = (P, txts, h0, c0, er.eval64(orc64, N, P, txts, h0, c0))
    return _reference[N]


def _handle(N, P, B=4, flags=0, S=3):
    import lstm_hip
    L = lstm_hip.Lstm(N, S, B, flags=flags)
    L.set_params(P)
    return L


def _same(a, b):
    if a["bits"].tobytes() != b["bits"].tobytes() or a["h"].tobytes() != b["h"].tobytes() or a["c"].tobytes() != b["c"].tobytes():
        return False
    return all(x.tobytes() == y.tobytes() for x, y in zip(a["surprisal"], b["surprisal"]))


@pytest.mark.parametrize("shape", SHAPES, ids=hsc.shape_id)
def test_against_the_float64_statement(shape, oracle64):
    N, K = shape.N, len(er.LENGTHS)
    P, txts, h0, c0, want = reference(N, oracle64)
    reps = shape.B // K + 1                      # more streams than the handle's B lanes: every lane holds a queue
    L = hr.create(shape)
    try:
        L.set_params(P)
        got = L.eval_texts(list(txts) * reps, h0=np.tile(h0, (reps, 1)), c0=np.tile(c0, (reps, 1)), surprisal=True)
    finally:
        L.close()
    assert len(got["bits"]) == K * reps > shape.B
    worst = dict(surprisal=0.0, bits_per_byte=0.0)
    for r in range(reps):
        part = dict(bits=got["bits"][r * K:(r + 1) * K], surprisal=got["surprisal"][r * K:(r + 1) * K])
        figures, fails = er.compare(part, want, N)
        worst = {k: max(worst[k], figures[k]) for k in worst}
        assert not fails, (hsc.shape_id(shape), r, fails, figures)
    print(f"{hsc.shape_id(shape)}: surprisal within {worst['surprisal']:.3g} bits (8 x D32 = {er.SUR_FACTOR * er.D32[N]:.3g}), "
          f"bits per scored byte within {worst['bits_per_byte']:.3g}")


@pytest.mark.parametrize("name", ["A", "B"])
def test_fixtures_as_one_stream(name):
    fx = gu.fixture(name)
    text = np.asarray(fx["text"], np.uint8)
    L = _handle(fx["N"], fx["params"], B=1, S=2)
    got = L.eval_texts([text])["bits"][0] / (text.size - 1)
    old = L.eval_bits(text)
    L.close()
    assert abs(got - fx["bits"]) <= FIXTURE_TOL, (got, fx["bits"])
    assert abs(got - old) <= FIXTURE_TOL, (got, old)


@pytest.mark.parametrize("flags", [0, 512])       # LSTM_HIP_STABLE_SOFTMAX
def test_by_bytes(flags):
    N, lengths = 64, [0, 1, 2, 300, 129, 17]
    P = gu.random_case(N, 2, 1, seed=8)[0]
    txts = er.texts(lengths, seed=9)
    rs = np.random.RandomState(10)
    h0, c0 = (rs.randn(6, N) * 0.1).astype(np.float32), (rs.randn(6, N) * 0.1).astype(np.float32)
    L = _handle(N, P, B=4, flags=flags)
    a = L.eval_texts(txts, h0=h0, c0=c0, surprisal=True)
    b = L.eval_texts(txts, h0=h0, c0=c0, surprisal=True)
    L.close()
    assert _same(a, b)
    for s, n in enumerate(lengths):
        total = 0.0
        for v in a["surprisal"][s]:               # the double sum in text order
            total += float(v)
        assert total == a["bits"][s], s
        assert a["surprisal"][s].size == n and (n == 0 or a["surprisal"][s][0] == 0)
        assert (a["surprisal"][s][1:] > 0).all() and np.isfinite(a["surprisal"][s]).all()
        if n <= 1:                                # no byte is fed: the start state comes back
            assert a["bits"][s] == 0 and np.array_equal(a["h"][s], h0[s]) and np.array_equal(a["c"][s], c0[s])
        else:
            assert not np.array_equal(a["h"][s], h0[s])
    # bits alone (no per-byte array) are the same bits
    L = _handle(N, P, B=4, flags=flags)
    c = L.eval_texts(txts, h0=h0, c0=c0)
    L.close()
    assert c["surprisal"] is None and c["bits"].tobytes() == a["bits"].tobytes()


def test_placement_changes_nothing_past_the_tolerance():
    N = 128
    lengths = [257, 3, 130, 40, 0, 129, 64]
    P = gu.random_case(N, 2, 1, seed=21)[0]
    txts = er.texts(lengths, seed=22)
    L = _handle(N, P, B=4)
    runs = [L.eval_texts(txts, lanes=lanes, surprisal=True) for lanes in (1, 0, 16)]
    L.close()
    cnt = er.scored(lengths)
    for other in runs[1:]:
        assert (np.abs(other["bits"] - runs[0]["bits"]) <= er.BITS_TOL * cnt).all(), (other["bits"], runs[0]["bits"])
        assert np.allclose(other["h"], runs[0]["h"], rtol=0, atol=ACT_TOL)
    print("placement: bit-equal" if all(_same(runs[0], o) for o in runs[1:]) else "placement: within tolerance, not bit-equal")


def test_chaining_overlaps_by_one_byte(oracle64):
    N, n = 64, 300
    P = gu.random_case(N, 2, 1, seed=31)[0]
    text = gu.text_bytes(n, 32)
    rs = np.random.RandomState(33)
    h0, c0 = (rs.randn(1, N) * 0.1).astype(np.float32), (rs.randn(1, N) * 0.1).astype(np.float32)
    L = _handle(N, P, B=2)
    whole = L.eval_texts([text], h0=h0, c0=c0)
    total, h, c = 0.0, h0, c0
    for a, b in ((0, 100), (99, 228), (227, n)):  # 100 bytes, 129 bytes, the rest; each piece starts with the last byte again
        r = L.eval_texts([text[a:b]], h0=h, c0=c)
        total, h, c = total + r["bits"][0], r["h"], r["c"]
    L.close()
    want = er.eval64(oracle64, N, P, [text], h0, c0)
    tol = er.BITS_TOL * (n - 1)
    assert abs(total - whole["bits"][0]) <= tol and abs(total - want["bits"][0]) <= tol and abs(whole["bits"][0] - want["bits"][0]) <= tol
    S = n                                          # the oracle's state after bytes 0 .. n - 2
    xi = np.full((S, 1), -1, np.int32)
    xi[1:, 0] = text[:n - 1]
    fw = oracle64.forward(N, 256, S, 1, P, xi, np.full((S, 1), -1, np.int32), h0, c0)
    for got in (h, whole["h"]):
        assert gu.max_rel(got[0], fw["h"][S - 1, 0]) <= ACT_TOL
    assert gu.max_rel(c[0], fw["c"][S - 1, 0]) <= ACT_TOL


def test_skip_and_split(oracle64):
    N = 64
    lengths = [200, 131, 5, 64]
    skip = [130, 1, 9, 0]
    P = gu.random_case(N, 2, 1, seed=41)[0]
    txts = er.texts(lengths, seed=42)
    L = _handle(N, P, B=2)
    plain = L.eval_texts(txts, surprisal=True)
    got = L.eval_texts(txts, skip=skip, surprisal=True)
    assert got["h"].tobytes() == plain["h"].tobytes()
    for s, k in enumerate(skip):
        assert not got["surprisal"][s][:k].any()
        assert got["surprisal"][s][k:].tobytes() == plain["surprisal"][s][k:].tobytes()
        assert got["bits"][s] == sum(float(v) for v in got["surprisal"][s])
    assert got["bits"][2] == 0 and got["bits"][3] == plain["bits"][3] and got["bits"][1] == plain["bits"][1]
    L.close()
    fx = gu.fixture("A")
    text = np.asarray(fx["text"], np.uint8)
    L = _handle(fx["N"], fx["params"], B=4)
    for warm in (0, 64):
        for pieces in (1, 5):
            want = er.split_bits64(oracle64, fx["N"], fx["params"], text, pieces, warm)
            got = L.eval_split(text, pieces, warm=warm)
            assert abs(got - want) <= er.BITS_TOL, (pieces, warm, got, want)
    L.close()


@pytest.mark.parametrize("shape", [s for s in SHAPES if s.forms in hsc.INFERENCE_ROWS], ids=hsc.shape_id)
def test_the_parent_is_untouched(shape):
    text = np.frombuffer(bytes(gu.text_bytes(4000, 51)), np.uint8)
    held = er.texts([300, 0, 129, 40], seed=52)
    A, twin = hr.start(shape, text), None
    try:
        A.train_windows(2, hr.LR)
        before = hr.snapshot(A, text)
        stats, steps, count = A.kernel_stats(), A.optimizer_steps(), A.lib.lstm_hip_kernel_stat_count(A._h)
        twin = hr.restore(shape, before)
        r = A.eval_texts(held, surprisal=True)
        assert np.isfinite(r["bits"]).all() and r["bits"][0] > 0
        A.eval_texts(held, lanes=3)
        hr.assert_same(before, hr.snapshot(A, text), "eval_texts must leave the handle as it was")
        assert A.kernel_stats() == stats and A.optimizer_steps() == steps and A.lib.lstm_hip_kernel_stat_count(A._h) == count
        la, lt = A.train_windows(3, hr.LR), twin.train_windows(3, hr.LR)
        assert la.tobytes() == lt.tobytes()
        hr.assert_same(hr.snapshot(A, text), hr.snapshot(twin, text), "training after eval_texts against a twin that never evaluated")
    finally:
        A.close()
        if twin is not None:
            twin.close()


def test_inference_source_and_weight_drop():
    import lstm_hip
    N, S, B = 128, 5, 8
    text = np.frombuffer(bytes(gu.text_bytes(3000, 61)), np.uint8)
    held = er.texts([200, 64], seed=62)
    L = lstm_hip.Lstm(N, S, B)
    L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(3), N))
    L.set_text(text)
    L.set_cursors(lstm_hip.initial_cursors(len(text), S, B))
    L.set_averaging(lstm_hip.AVG_EMA, decay=0.5)
    L.train_windows(4, 0.05)
    own = L.eval_texts(held)["bits"]
    L.set_inference_source(lstm_hip.SRC_AVERAGE)
    avg = L.eval_texts(held)["bits"]
    L.set_inference_source(lstm_hip.SRC_PARAMS)
    M = _handle(N, L.get_average(), B=B, S=S)
    assert M.eval_texts(held)["bits"].tobytes() == avg.tobytes() and avg.tobytes() != own.tobytes()
    M.close()
    L.set_weight_drop(0.5, seed=7)
    assert L.eval_texts(held)["bits"].tobytes() == own.tobytes()
    assert L.weight_drop()[0] == 0.5
    L.close()


def test_refusals_launch_nothing():
    import lstm_hip
    N = 64
    L = _handle(N, gu.random_case(N, 2, 1, seed=71)[0], B=2)
    L.set_profiling(True)
    stats = L.kernel_stats()
    p = lstm_hip._ptr
    text = np.arange(10, dtype=np.uint8)
    off = np.array([0, 4, 10], np.uint64)
    bits = np.zeros(2)

    def call(streams=2, text=text, off=off, opt=None):
        return L.lib.lstm_hip_eval_texts(L._h, C.c_int32(streams), p(text, C.c_uint8) if text is not None else None,
                                         p(off, C.c_uint64) if off is not None else None, None, None, None,
                                         C.byref(opt) if opt is not None else None, p(bits, C.c_double), None, None, None, None)

    Opt = lstm_hip._EvalOpt
    for kw, word in ((dict(opt=Opt(4, 0)), "options of 4 bytes"), (dict(opt=Opt(8, -1)), "lanes must be in [0, 4096]"),
                     (dict(opt=Opt(8, 4097)), "lanes must be in [0, 4096]"), (dict(streams=0), "streams must be >= 1"),
                     (dict(off=None), "null text_off"), (dict(off=np.array([1, 4, 10], np.uint64)), "must be 0"),
                     (dict(off=np.array([0, 11, 10], np.uint64)), "decreases"), (dict(text=None), "null text with 10 bytes")):
        assert call(**kw) == lstm_hip.EINVAL, kw
        assert word in L.lib.lstm_hip_last_error().decode(), (kw, L.lib.lstm_hip_last_error())
    assert L.kernel_stats() == stats               # nothing ran on the handle
    assert call() == 0 and bits[0] > 0 and bits[1] > 0   # and it still works: opt NULL = the handle's B lanes
    assert call(text=None, off=np.zeros(3, np.uint64)) == 0   # no bytes to read: no text needed
    L.close()


def test_program_test_streams(tmp_path):
    rs = np.random.RandomState(11)
    words = [bytes(rs.randint(97, 123, size=rs.randint(2, 8)).astype(np.uint8)) for _ in range(40)]
    f = tmp_path / "corpus.txt"
    f.write_bytes(b" ".join(words[i] for i in rs.randint(0, 40, size=600))[:2500])
    args = [LSTM, str(f), "32", "8", "4", "0.05", "--epochs", "1", "--windows", "20", "--seed", "1", "--sample", "0",
            "--eval-file", str(f), "--quiet"]
    figures = []
    for extra in ([], ["--test-streams", "1"], ["--test-streams", "7", "--test-warmup", "100000"]):
        out = subprocess.run(args + extra, capture_output=True, text=True, errors="replace", timeout=120)
        assert out.returncode == 0, out.stderr
        m = re.search(r"Test error: ([\d.]+) bits/char", out.stdout)
        assert m, out.stdout
        figures.append(float(m.group(1)))
    assert abs(figures[1] - figures[0]) <= 1e-4 and abs(figures[2] - figures[0]) <= 1e-4, figures
    bad = subprocess.run(args + ["--test-warmup", "5"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--test-warmup needs --test-streams" in bad.stderr


def test_program_score_streams(tmp_path):
    rs = np.random.RandomState(12)
    files = []
    for i, n in enumerate((700, 131)):
        files.append(tmp_path / f"text{i}.txt")
        files[-1].write_bytes(bytes(rs.randint(97, 123, size=n).astype(np.uint8)))
    ck = tmp_path / "ck"
    out = subprocess.run([LSTM, str(files[0]), "32", "8", "4", "0.05", "--epochs", "1", "--windows", "10", "--seed", "1",
                          "--sample", "0", "--save", str(ck), "--quiet"], capture_output=True, text=True, errors="replace", timeout=120)
    assert out.returncode == 0, out.stderr
    gen = os.path.join(ROOT, "eigen-lstm_amd", "lstm_generate")
    lines = []
    for extra in ([], ["--score-streams", "1"], ["--score-streams", "4", "--score-warmup", "100000"]):
        out = subprocess.run([gen, "--load", str(ck), "--score"] + [str(f) for f in files] + extra, capture_output=True, text=True,
                             timeout=120)
        assert out.returncode == 0, out.stderr
        lines.append([float(v) for v in re.findall(r": ([\d.]+) bits/char", out.stdout)])
        assert len(lines[-1]) == 3, out.stdout     # two files and the total
    for other in lines[1:]:
        assert np.abs(np.array(other) - np.array(lines[0])).max() <= 1e-4, lines
    bad = subprocess.run([gen, "--load", str(ck), "--count", "5", "--score-streams", "2"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--score-streams needs --score" in bad.stderr
