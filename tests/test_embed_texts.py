"""-m gpu: lstm_hip_embed_texts -- pooled, last and picked hidden states of many texts on lstm_hip_eval_texts' engine
(include/lstm_hip.h).

Against the float64 statement of tests/embed_ref.py on every pair of recurrence forms (the rows of
handle_sequence_cases.SHAPES, a padded N = 100 handle, a per-step handle and a bf16 parent): every element of mean, max and
last within max(2e-5, 8 x H32[N]) (H32: the float32 oracle's own distance from float64, pinned in
tests/test_embed_texts_cpu.py, where the comparison's mutants are).  The call's own arithmetic by bytes -- the pools are the
numpy pooling of the call's own picked states --, picks, placement, bits against eval_texts, the untouched parent, the
inference source, the refusals and the program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import embed_ref as er
import gpu_util as gu
import handle_replay as hr
import handle_sequence_cases as hsc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSTM = os.path.join(ROOT, "eigen-lstm_amd", "lstm")
GEN = os.path.join(ROOT, "eigen-lstm_amd", "lstm_generate")

EXTRA = [hsc.Shape("padded N = 100", 100, 5, 8, ("PAD_HIDDEN",), {}, {}),
         hsc.Shape("per-step engine", 64, 5, 4, ("STEP_KERNELS",), {}, {}),
         hsc.Shape("bf16 parent", 128, 5, 8, ("BF16_RECURRENCE",), {}, {})]
SHAPES = hsc.SHAPES + EXTRA
SKIP = [0, 1, 1, 40, 0, 128, 200, 130, 36, 9]   # per er.LENGTHS: none, past the end, inside, on a window's edge

_reference = {}


def reference(N, orc64):
    """the float64 statement of er.case(N), without and with SKIP, computed once per width and shared"""
    if N not in _reference:
        P, txts, h0, c0 = er.case(N)
        _reference[N] = (P, txts, h0, c0, er.embed(orc64, N, P, txts, h0, c0), er.embed(orc64, N, P, txts, h0, c0, skip=SKIP))
    return _reference[N]


def _handle(N, P, B=4, flags=0, S=3):
    import lstm_hip
    L = lstm_hip.Lstm(N, S, B, flags=flags)
    L.set_params(P)
    return L


def _pool(rows, start, L, skip):
    return er.pool_one(rows, start, L, skip)


@pytest.mark.parametrize("shape", SHAPES, ids=hsc.shape_id)
def test_against_the_float64_statement(shape, oracle64):
    N, K = shape.N, len(er.LENGTHS)
    P, txts, h0, c0, plain, skipped = reference(N, oracle64)
    reps = shape.B // K + 1                      # more streams than the handle's B lanes: every lane holds a queue
    L = hr.create(shape)
    try:
        L.set_params(P)
        kw = dict(h0=np.tile(h0, (reps, 1)), c0=np.tile(c0, (reps, 1)))
        runs = [(L.embed_texts(list(txts) * reps, cell=True, **kw), plain, True),
                (L.embed_texts(list(txts) * reps, skip=SKIP * reps, **kw), skipped, False)]
    finally:
        L.close()
    worst = {}
    for got, want, cell in runs:
        assert len(got["count"]) == K * reps > shape.B
        assert ("mean_c" in got) == cell
        for r in range(reps):
            part = {k: v[r * K:(r + 1) * K] for k, v in got.items() if k != "ms"}
            figures, fails = er.compare(part, want, N, cell=cell)
            worst.update({k: max(worst.get(k, 0.0), v) for k, v in figures.items()})
            assert not fails, (hsc.shape_id(shape), r, fails, figures)
            assert all(np.isfinite(part[k]).all() for k in figures)
    print(f"{hsc.shape_id(shape)}: within " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())) +
          f" (tolerance {er.tolerance(N):.3g})")


@pytest.mark.parametrize("shape", [SHAPES[2], EXTRA[0], EXTRA[1]], ids=hsc.shape_id)
def test_pools_are_the_pooling_of_the_calls_own_states(shape):
    """bit for bit within one call: mean / max / last equal the numpy pooling of that call's own picked states"""
    N = shape.N
    P, txts, h0, c0 = er.case(N)
    off = np.concatenate([[0], np.cumsum(er.LENGTHS)]).astype(int)
    L = hr.create(shape)
    try:
        L.set_params(P)
        got = L.embed_texts(txts, h0=h0, c0=c0, skip=SKIP, cell=True, pick="all")
        again = L.embed_texts(txts, h0=h0, c0=c0, skip=SKIP, cell=True, pick="all")
        subset = np.array([0, 1, 2, 3, 129, 130, 257, 258, 300, 385, 386, 387, 514, 642, 643, 899, 900, 936, 937, 941], np.uint64)
        some = L.embed_texts(txts, h0=h0, c0=c0, skip=SKIP, cell=True, pick=subset, pool=("last",))
        only_c = L.embed_texts(txts, h0=h0, c0=c0, pool=(), pick=subset)
    finally:
        L.close()
    assert got["picked_h"].shape == got["picked_c"].shape == (off[-1], N) and off[-1] == 942
    assert all(got[k].tobytes() == again[k].tobytes() for k in got if k != "ms")
    for x, start in (("h", h0), ("c", c0)):
        for s, n in enumerate(er.LENGTHS):
            rows = got[f"picked_{x}"][off[s]:off[s + 1]]
            mean, mx, last, count = _pool(rows, start[s], n, SKIP[s])
            assert count == got["count"][s]
            assert mean.tobytes() == got[f"mean_{x}"][s].tobytes(), (x, s)
            assert mx.tobytes() == got[f"max_{x}"][s].tobytes(), (x, s)
            assert last.tobytes() == got[f"last_{x}"][s].tobytes(), (x, s)
            if n:
                assert got[f"last_{x}"][s].tobytes() == got[f"picked_{x}"][off[s + 1] - 1].tobytes()
                assert not np.array_equal(rows[-1], start[s])
        # a subset of picks is the same columns of the "all" call, byte for byte
        assert some[f"picked_{x}"].tobytes() == got[f"picked_{x}"][subset.astype(int)].tobytes()
        assert some[f"last_{x}"].tobytes() == got[f"last_{x}"].tobytes() and f"mean_{x}" not in some
    assert "picked_c" not in only_c and "last_h" not in only_c and only_c["picked_h"].shape == (subset.size, N)
    assert list(got["count"]) == [0, 0, 1, 87, 128, 1, 56, 127, 1, 0]
    for s in (0, 1, 9):                            # empty pools: +0.0f
        for k in ("mean_h", "max_h", "mean_c", "max_c"):
            assert not got[k][s].any() and not np.signbit(got[k][s]).any()


def test_placement_changes_nothing_past_the_tolerance():
    N = 128
    lengths = [257, 3, 130, 40, 0, 129, 64, 128, 1]
    P = gu.random_case(N, 2, 1, seed=21)[0]
    txts = er.texts(lengths, seed=22)
    L = _handle(N, P, B=4)
    runs = [L.embed_texts(txts, lanes=lanes, cell=True, pick="all") for lanes in (1, 0, 16)]
    L.close()
    for other in runs[1:]:
        assert np.array_equal(other["count"], runs[0]["count"])
        for k in runs[0]:
            if k not in ("count", "bits", "ms"):
                assert np.allclose(other[k], runs[0][k], rtol=0, atol=er.ACT_TOL), k
    same = all(o[k].tobytes() == runs[0][k].tobytes() for o in runs[1:] for k in o if k != "ms")
    print("placement: bit-equal" if same else "placement: within tolerance, not bit-equal")


def test_bits_are_eval_texts_bits():
    import eval_texts_ref as ev
    N = 64
    lengths = [200, 131, 5, 64, 0, 1, 129, 128]
    skip = [130, 1, 9, 0, 0, 0, 128, 2]
    P = gu.random_case(N, 2, 1, seed=41)[0]
    txts = er.texts(lengths, seed=42)
    L = _handle(N, P, B=2)
    for sk in (None, skip):
        want = L.eval_texts(txts, skip=sk)
        got = L.embed_texts(txts, skip=sk, pool=("last",))
        cnt = ev.scored(lengths, sk)
        assert (np.abs(got["bits"] - want["bits"]) <= er.BITS_TOL * cnt).all(), (got["bits"], want["bits"])
        assert (got["bits"][cnt == 0] == 0).all() and (got["bits"][cnt > 0] > 0).all()
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
        ev0 = A.eval_texts(held, surprisal=True)
        r = A.embed_texts(held, cell=True, pick=[0, 299, 300, 468])
        assert all(np.isfinite(v).all() for k, v in r.items() if k != "ms") and r["bits"][0] > 0
        A.embed_texts(held, lanes=3)
        ev1 = A.eval_texts(held, surprisal=True)
        assert ev0["bits"].tobytes() == ev1["bits"].tobytes() and ev0["h"].tobytes() == ev1["h"].tobytes()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(ev0["surprisal"], ev1["surprisal"]))
        hr.assert_same(before, hr.snapshot(A, text), "embed_texts must leave the handle as it was")
        assert A.kernel_stats() == stats and A.optimizer_steps() == steps and A.lib.lstm_hip_kernel_stat_count(A._h) == count
        la, lt = A.train_windows(3, hr.LR), twin.train_windows(3, hr.LR)
        assert la.tobytes() == lt.tobytes()
        hr.assert_same(hr.snapshot(A, text), hr.snapshot(twin, text), "training after embed_texts against a twin that never embedded")
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
    own = L.embed_texts(held)
    L.set_inference_source(lstm_hip.SRC_AVERAGE)
    avg = L.embed_texts(held)
    L.set_inference_source(lstm_hip.SRC_PARAMS)
    M = _handle(N, L.get_average(), B=B, S=S)
    twin = M.embed_texts(held)
    M.close()
    for k in ("mean_h", "max_h", "last_h", "bits"):
        assert twin[k].tobytes() == avg[k].tobytes() and avg[k].tobytes() != own[k].tobytes(), k
    L.set_weight_drop(0.5, seed=7)
    dropped = L.embed_texts(held)
    assert all(dropped[k].tobytes() == own[k].tobytes() for k in ("mean_h", "max_h", "last_h", "bits"))
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
    last, picked = np.zeros((2, N), np.float32), np.zeros((3, N), np.float32)
    Emb, Opt = lstm_hip._Embedding, lstm_hip._EvalOpt

    def outputs(size=C.sizeof(Emb), with_picked=False, with_picked_c=False):
        out = Emb(size=size)
        out.last_h = p(last)
        if with_picked:
            out.picked_h = p(picked)
        if with_picked_c:
            out.picked_c = p(picked)
        return out

    def call(streams=2, text=text, off=off, opt=None, pick=None, npick=0, out=outputs()):
        pk = None if pick is None else np.asarray(pick, np.uint64)
        return L.lib.lstm_hip_embed_texts(L._h, C.c_int32(streams), p(text, C.c_uint8) if text is not None else None,
                                          p(off, C.c_uint64) if off is not None else None, None, None, None,
                                          C.byref(opt) if opt is not None else None, p(pk, C.c_uint64) if pk is not None else None,
                                          C.c_int64(npick), C.byref(out) if out is not None else None, None)

    wp = outputs(with_picked=True)
    gib = (1 << 30) // (N * 4)
    for kw, message in (
            (dict(opt=Opt(4, 0)), "embed_texts: options of 4 bytes, expected 8"),
            (dict(opt=Opt(8, -1)), "embed_texts: lanes must be in [0, 4096] (got -1)"),
            (dict(opt=Opt(8, 4097)), "embed_texts: lanes must be in [0, 4096] (got 4097)"),
            (dict(streams=0), "embed_texts: streams must be >= 1 (got 0)"),
            (dict(off=None), "embed_texts: null text_off"),
            (dict(off=np.array([1, 4, 10], np.uint64)), "embed_texts: text_off[0] must be 0 (got 1)"),
            (dict(off=np.array([0, 11, 10], np.uint64)), "embed_texts: text_off decreases at stream 1 (10 < 11)"),
            (dict(text=None), "embed_texts: null text with 10 bytes to read"),
            (dict(out=None), "embed_texts: null out"),
            (dict(out=outputs(size=8)), f"embed_texts: outputs of 8 bytes, expected {C.sizeof(Emb)}"),
            (dict(npick=-1, out=wp), "embed_texts: npick must be >= 0 (got -1)"),
            (dict(npick=2, out=wp), "embed_texts: null pick with npick = 2"),
            (dict(pick=[3, 10], npick=2, out=wp), "embed_texts: pick[1] = 10 is not below text_off[streams] = 10"),
            (dict(pick=[3, 3], npick=2, out=wp), "embed_texts: pick must be strictly increasing (pick[1] = 3 after 3)"),
            (dict(pick=[5, 2], npick=2, out=wp), "embed_texts: pick must be strictly increasing (pick[1] = 2 after 5)"),
            (dict(out=wp), "embed_texts: picked_h / picked_c given with npick = 0"),
            (dict(pick=[1, 2], npick=2), "embed_texts: npick = 2 with neither picked_h nor picked_c")):
        assert call(**kw) == lstm_hip.EINVAL, kw
        assert L.lib.lstm_hip_last_error().decode() == message, (kw, L.lib.lstm_hip_last_error())
    # a picked block above 1 GiB (the positions themselves are in range and increasing; the text is never read)
    big_text, n_big = np.zeros(1, np.uint8), gib // 2 + 1
    big_off = np.array([0, n_big], np.uint64)
    big_pick = np.arange(n_big, dtype=np.uint64)
    assert call(streams=1, text=big_text, off=big_off, pick=big_pick, npick=n_big,
                out=outputs(with_picked=True, with_picked_c=True)) == lstm_hip.EINVAL
    assert L.lib.lstm_hip_last_error().decode() == \
        f"embed_texts: {n_big} picked positions of width {N} from 2 source(s) need more than {1 << 30} bytes"
    assert L.kernel_stats() == stats               # nothing ran on the handle
    assert call() == 0 and last.any()              # and it still works: opt NULL = the handle's B lanes
    assert call(pick=[0, 3, 9], npick=3, out=wp) == 0 and picked.any()
    assert picked[1].tobytes() == last[0].tobytes() and picked[2].tobytes() == last[1].tobytes()
    assert call(text=None, off=np.zeros(3, np.uint64)) == 0 and not last.any()   # no bytes to read: the zero start states
    L.close()


@pytest.mark.parametrize("pool,cell", [("concat", True), ("mean", False), (None, False)])
def test_program_embeds_records(tmp_path, pool, cell):
    import lstm_hip
    rs = np.random.RandomState(12)
    data = bytes(rs.randint(97, 123, size=700).astype(np.uint8))
    corpus = tmp_path / "train.txt"
    corpus.write_bytes(data)
    ck = tmp_path / "ck"
    out = subprocess.run([LSTM, str(corpus), "32", "8", "4", "0.05", "--epochs", "1", "--windows", "10", "--seed", "1",
                          "--sample", "0", "--save", str(ck), "--quiet"], capture_output=True, text=True, errors="replace", timeout=120)
    assert out.returncode == 0, out.stderr
    records = [b"abc|", b"|", b"x" * 200 + b"|", b"hello world|", b"tail without its delimiter"]
    f, dest = tmp_path / "records.txt", tmp_path / "emb.tsv"
    f.write_bytes(b"".join(records))
    args = [GEN, "--load", str(ck), "--embed", str(f), "--embed-delim", str(ord("|")), "--embed-streams", "3", "--embed-out", str(dest)]
    out = subprocess.run(args + (["--pool", pool] if pool else []) + (["--embed-cell"] if cell else []), capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rows = np.array([[np.float32(v) for v in line.split("\t")] for line in dest.read_text().splitlines()], np.float32)
    N = 32
    P = np.concatenate([np.loadtxt(f"{ck}_{k}.txt", dtype=np.float32, ndmin=2).ravel(order="F") for k in ("W", "U", "b", "Why", "by")])
    L = lstm_hip.Lstm(N, 2, 1, flags=lstm_hip.PAD_HIDDEN)
    L.set_params(P)
    r = L.embed_texts(records, lanes=3, cell=cell)
    L.close()
    names = {"concat": ("last", "max", "mean"), "mean": ("mean",), None: ("last",)}[pool]
    want = np.concatenate([r[f"{k}_{x}"] for x in ("hc" if cell else "h") for k in names], axis=1)
    assert rows.shape == want.shape == (5, N * len(names) * (2 if cell else 1))
    assert rows.tobytes() == want.tobytes()        # %.9g round-trips a float32


def test_program_usage_errors(tmp_path):
    f = tmp_path / "r.txt"
    f.write_bytes(b"a\nb\n")
    base = [GEN, "--load", str(tmp_path / "none")]
    for extra, word in ((["--embed", str(f)], "--embed needs --embed-out OUT"),
                        (["--embed-out", "x"], "--embed-out needs --embed"),
                        (["--pool", "mean", "--count", "3"], "--pool needs --embed"),
                        (["--embed", str(f), "--embed-out", "x", "--count", "3"], "--embed goes with neither --count nor --score"),
                        (["--embed", str(f), "--embed-out", "x", "--score", str(f)], "--embed goes with neither --count nor --score"),
                        (["--embed", str(f), "--embed-out", "x", "--pool", "sum"], "--pool needs one of last, mean, max, concat, got 'sum'"),
                        (["--embed", str(f), "--embed-out", "x", "--embed-streams", "0"], "--embed-streams needs an integer in [1, 4096]"),
                        (["--embed", str(f), "--embed-out", "x", "--embed-delim", "256"], "--embed-delim needs an integer in [0, 255]")):
        bad = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert bad.returncode == 2 and word in bad.stderr, (extra, bad.stderr)
