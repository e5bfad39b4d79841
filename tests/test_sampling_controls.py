"""-m gpu: lstm_hip_generate_ex -- top-k, nucleus and stop-byte sampling in the batched generator (include/lstm_hip.h,
DESIGN.md section 3.8).

With the controls off the call is lstm_hip_generate bit for bit; top_k = 1 is greedy decoding bit for bit; against the
oracle every drawn byte lies in the float64 reference's kept set (tests/sampling_ref.py), `kept` is its count and the draw
lies in the byte's renormalised interval, with the thresholds of test_temperature_and_greedy_against_the_oracle; a stopped
stream is the prefix of the unstopped one with the same draws."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sampling_ref as sr
from oracle_lib import split_params
from test_pad_hidden import pad_cols, pad_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 256
FILTERS = dict(top_k=40, top_p=0.9, temperature=0.8)


def _state(streams, N, seed):
    rs = np.random.RandomState(seed)
    return (rs.randn(streams, N) * 0.1).astype(np.float32), (rs.randn(streams, N) * 0.1).astype(np.float32)


def _prompts(lengths, seed):
    rs = np.random.RandomState(seed)
    return [rs.randint(32, 127, size=n).astype(np.uint8) for n in lengths]


def _same(a, b):
    """the first four results (out, bits, h, c) agree bit for bit"""
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a[:4], b[:4]))


@pytest.mark.parametrize("N,flags", [(128, 0), (512, 0), (128, 512)])  # 512: LSTM_HIP_STABLE_SOFTMAX
def test_defaults_are_the_old_call(N, flags):
    import lstm_hip
    K, Cn = 7, 60
    P = sr.peaked_params(N, seed=3, scale=0.1)
    prompts = _prompts([0, 1, 2, 9, 40, 130, 5], seed=4)
    h0, c0 = _state(K, N, seed=5)
    u = np.random.RandomState(6).random_sample((Cn, K))
    L = lstm_hip.Lstm(N, 2, 1, flags=flags)
    L.set_params(P)
    for tau in (1.0, 0.7, 0.0):
        kw = dict(count=Cn, u=u, temperature=tau, h0=h0, c0=c0, score=True)
        old = L.generate(prompts, **kw)
        off = L.generate(prompts, info=True, **kw)  # lstm_hip_generate_ex with everything off
        assert len(old) == 4 and len(off) == 5
        assert _same(old, off), tau
        assert (off[4]["out_len"] == Cn).all() and (off[4]["kept"] == (1 if tau == 0.0 else 256)).all()
        assert _same(old, L.generate(prompts, top_k=256, **kw)), tau
        assert _same(old, L.generate(prompts, top_k=256, top_p=1.0, stop_byte=None, info=True, **kw)), tau
    L.close()


@pytest.mark.parametrize("tau", [1.0, 0.7])
def test_top_k_one_is_greedy(tau):
    import lstm_hip
    N, K, Cn = 128, 9, 120
    P = sr.peaked_params(N, seed=11, scale=0.1)
    prompts = _prompts([3, 0, 17, 40, 1, 9, 2, 2, 60], seed=12)
    h0, c0 = _state(K, N, seed=13)
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(P)
    greedy = L.generate(prompts, count=Cn, u=None, temperature=0.0, h0=h0, c0=c0)
    for seed in (14, 15):
        u = np.random.RandomState(seed).random_sample((Cn, K))
        got = L.generate(prompts, count=Cn, u=u, temperature=tau, h0=h0, c0=c0, top_k=1, info=True)
        assert np.array_equal(got[0], greedy[0]), (tau, seed)
        assert np.array_equal(got[2], greedy[2]) and np.array_equal(got[3], greedy[3])
        assert (got[4]["kept"] == 1).all()
        tiny = L.generate(prompts, count=Cn, u=u, temperature=tau, h0=h0, c0=c0, top_p=1e-30, info=True)
        assert np.array_equal(tiny[0], greedy[0]), (tau, seed)
        assert np.array_equal(tiny[2], greedy[2]) and np.array_equal(tiny[3], greedy[3])
        assert (tiny[4]["kept"] == 1).all()
    # the unfiltered draws of the same u are something else (the options are not ignored)
    free = L.generate(prompts, count=Cn, u=u, temperature=tau, h0=h0, c0=c0)
    assert not np.array_equal(free[0], greedy[0])
    L.close()


@pytest.mark.parametrize("top_k,top_p,tau", sr.ORACLE_SETTINGS)
def test_filtered_draws_against_the_oracle(top_k, top_p, tau, oracle32):
    """As test_temperature_and_greedy_against_the_oracle: the drawn bytes are fed back through the oracle, and the float64
    reference filter is applied to each step's distribution.  Ambiguous draws (tests/sampling_ref.py; their share on
    oracle trajectories is what tests/test_sampling_controls_cpu.py controls) are skipped, at most 5 % of them."""
    import lstm_hip
    N, K, Cn = sr.ORACLE_N, sr.ORACLE_STREAMS, sr.ORACLE_COUNT
    P, prompts, u = sr.oracle_case()
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(P)
    out, _, _, _, info = L.generate(prompts, count=Cn, u=u, temperature=tau, top_k=top_k, top_p=top_p, info=True)
    L.close()
    kept = info["kept"]
    skipped = checked = inside = near = 0
    keeps = []
    for s in range(K):
        p1 = sr.replay(oracle32, N, P, prompts[s], out[:, s])
        for i in range(Cn):
            p = sr.tempered(p1[i], tau)
            if sr.ambiguous(p, top_k, top_p):
                skipped += 1
                continue
            keep, mask, q = sr.filter64(p1[i], p, top_k, top_p)
            x = int(out[i, s])
            assert mask[x], (s, i, x, keep)
            assert int(kept[i, s]) == keep, (s, i, int(kept[i, s]), keep)
            keeps.append(keep)
            lo = q[:x].sum()
            hi = lo + q[x]
            checked += 1
            inside += lo <= u[i, s] < hi
            near += lo - 1e-5 <= u[i, s] < hi + 1e-5
    print(f"top_k {top_k} top_p {top_p} tau {tau}: skipped {skipped}, checked {checked}, inside {inside}, near {near}, "
          f"mean kept {np.mean(keeps):.2f}")
    assert skipped <= 0.05 * K * Cn, skipped
    assert inside >= 0.99 * checked and near == checked, (inside, near, checked)


def test_one_state_many_draws_stay_in_the_top_three():
    import lstm_hip
    N, K = 64, 512
    P = sr.peaked_params(N, seed=21)
    h1, c1 = _state(1, N, seed=22)
    h0, c0 = np.repeat(h1, K, axis=0), np.repeat(c1, K, axis=0)
    u = np.random.RandomState(23).random_sample((1, K))
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(P)
    out, _, _, _, info = L.generate(count=1, u=u, h0=h0, c0=c0, top_k=3, info=True)
    free, _, _, _ = L.generate(count=1, u=u, h0=h0, c0=c0)
    L.close()
    sp = split_params(np.asarray(P, np.float64), N)
    z = sp["Why"] @ h1[0].astype(np.float64) + sp["by"][:, 0]
    order = np.argsort(-z)
    assert z[order[2]] - z[order[3]] > 1e-6 * np.abs(z).max()  # the third and the fourth are apart (a property of the seed)
    got = set(int(x) for x in out[0])
    assert got <= set(int(x) for x in order[:3]), (got, order[:3])
    assert len(got) > 1
    assert (info["kept"] == 3).all()
    assert len(set(int(x) for x in free[0])) > 3  # unfiltered, the same draws reach further


@pytest.mark.parametrize("K", [1024, 4096])
def test_filtered_wide_batches_match_small_batches(K):
    """gen_head puts 4 (1024 streams) and 16 (4096) streams into one workgroup: with the filters on, every stream must come
    out as it does in a batch of 8 (one stream per workgroup) -- bytes, kept counts, final states, lengths."""
    import lstm_hip
    N, Cn = 64, 24
    rs = np.random.RandomState(K)
    P = sr.peaked_params(N, seed=31)
    lengths = rs.randint(0, 12, size=K)
    lengths[::7] = 0
    prompts = _prompts(lengths, seed=K + 1)
    h0, c0 = _state(K, N, seed=K + 2)
    u = rs.random_sample((Cn, K))
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(P)
    wide = L.generate(prompts, count=Cn, u=u, h0=h0, c0=c0, stop_byte=None, info=True, **FILTERS)
    assert 1 < wide[4]["kept"].mean() < 41 and len(np.unique(wide[4]["kept"])) > 5
    if K == 1024:
        groups = [np.arange(g, g + 8) for g in range(0, K, 8)]  # all of them
    else:  # the first and the last two workgroups' streams in every position, and a few more
        pick = np.unique(np.concatenate([np.arange(32), np.arange(K - 32, K), rs.choice(K, 16, replace=False)]))
        groups = [pick[g:g + 8] for g in range(0, pick.size, 8)]
    for g in groups:
        small = L.generate([prompts[i] for i in g], count=Cn, u=u[:, g], h0=h0[g], c0=c0[g], info=True, **FILTERS)
        assert np.array_equal(wide[0][:, g], small[0]), g
        assert np.array_equal(wide[2][g], small[2]) and np.array_equal(wide[3][g], small[3]), g
        assert np.array_equal(wide[4]["kept"][:, g], small[4]["kept"]), g
        assert np.array_equal(wide[4]["out_len"][g], small[4]["out_len"]), g
    L.close()


def _check_truncation(full, cut, stop, Cn):
    """`cut` (with stop byte `stop`) is `full` (without, same draws) truncated after each stream's first stop byte"""
    out, info = cut[0], cut[4]
    for s in range(out.shape[1]):
        where = np.nonzero(full[0][:, s] == stop)[0]
        n = int(where[0]) + 1 if where.size else Cn
        assert info["out_len"][s] == n, (s, info["out_len"][s], n)
        assert np.array_equal(out[:n, s], full[0][:n, s]), s
        assert not out[n:, s].any() and not info["kept"][n:, s].any(), s
        assert np.array_equal(info["kept"][:n, s], full[4]["kept"][:n, s]), s


def test_stop_byte_is_truncation():
    import lstm_hip
    N, K, Cn = 64, 24, 160
    P = sr.peaked_params(N, seed=41)
    lengths = [0, 1, 5, 30] * (K // 4)
    prompts = _prompts(lengths, seed=42)
    h0, c0 = _state(K, N, seed=43)
    u = np.random.RandomState(44).random_sample((Cn, K))
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(P)
    for kw in (dict(), dict(FILTERS)):
        run = lambda **extra: L.generate(prompts, count=Cn, u=u, h0=h0, c0=c0, score=True, info=True, **kw, **extra)
        full = run()
        stop = int(np.bincount(full[0][:Cn // 2].ravel(), minlength=256).argmax())  # a byte many streams draw early
        cut = run(stop_byte=stop)
        _check_truncation(full, cut, stop, Cn)
        assert np.array_equal(cut[1], full[1])  # the prompts' bits
        lens = cut[4]["out_len"]
        assert len(np.unique(lens[lens < Cn])) >= 4, lens  # (a property of the seeds)
        # the final state is the one after the stop byte: an unstopped run of exactly that many draws
        done = set()
        for s in np.argsort(lens):
            n = int(lens[s])
            if n in done or n == Cn or len(done) >= 5:
                continue
            done.add(n)
            short = L.generate(prompts, count=n, u=u[:n], h0=h0, c0=c0, **kw)
            assert np.array_equal(short[0][:, s], cut[0][:n, s]), s
            assert np.array_equal(short[2][s], cut[2][s]) and np.array_equal(short[3][s], cut[3][s]), (s, n)
        assert len(done) >= 4
        never = lens == Cn
        assert np.array_equal(cut[2][never], full[2][never]) and np.array_equal(cut[3][never], full[3][never])
        # a stop byte that never comes, also when the prompts hold it
        absent = [b for b in range(256) if not (full[0] == b).any()]
        assert absent
        same = run(stop_byte=absent[0])
        assert _same(same, full) and (same[4]["out_len"] == Cn).all() and np.array_equal(same[4]["kept"], full[4]["kept"])
        with_it = [np.concatenate([p, np.array([absent[0]] * 3, np.uint8)]) for p in prompts]
        a = L.generate(with_it, count=Cn, u=u, h0=h0, c0=c0, info=True, **kw)
        b = L.generate(with_it, count=Cn, u=u, h0=h0, c0=c0, info=True, stop_byte=absent[0], **kw)
        if not (a[0] == absent[0]).any():
            assert _same(a, b) and (b[4]["out_len"] == Cn).all()
        else:
            _check_truncation(a, b, absent[0], Cn)
    # greedy decoding with a stop byte
    full = L.generate(prompts, count=Cn, temperature=0.0, h0=h0, c0=c0, info=True)
    stop = int(full[0][7, 3])
    cut = L.generate(prompts, count=Cn, temperature=0.0, h0=h0, c0=c0, stop_byte=stop, info=True)
    _check_truncation(full, cut, stop, Cn)
    assert cut[4]["out_len"][3] <= 8 and (cut[4]["kept"][:1] == 1).all()
    n = int(cut[4]["out_len"][3])
    short = L.generate(prompts, count=n, temperature=0.0, h0=h0, c0=c0)
    assert np.array_equal(short[2][3], cut[2][3]) and np.array_equal(short[3][3], cut[3][3])
    L.close()


def test_bf16_padded_and_step_kernel_handles_match_their_twins():
    import lstm_hip
    K, Cn = 5, 80
    u = np.random.RandomState(51).random_sample((Cn, K))
    prompts = _prompts([0, 4, 60, 1, 200], seed=52)
    kw = dict(count=Cn, u=u, score=True, info=True, stop_byte=101, **FILTERS)

    def agree(ra, rb):
        assert _same(ra, rb)
        assert np.array_equal(ra[4]["out_len"], rb[4]["out_len"]) and np.array_equal(ra[4]["kept"], rb[4]["kept"])

    for twin in (lstm_hip.BF16_RECURRENCE, lstm_hip.STEP_KERNELS):  # the generator runs on the fp32 master weights
        N = 256 if twin == lstm_hip.BF16_RECURRENCE else 64
        P = sr.peaked_params(N, seed=53, scale=0.1)
        h0, c0 = _state(K, N, seed=54)
        res = []
        for flags in (0, twin):
            L = lstm_hip.Lstm(N, 2, 8, flags=flags)
            L.set_params(P)
            res.append(L.generate(prompts, h0=h0, c0=c0, **kw))
            L.close()
        agree(*res)
        assert 1 < res[0][4]["kept"][res[0][4]["kept"] > 0].mean() < 41
    # N = 500 padded to 512 against an explicit 512 handle with zero-padded parameters and state
    N, Np = 500, 512
    P = sr.peaked_params(N, seed=55, scale=0.1)
    h0, c0 = _state(K, N, seed=56)
    A = lstm_hip.Lstm(N, 2, 1, flags=lstm_hip.PAD_HIDDEN)
    A.set_params(P)
    ra = A.generate(prompts, h0=h0, c0=c0, **kw)
    A.close()
    Bh = lstm_hip.Lstm(Np, 2, 1)
    Bh.set_params(pad_params(P, N, Np))
    rb = Bh.generate(prompts, h0=pad_cols(h0, N, Np), c0=pad_cols(c0, N, Np), **kw)
    Bh.close()
    assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1])
    assert np.array_equal(ra[2], rb[2][:, :N]) and np.array_equal(ra[3], rb[3][:, :N])
    assert not rb[2][:, N:].any() and not rb[3][:, N:].any()
    assert np.array_equal(ra[4]["out_len"], rb[4]["out_len"]) and np.array_equal(ra[4]["kept"], rb[4]["kept"])


def _trainer(text, N, S, B):
    import lstm_hip
    L = lstm_hip.Lstm(N, S, B)
    L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(5), N))
    L.set_text(text)
    L.set_cursors(lstm_hip.initial_cursors(text.size, S, B))
    return L


def test_training_state_is_untouched_by_filtered_generation():
    import lstm_hip
    N, S, B = 64, 8, 4
    text = np.random.RandomState(61).randint(97, 123, size=5000).astype(np.uint8)
    A, Bh = _trainer(text, N, S, B), _trainer(text, N, S, B)
    la = [A.train_windows(5, 0.1)]
    A.generate(_prompts([3, 40], seed=62), count=50, u=np.random.RandomState(63).random_sample((50, 2)), score=True,
               stop_byte=104, info=True, **FILTERS)
    la.append(A.train_windows(5, 0.1))
    lb = [Bh.train_windows(5, 0.1), Bh.train_windows(5, 0.1)]
    assert np.array_equal(np.concatenate(la), np.concatenate(lb))
    for which in (lstm_hip.P_PARAMS, lstm_hip.P_GRADS, lstm_hip.P_MEM):
        assert np.array_equal(A.get_params(which), Bh.get_params(which)), which
    assert np.array_equal(A.get_cursors(), Bh.get_cursors())
    for a, b in zip(A.get_window(), Bh.get_window()):
        assert np.array_equal(a, b)
    for t in range(S):
        for a, b in zip(A.get_state(t), Bh.get_state(t)):
            assert np.array_equal(a, b), t
    A.close()
    Bh.close()


def test_refused_options_leave_a_usable_handle():
    import lstm_hip
    N, S, B = 32, 6, 2
    text = np.random.RandomState(71).randint(97, 123, size=2000).astype(np.uint8)
    L = _trainer(text, N, S, B)
    lib = L.lib
    u = np.random.RandomState(72).random_sample(64)
    out = np.zeros(64, np.uint8)
    dp = u.ctypes.data_as(C.POINTER(C.c_double))
    op = out.ctypes.data_as(C.POINTER(C.c_uint8))
    size = C.sizeof(lstm_hip._Sampling)
    good = (size, 1.0, 0, 1.0, -1)
    cases = [
        None,                                  # no options
        (size - 4, 1.0, 0, 1.0, -1),           # a wrong size
        (size + 8, 1.0, 0, 1.0, -1),
        (0, 1.0, 0, 1.0, -1),
        (size, 1.0, -1, 1.0, -1),              # top_k outside 0..256
        (size, 1.0, 257, 1.0, -1),
        (size, 1.0, 0, float("nan"), -1),      # top_p NaN, <= 0, > 1
        (size, 1.0, 0, 0.0, -1),
        (size, 1.0, 0, -0.5, -1),
        (size, 1.0, 0, 1.0000001, -1),
        (size, 1.0, 0, float("inf"), -1),
        (size, 1.0, 0, 1.0, -2),               # stop_byte outside -1..255
        (size, 1.0, 0, 1.0, 256),
        (size, -0.5, 40, 0.9, 10),             # and what lstm_hip_generate refuses, still refused
        (size, float("nan"), 40, 0.9, 10),
    ]
    for case in cases:
        opt = C.byref(lstm_hip._Sampling(*case)) if case else None
        rc = lib.lstm_hip_generate_ex(L._h, 1, None, None, None, None, opt, dp, 4, op, None, None, None, None, None)
        assert rc == lstm_hip.EINVAL, (case, rc)
        assert lib.lstm_hip_last_error().decode().startswith("generate:")
    rc = lib.lstm_hip_generate_ex(L._h, 1, None, None, None, None, C.byref(lstm_hip._Sampling(*good)), None, 4, op, None, None,
                                  None, None, None)
    assert rc == lstm_hip.EINVAL  # no draws with temperature > 0
    with pytest.raises(lstm_hip.LstmHipError):
        L.generate(count=4, u=u[:4].reshape(4, 1), top_k=300)
    losses = L.train_windows(3, 0.1)
    assert np.isfinite(losses).all()
    got = L.generate(count=10, u=u[:10].reshape(10, 1), top_k=5, top_p=0.5, stop_byte=0, info=True)  # and still generates
    assert got[0].shape == (10, 1) and 1 <= got[4]["kept"][0, 0] <= 5
    L.close()


LSTM = os.path.join(ROOT, "eigen-lstm_amd", "lstm")
GEN = os.path.join(ROOT, "eigen-lstm_amd", "lstm_generate")


def test_program_top_k_one_is_greedy_and_stop_byte_ends_samples(tmp_path):
    rs = np.random.RandomState(81)
    # lines of 3..12 letters: a model trained on them draws newlines
    text = b"".join(bytes(rs.randint(97, 110, size=rs.randint(3, 13)).astype(np.uint8)) + b"\n" for _ in range(500))
    corpus = tmp_path / "corpus.txt"
    corpus.write_bytes(text)
    tr = subprocess.run([LSTM, str(corpus), "64", "8", "4", "0.1", "--epochs", "1", "--windows", "200", "--sample", "0",
                         "--save", str(tmp_path / "ck"), "--quiet"], capture_output=True, text=True, errors="replace", timeout=300)
    assert tr.returncode == 0, tr.stderr
    run = lambda *extra: subprocess.run([GEN, "--load", str(tmp_path / "ck"), "--count", "200", "--streams", "4", "--prime", "ab",
                                         *extra], capture_output=True, timeout=300)
    greedy, one = run("--temperature", "0"), run("--top-k", "1", "--seed", "5")
    assert greedy.returncode == 0 and one.returncode == 0, (greedy.stderr, one.stderr)
    assert greedy.stdout == one.stdout and greedy.stdout.count(b"== sample ") == 4
    full, cut = run("--seed", "3"), run("--seed", "3", "--stop-byte", "10")
    assert full.returncode == 0 and cut.returncode == 0, (full.stderr, cut.stderr)

    def samples(blob):
        parts = blob.split(b"== sample ")[1:]
        return [p.split(b" ==\n", 1)[1][:-1] for p in parts]  # (the program ends every sample with a newline of its own)

    sf, sc = samples(full.stdout), samples(cut.stdout)
    assert len(sf) == len(sc) == 4
    ended = 0
    for a, b in zip(sf, sc):
        assert a.startswith(b"ab") and len(a) == 202
        drawn = a[2:]
        n = drawn.index(b"\n") + 1 if b"\n" in drawn else 200
        assert b == a[:2 + n], (a, b)
        ended += n < 200
    assert ended >= 1  # (a property of the corpus: the model draws newlines)
    filt = run("--seed", "3", "--top-k", "3", "--top-p", "0.8")
    assert filt.returncode == 0 and filt.stdout != full.stdout
