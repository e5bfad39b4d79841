"""-m gpu: lstm_hip_generate -- batched, prompted sampling and per-text scoring (include/lstm_hip.h).

A stream of a batched call must be exactly what lstm_hip_sample makes of it alone (bit for bit: every logit is summed in
the same order, and the recurrence's columns do not interact); against the oracle the usual sampler agreement (>= 99 % of
draws: a draw within rounding of a CDF edge may go either way) and evaluator tolerances hold."""
import os
import re
import subprocess

import numpy as np
import pytest

import gpu_util as gu
from test_pad_hidden import pad_cols, pad_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 256


def _params(N, seed, scale=0.3):
    return gu.random_case(N, 2, 1, seed=seed, scale=scale)[0]


def _state(streams, N, seed):
    rs = np.random.RandomState(seed)
    return (rs.randn(streams, N) * 0.1).astype(np.float32), (rs.randn(streams, N) * 0.1).astype(np.float32)


def _prompts(lengths, seed):
    rs = np.random.RandomState(seed)
    return [rs.randint(32, 127, size=n).astype(np.uint8) for n in lengths]


def _oracle_after_prompt(orc, N, P, prompt):
    """the oracle's state after feeding `prompt` from zero"""
    L = len(prompt)
    if L == 0:
        return np.zeros(N, np.float32), np.zeros(N, np.float32)
    xi = np.full((L + 1, 1), -1, np.int32)
    ti = np.full((L + 1, 1), -1, np.int32)
    xi[1:, 0] = prompt
    ti[1:L, 0] = prompt[1:]
    fw = orc.forward(N, M, L + 1, 1, P, xi, ti, np.zeros((1, N), np.float32), np.zeros((1, N), np.float32))
    return fw["h"][L][0].copy(), fw["c"][L][0].copy()


@pytest.mark.parametrize("N", [128, 512])
def test_batch_equals_single_stream_bit_for_bit(N):
    import lstm_hip
    K, C = 37, 300
    P = _params(N, seed=3)
    h0, c0 = _state(K, N, seed=4)
    u = np.random.RandomState(5).random_sample((C, K))
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(P)
    out, bits, h, c = L.generate(count=C, u=u, h0=h0, c0=c0)
    assert bits is None and out.shape == (C, K) and h.shape == (K, N)
    for s in range(K):
        o1, h1, c1 = L.sample(h0[s], c0[s], u[:, s])
        assert np.array_equal(out[:, s], o1), s
        assert np.array_equal(h[s], h1) and np.array_equal(c[s], c1), s
    L.close()


# persistent; LSTM_HIP_STEP_KERNELS; padded 500 -> 512; widths the plan puts on the per-step engine (12 and 65 k-steps)
@pytest.mark.parametrize("N,flags", [(128, 0), (64, 4), (500, 256), (192, 0), (1040, 0)])
def test_streams_agree_with_the_oracle_sampler(N, flags, oracle32):
    import lstm_hip
    K, C = 6, 200
    # (at 0.3 a 500-unit recurrence is chaotic: fp32 and fp64 oracles part; so does a 1040-unit one at 0.1)
    P = _params(N, seed=7, scale=0.3 if N <= 128 else 0.1 if N <= 512 else 0.05)
    h0, c0 = _state(K, N, seed=8)
    u = np.random.RandomState(9).random_sample((C, K))
    L = lstm_hip.Lstm(N, 2, 1, flags=flags)
    L.set_params(P)
    out, _, h, c = L.generate(count=C, u=u, h0=h0, c0=c0)
    L.close()
    for s in range(K):
        want, hw, cw = oracle32.sample(N, M, P, h0[s], c0[s], u[:, s])
        assert (out[:, s] == want).mean() >= 0.99, (s, (out[:, s] == want).mean())
        if (out[:, s] == want).all():
            assert gu.max_rel(h[s], hw) <= 1e-3 and gu.max_rel(c[s], cw) <= 1e-3


def test_streams_are_independent_and_permute():
    import lstm_hip
    N, K, C = 128, 6, 120
    P = _params(N, seed=11)
    prompts = _prompts([3, 0, 17, 40, 1, 9], seed=12)
    h0, c0 = _state(K, N, seed=13)
    u = np.random.RandomState(14).random_sample((C, K))
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(P)
    ref = L.generate(prompts, count=C, u=u, h0=h0, c0=c0, score=True)
    # everything but stream 2 changed
    p2 = _prompts([7, 50, 0, 2, 33, 4], seed=15)
    p2[2] = prompts[2]
    h2, c2 = _state(K, N, seed=16)
    h2[2], c2[2] = h0[2], c0[2]
    u2 = np.random.RandomState(17).random_sample((C, K))
    u2[:, 2] = u[:, 2]
    got = L.generate(p2, count=C, u=u2, h0=h2, c0=c2, score=True)
    assert np.array_equal(got[0][:, 2], ref[0][:, 2]) and got[1][2] == ref[1][2]
    assert np.array_equal(got[2][2], ref[2][2]) and np.array_equal(got[3][2], ref[3][2])
    # a permutation of the streams permutes the results
    perm = np.array([4, 2, 0, 5, 1, 3])
    got = L.generate([prompts[i] for i in perm], count=C, u=u[:, perm], h0=h0[perm], c0=c0[perm], score=True)
    L.close()
    assert np.array_equal(got[0], ref[0][:, perm]) and np.array_equal(got[1], ref[1][perm])
    assert np.array_equal(got[2], ref[2][perm]) and np.array_equal(got[3], ref[3][perm])


def test_ragged_prompts_score_state_and_continuation(oracle32):
    import lstm_hip
    N, C = 128, 100
    lengths = [0, 1, 2, 5, 129, 130, 1000, 3001]
    K = len(lengths)
    P = _params(N, seed=21, scale=0.15)
    prompts = _prompts(lengths, seed=22)
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(P)
    _, bits, h, c = L.generate(prompts, count=0, score=True)
    u = np.random.RandomState(23).random_sample((C, K))
    out, bits2, _, _ = L.generate(prompts, count=C, u=u, score=True)
    L.close()
    assert np.array_equal(bits, bits2)  # the draws after the prompt do not touch its score
    for s, (n, p) in enumerate(zip(lengths, prompts)):
        if n >= 2:
            want = oracle32.eval_bits(N, M, P, p) * (n - 1)
            assert abs(bits[s] - want) <= 2e-5 * (n - 1), (n, bits[s], want)
        else:
            assert bits[s] == 0.0
        hw, cw = _oracle_after_prompt(oracle32, N, P, p)
        assert gu.max_rel(h[s], hw) <= 1e-3 if n else np.array_equal(h[s], hw), n
        want, _, _ = oracle32.sample(N, M, P, hw, cw, u[:, s])
        assert (out[:, s] == want).mean() >= 0.99, (n, (out[:, s] == want).mean())


def test_known_answer_fixture_as_one_stream_of_four():
    import lstm_hip
    fx = np.load(os.path.join(ROOT, "tests", "golden", "fixture_A.npz"))
    N, text = int(fx["N"]), fx["text"]
    others = _prompts([500, 0, 1500], seed=31)
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(fx["params"])
    _, bits, _, _ = L.generate([others[0], others[1], text, others[2]], score=True)
    L.close()
    got = bits[2] / (text.size - 1)
    assert abs(got - float(fx["expected_bits"])) <= 1e-4, got


def _tempered(p, tau):
    q = np.asarray(p, np.float64) ** (1.0 / tau)
    return q / q.sum()


@pytest.mark.parametrize("tau", [0.5, 2.0, 0.0])
def test_temperature_and_greedy_against_the_oracle(tau, oracle32):
    import lstm_hip
    N, K, C = 64, 4, 150
    P = _params(N, seed=41, scale=0.2)
    prompts = _prompts([1] * K, seed=42)
    u = np.random.RandomState(43).random_sample((C, K))
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(P)
    out, _, _, _ = L.generate(prompts, count=C, u=u, temperature=tau)
    if tau == 0.0:  # greedy decoding takes no draws
        out2, _, _, _ = L.generate(prompts, count=C, u=None, temperature=0.0)
        out3, _, _, _ = L.generate(prompts, count=C, u=u[::-1].copy(), temperature=0.0)
        assert np.array_equal(out, out2) and np.array_equal(out, out3)
        for tiny in (1e-39, 1e-60):  # below the smallest normal float (denormal, or 0 in float): the greedy limit
            out4, _, _, _ = L.generate(prompts, count=C, u=u, temperature=tiny)
            assert np.array_equal(out, out4), tiny
    L.close()
    inside, near, checked = 0, 0, 0
    for s in range(K):
        # feed the stream's inputs back through the oracle: probs[t] is the distribution byte t - 1 was drawn from
        xi = np.full((C + 1, 1), -1, np.int32)
        xi[1, 0] = prompts[s][0]
        xi[2:, 0] = out[:-1, s]
        fw = oracle32.forward(N, M, C + 1, 1, P, xi, np.full((C + 1, 1), -1, np.int32), np.zeros((1, N), np.float32),
                              np.zeros((1, N), np.float32))
        for i in range(C):
            p = np.asarray(fw["probs"][i + 1][0], np.float64)
            x = int(out[i, s])
            if tau == 0.0:
                top = np.sort(p)[::-1]
                if (top[0] - top[1]) > 1e-6 * top[0]:
                    assert x == int(np.argmax(p)), (s, i)
                continue
            q = _tempered(p, tau)
            lo = q[:x].sum()
            hi = lo + q[x]
            checked += 1
            inside += lo <= u[i, s] < hi
            near += lo - 1e-5 <= u[i, s] < hi + 1e-5
    if tau != 0.0:
        assert inside >= 0.99 * checked and near == checked, (inside, near, checked)


@pytest.mark.parametrize("K", [512, 1024, 2048, 4096])
def test_wide_batches_match_a_small_batch(K):
    """From 512 streams up gen_head puts 2, 4, 8 and then 16 streams into one workgroup (kernels.hip, gen_head_group): every
    stream of those, in whatever position, must come out bit-identical -- bytes, prompt bits, final h and c -- to the same
    stream run in a small batch (one stream per workgroup), with ragged prompts, scoring and tempered or greedy draws."""
    import lstm_hip
    N, C = 64, 24
    rs = np.random.RandomState(K)
    P = _params(N, seed=91)
    lengths = rs.randint(0, 20, size=K)
    lengths[::7] = 0
    prompts = _prompts(lengths, seed=K + 1)
    h0, c0 = _state(K, N, seed=K + 2)
    u = rs.random_sample((C, K))
    # the first and the last two workgroups' streams in every position (at most 16 per group), and a few more
    pick = np.unique(np.concatenate([np.arange(32), np.arange(K - 32, K), rs.choice(K, 8, replace=False)]))
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(P)
    for tau in (1.0, 0.5, 0.0):
        wide = L.generate(prompts, count=C, u=u, temperature=tau, h0=h0, c0=c0, score=True)
        small = L.generate([prompts[i] for i in pick], count=C, u=u[:, pick], temperature=tau, h0=h0[pick], c0=c0[pick],
                           score=True)
        assert np.array_equal(wide[0][:, pick], small[0]), tau
        assert np.array_equal(wide[1][pick], small[1]), tau
        assert np.array_equal(wide[2][pick], small[2]) and np.array_equal(wide[3][pick], small[3]), tau
        assert wide[1][lengths >= 2].min() > 0.0 and not wide[1][lengths < 2].any()
    L.close()


def test_bf16_and_padded_handles_match_their_fp32_twins():
    import lstm_hip
    K, C = 5, 80
    u = np.random.RandomState(51).random_sample((C, K))
    prompts = _prompts([0, 4, 60, 1, 200], seed=52)
    # bf16 handle: the generator runs on the fp32 master weights
    N = 256
    P = _params(N, seed=53, scale=0.1)
    h0, c0 = _state(K, N, seed=54)
    res = []
    for flags, B in ((0, 8), (lstm_hip.BF16_RECURRENCE, 8)):
        L = lstm_hip.Lstm(N, 2, B, flags=flags)
        L.set_params(P)
        res.append(L.generate(prompts, count=C, u=u, h0=h0, c0=c0, score=True))
        L.close()
    for a, b in zip(*res):
        assert np.array_equal(a, b)
    # N = 500 padded to 512 against an explicit 512 handle with zero-padded parameters and state
    N, Np = 500, 512
    P = _params(N, seed=55, scale=0.1)
    h0, c0 = _state(K, N, seed=56)
    A = lstm_hip.Lstm(N, 2, 1, flags=lstm_hip.PAD_HIDDEN)
    A.set_params(P)
    ra = A.generate(prompts, count=C, u=u, h0=h0, c0=c0, score=True)
    A.close()
    Bh = lstm_hip.Lstm(Np, 2, 1)
    Bh.set_params(pad_params(P, N, Np))
    rb = Bh.generate(prompts, count=C, u=u, h0=pad_cols(h0, N, Np), c0=pad_cols(c0, N, Np), score=True)
    Bh.close()
    assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1])
    assert np.array_equal(ra[2], rb[2][:, :N]) and np.array_equal(ra[3], rb[3][:, :N])
    assert not rb[2][:, N:].any() and not rb[3][:, N:].any()


def _trainer(text, N, S, B):
    import lstm_hip
    L = lstm_hip.Lstm(N, S, B)
    L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(5), N))
    L.set_text(text)
    L.set_cursors(lstm_hip.initial_cursors(text.size, S, B))
    return L


def test_training_state_is_untouched():
    import lstm_hip
    N, S, B = 64, 8, 4
    text = np.random.RandomState(61).randint(97, 123, size=5000).astype(np.uint8)
    A, Bh = _trainer(text, N, S, B), _trainer(text, N, S, B)
    la = [A.train_windows(5, 0.1)]
    A.generate(_prompts([3, 40], seed=62), count=50, u=np.random.RandomState(63).random_sample((50, 2)), score=True)
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


def test_refused_arguments_leave_a_usable_handle():
    import ctypes as C
    import lstm_hip
    N, S, B = 32, 6, 2
    text = np.random.RandomState(71).randint(97, 123, size=2000).astype(np.uint8)
    L = _trainer(text, N, S, B)
    lib = L.lib
    u = np.random.RandomState(72).random_sample(64)
    out = np.zeros(64, np.uint8)
    p = np.frombuffer(b"abcdef", np.uint8).copy()
    up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    dp = u.ctypes.data_as(C.POINTER(C.c_double))
    op = out.ctypes.data_as(C.POINTER(C.c_uint8))
    pp = p.ctypes.data_as(C.POINTER(C.c_uint8))
    bad_start = np.array([1, 3], np.uint64)
    decreasing = np.array([0, 4, 2, 6], np.uint64)
    cases = [
        (0, None, None, 1.0, dp, 4, op),                          # streams < 1
        (4097, None, None, 1.0, dp, 0, op),                       # streams > 4096
        (1, None, None, 1.0, dp, -1, op),                         # count < 0
        (1, pp, up(bad_start), 1.0, dp, 4, op),                   # offsets not starting at 0
        (3, pp, up(decreasing), 1.0, dp, 4, op),                  # decreasing offsets
        (1, None, None, -0.5, dp, 4, op),                         # negative temperature
        (1, None, None, float("inf"), dp, 4, op),                 # temperature not finite
        (1, None, None, float("nan"), dp, 4, op),
        (1, None, None, 0.7, None, 4, op),                        # no draws with temperature > 0
        (1, None, None, 1.0, dp, 4, None),                        # no out with count > 0
    ]
    for streams, prompts, off, tau, uu, count, o in cases:
        rc = lib.lstm_hip_generate(L._h, streams, prompts, off, None, None, C.c_double(tau), uu, count, o, None, None, None)
        assert rc == lstm_hip.EINVAL, (streams, tau, count, rc)
        assert lib.lstm_hip_last_error().decode().startswith("generate:")
    losses = L.train_windows(3, 0.1)
    assert np.isfinite(losses).all()
    out, _, _, _ = L.generate(count=10, u=u[:10].reshape(10, 1))  # and still generates
    assert out.shape == (10, 1)
    L.close()


LSTM = os.path.join(ROOT, "eigen-lstm_amd", "lstm")
GEN = os.path.join(ROOT, "eigen-lstm_amd", "lstm_generate")


def test_program_scores_and_generates_from_a_checkpoint(tmp_path):
    import lstm_hip
    rs = np.random.RandomState(81)
    text = rs.randint(97, 110, size=3000).astype(np.uint8)
    corpus = tmp_path / "corpus.txt"
    text.tofile(corpus)
    N = 64
    tr = subprocess.run([LSTM, str(corpus), str(N), "8", "4", "0.1", "--epochs", "1", "--windows", "30", "--sample", "0",
                         "--save", str(tmp_path / "ck"), "--quiet"], capture_output=True, text=True, errors="replace", timeout=300)
    assert tr.returncode == 0, tr.stderr
    files = []
    for i, n in enumerate((400, 2, 1500)):
        f = tmp_path / f"t{i}.txt"
        rs.randint(97, 115, size=n).astype(np.uint8).tofile(f)
        files.append(f)
    out = subprocess.run([GEN, "--load", str(tmp_path / "ck"), "--score"] + [str(f) for f in files], capture_output=True,
                         text=True, errors="replace", timeout=300)
    assert out.returncode == 0, out.stderr
    P = np.concatenate([np.loadtxt(tmp_path / f"ck_{k}.txt", ndmin=2).astype(np.float32).flatten(order="F")
                        for k in ("W", "U", "b", "Why", "by")])
    L = lstm_hip.Lstm(N, 2, 1, flags=lstm_hip.PAD_HIDDEN)
    L.set_params(P)
    total_bits = total_n = 0.0
    for f in files:
        m = re.search(re.escape(str(f)) + r": ([\d.]+) bits/char \((\d+) bytes\)", out.stdout)
        assert m, out.stdout
        data = np.fromfile(f, np.uint8)
        assert int(m.group(2)) == data.size
        want = L.eval_bits(data)
        assert abs(float(m.group(1)) - want) <= 1e-5, (f, m.group(1), want)
        total_bits += want * (data.size - 1)
        total_n += data.size - 1
    L.close()
    m = re.search(r"total: ([\d.]+) bits/char", out.stdout)
    assert m and abs(float(m.group(1)) - total_bits / total_n) <= 1e-5
    run = lambda *extra: subprocess.run([GEN, "--load", str(tmp_path / "ck"), "--count", "200", "--streams", "4", "--prime", "The ",
                                         *extra], capture_output=True, timeout=300)
    a, b = run("--seed", "3"), run("--seed", "3")
    assert a.returncode == 0 and a.stdout == b.stdout
    assert a.stdout.count(b"== sample ") == 4 and a.stdout.count(b"The ") >= 4
    g1, g2 = run("--temperature", "0", "--seed", "1"), run("--temperature", "0", "--seed", "99")
    assert g1.returncode == 0 and g1.stdout == g2.stdout
