"""-m gpu: lstm_hip_encode_mixed / lstm_hip_decode_mixed -- the static coder on a log-linear mix of several models, the mixing
weights fixed or learned per stream (include/lstm_hip.h).

With the block NULL the calls are lstm_hip_encode / lstm_hip_decode byte for byte; weights (1, 0) and (0, 1) at rate 0 give the
main handle's and the guide handle's own codes; every combination round-trips with the decoder's final weights equal to the
encoder's; whole tables, read with the 256 probe streams of tests/test_code_tables.py, lie inside code_table_ref's interval of
the float32 mix (tests/mix_coder_ref.py) of every model's logits under the device's own w_trace row, and each probe stream's
final weights are, bit for bit, the reference update from that row, the device's own whole table, the float32 logits and the
probe's byte; rate-0 bits agree with the guided scorer within the quantisation's own bound; and learned weights beat fixed ones
where the guide is the better model.

The bound of the bits against the scorer, from the rule of section 3.6: q = 1 + floor(v), v = 65024 p (1 +- delta) with
delta = code_table_ref.DELTA, and sum_m v_m < T <= 65281.  So q / T >= 65024 p (1 - delta) / 65281, which is at most
log2(65281 / 65024) + delta / ln 2 < 0.00575 bits above -log2 p, and q / T <= (1 + 65024 p (1 + delta)) / (65024 (1 - delta)),
which is at most log2(1 + 1 / (65024 p)) + 2 delta / ln 2 bits below it.  The scorer's own float32 surprisal is within
score_ref.BOUND = 1e-4 bits of -log2 p (tests/test_guided_score.py), which is added on both sides."""
import os

import numpy as np
import pytest

import code_table_ref as ct
import mix_coder_ref as mr
import sampling_ref as sr
import score_ref as sc
from logits_ref import logits32
from oracle_lib import split_params
from test_logit_processors import _group_rule

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 256
f32 = np.float32
N, GN, GP, K = 16, 32, 40, 20
PREFIXES = (0, 1, 2, 5, 9)
RATE = 0.01


@pytest.fixture(scope="module")
def models():
    """main (N = 16), a guide at 32, a padded guide at 40, the 32 guide's parameters under LSTM_HIP_FAST_MATH: (handle, P)"""
    import lstm_hip
    specs = ((N, 7, 0), (GN, 8, 0), (GP, 9, lstm_hip.PAD_HIDDEN), (GN, 8, lstm_hip.FAST_MATH))
    hs = []
    for n, seed, flags in specs:
        L = lstm_hip.Lstm(n, 2, 1, flags=flags)
        P = sr.peaked_params(n, seed=seed, gain=6.0)
        L.set_params(P)
        hs.append((L, P))
    yield hs
    for L, _ in hs:
        L.close()


def _texts(k=K, seed=3):
    rs = np.random.RandomState(seed)
    lengths = [(7 * s + 3) % 29 for s in range(k)]
    assert lengths[12] == 0 and lengths[8] == 1
    return [bytes(rs.randint(97, 123, size=n).astype(np.uint8)) for n in lengths]


def _sb2_count():
    group = _group_rule()
    k2 = next(k for k in range(1, 4097) if group(N, k) == 2)
    assert group(N, k2 - 1) == 1
    return k2


def test_a_null_block_is_the_unmixed_coder(models):
    L = models[0][0]
    texts = _texts()
    a, b = L.encode(texts, trace=True), L.encode_mixed(texts, guides=None, trace=True)
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    lengths = [len(t) for t in texts]
    assert L.decode_mixed(a[0], lengths, guides=None) == L.decode(a[0], lengths) == texts
    assert sum(len(c) for c in a[0]) > 0


@pytest.mark.parametrize("k", ["20", "sb2"])
def test_selecting_weights_give_each_handles_own_code(models, k):
    (L, _), (G, _) = models[0], models[1]
    texts = _texts(K if k == "20" else _sb2_count())
    own, guide = L.encode(texts, trace=True), G.encode(texts, trace=True)
    a = L.encode_mixed(texts, guides=[(G, 0.0)], main_weight=1.0, rate=0.0, trace=True)
    b = L.encode_mixed(texts, guides=[(G, 1.0)], main_weight=0.0, rate=0.0, trace=True)
    assert a[0] == own[0] and a[2].tobytes() == own[2].tobytes() and a[1].tobytes() == own[1].tobytes()
    assert b[0] == guide[0] and b[2].tobytes() == guide[2].tobytes() and b[1].tobytes() == guide[1].tobytes()
    assert own[0] != guide[0]


# (guides as indices into models, weights, rate)
ROUND_TRIPS = {
    "fixed_one_guide": ((1,), (0.6, 0.4), 0.0),
    "learned_one_guide": ((1,), (0.6, 0.4), RATE),
    "fixed_two_guides": ((1, 2), (0.7, 0.3, -0.2), 0.0),
    "learned_two_guides": ((1, 2), (0.7, 0.3, -0.2), RATE),
    "learned_fast_math_guide": ((3,), (0.5, 0.5), RATE),
    "learned_own_guide": ((0,), (0.75, 0.35), RATE),
    "learned_from_1_0": ((1,), (1.0, 0.0), 0.03),
}


# every combination at 20 streams; two of them again at the first stream count of the second group size
@pytest.mark.parametrize("name,k", [(n, "20") for n in sorted(ROUND_TRIPS)] + [("learned_two_guides", "sb2"), ("fixed_one_guide", "sb2")])
def test_round_trips(models, name, k):
    idx, w, rate = ROUND_TRIPS[name]
    L = models[0][0]
    guides = [(models[i][0], w[1 + j]) for j, i in enumerate(idx)]
    texts = _texts(K if k == "20" else _sb2_count())
    lengths = [len(t) for t in texts]
    codes, bits, w_out, w_trace = L.encode_mixed(texts, guides=guides, main_weight=w[0], rate=rate, weights=True)
    back, w_dec = L.decode_mixed(codes, lengths, guides=guides, main_weight=w[0], rate=rate, weights=True)
    assert back == texts
    assert w_dec.tobytes() == w_out.tobytes()
    v0 = np.array(w, f32)
    off = np.concatenate([[0], np.cumsum(lengths)])
    for s, n in enumerate(lengths):
        if n:
            assert w_trace[off[s]].tobytes() == v0.tobytes(), s  # byte 0 is coded under the call's weights
        else:
            assert w_out[s].tobytes() == v0.tobytes() and codes[s] == b""
    moved = sum(w_out[s].tobytes() != v0.tobytes() for s in range(len(texts)))
    assert moved == (sum(n > 0 for n in lengths) if rate > 0 else 0), (moved, name)
    if rate > 0:  # other weights or another rate do not decode it
        wrong = L.decode_mixed(codes, lengths, guides=guides, main_weight=w[0], rate=2 * rate)
        assert wrong != texts


def _state_of(L, n):
    def state_of(prefix):
        if not prefix:
            return np.zeros(n, f32)
        return np.asarray(L.generate([prefix], count=0)[2], f32).reshape(n)
    return state_of


def _why(P, n):
    sp = split_params(np.asarray(P, f32), n)
    return np.asarray(sp["Why"], f32), np.asarray(sp["by"], f32).reshape(M)


@pytest.mark.parametrize("k", ["300", "sb2"])
@pytest.mark.parametrize("rate", [0.0, RATE])
def test_whole_tables_and_the_update_from_them(models, rate, k):
    """the probes of tests/test_code_tables.py: prefix + bytes([b]) for b = 0..255 among fillers, at a position that is no
    multiple of the group size"""
    streams = 300 if k == "300" else _sb2_count()
    pos = 0 if k == "300" else 3
    members = [models[0], models[1], models[2]]
    L = members[0][0]
    guides = [(members[1][0], 0.3), (members[2][0], -0.2)]
    v0 = np.array((0.7, 0.3, -0.2), f32)
    text = bytes(np.random.RandomState(5).randint(97, 123, size=9).astype(np.uint8))
    whys = [_why(P, h.N) for h, P in members]
    states = [_state_of(h, h.N) for h, _ in members]
    rs = np.random.RandomState(11)
    moved = 0
    for n in PREFIXES:
        prefix = text[:n]
        texts = [bytes(rs.randint(97, 123, size=int(rs.randint(0, 13))).astype(np.uint8)) for _ in range(streams)]
        texts[pos:pos + M] = [prefix + bytes([b]) for b in range(M)]
        codes, bits, tr, w_out, w_trace = L.encode_mixed(texts, guides=guides, main_weight=0.7, rate=rate, trace=True, weights=True)
        off = np.concatenate([[0], np.cumsum([len(t) for t in texts])])
        at = off[pos:pos + M] + n
        rows = tr[at].astype(np.int64)
        wrow = w_trace[at]
        assert all(r.tobytes() == wrow[0].tobytes() for r in wrow), n  # the same prefix, the same weights
        assert w_trace[off[pos]].tobytes() == v0.tobytes()
        if n == 0 or rate == 0:
            assert wrow[0].tobytes() == v0.tobytes(), n
        else:
            moved += wrow[0].tobytes() != v0.tobytes()
        zs = [logits32(Why, by, st(prefix)) for (Why, by), st in zip(whys, states)]
        z = mr.mix32(zs, wrow[0])
        cum, q, T = rows[:, 0], rows[:, 1], rows[:, 2]
        assert (T == T[0]).all() and T[0] == q.sum(), (n, np.unique(T), int(q.sum()))
        assert np.array_equal(cum, np.concatenate([[0], np.cumsum(q)[:-1]])), n
        bad = ct.outside(q, z)
        lo, hi = ct.interval64(z)
        assert bad.size == 0, (n, [(int(m), int(q[m]) - 1, int(lo[m]), int(hi[m])) for m in bad[:8]])
        for b in range(M):  # the update: no tolerance
            want = mr.update32(wrow[0], q.astype(np.uint32), int(T[0]), zs, b, rate)
            assert w_out[pos + b].tobytes() == want.tobytes(), (n, b, w_out[pos + b], want)
    assert moved == (len(PREFIXES) - 1 if rate > 0 else 0)


def test_rate_zero_bits_agree_with_the_guided_scorer(models):
    (L, _), (G, _), (G2, _) = models[0], models[1], models[2]
    texts = _texts()
    guides = [(G, 0.3), (G2, -0.2)]
    codes, bits, tr = L.encode_mixed(texts, guides=guides, main_weight=0.7, rate=0.0, trace=True)
    got = L.score_guided(texts, guides=guides, main_weight=0.7, first=True)
    delta = ct.DELTA / np.log(2.0)
    off = np.concatenate([[0], np.cumsum([len(t) for t in texts])])
    checked = 0
    for s, t in enumerate(texts):
        sur = np.asarray(got["surprisal"][s], np.float64)
        assert sur.size == len(t)
        per = -np.log2(tr[off[s]:off[s + 1], 1].astype(np.float64) / tr[off[s]:off[s + 1], 2])
        assert abs(per.sum() - bits[s]) <= 1e-9 * max(1.0, bits[s])
        above = len(t) * (np.log2(65281.0 / 65024.0) + delta + sc.BOUND)
        below = float(np.sum(np.log2(1.0 + 2.0 ** sur / 65024.0))) + len(t) * (2 * delta + sc.BOUND)
        diff = bits[s] - float(sur.sum())
        print(f"stream {s}: {len(t)} bytes, coder {bits[s]:.6f} bits, scorer {sur.sum():.6f}, difference {diff:+.6f} in [-{below:.6f}, +{above:.6f}]")
        assert -below <= diff <= above, (s, diff, below, above)
        checked += len(t)
    assert checked == sum(len(t) for t in texts) > 200


def test_learned_weights_beat_the_fixed_mix_where_the_guide_is_the_better_model(models):
    """the text is drawn from the guide, so the guide is the better model of it; the margin the reference alone shows on the
    device's own states (every model's logits along the text by tests/logits_ref.py) is what the device must reach half of"""
    (L, P), (G, Pg) = models[0], models[1]
    n, rate = 240, 0.02
    u = np.random.RandomState(21).random_sample((n, 1))
    text = bytes(np.asarray(G.generate([b"a"], count=n, u=u)[0], np.uint8).reshape(n))
    assert len(text) >= 200
    zs = []
    for h, Pm in ((L, P), (G, Pg)):
        Why, by = _why(Pm, h.N)
        st = np.asarray(h.generate([text[:j] for j in range(1, n)], count=0)[2], f32).reshape(n - 1, h.N)
        st = np.concatenate([np.zeros((1, h.N), f32), st])
        zs.append([logits32(Why, by, st[j]) for j in range(n)])
    zs_of = lambda j: [zs[0][j], zs[1][j]]
    sym = np.frombuffer(text, np.uint8)
    ref_fixed = mr.steps(sym, zs_of, (0.5, 0.5), 0.0)[3]
    ref_learned = mr.steps(sym, zs_of, (0.5, 0.5), rate)[3]
    margin = ref_fixed - ref_learned
    assert margin >= 0.05 * ref_fixed, (ref_fixed, ref_learned)  # visible in the reference
    fixed = L.encode_mixed([text], guides=[(G, 0.5)], main_weight=0.5, rate=0.0)
    codes, bits, w_out, w_trace = L.encode_mixed([text], guides=[(G, 0.5)], main_weight=0.5, rate=rate, weights=True)
    print(f"reference: fixed {ref_fixed:.2f} bits, learned {ref_learned:.2f}; device: fixed {fixed[1][0]:.2f}, learned {bits[0]:.2f}; "
          f"final weights {w_out[0]}")
    assert fixed[1][0] - bits[0] >= 0.5 * margin, (fixed[1][0], bits[0], margin)
    assert w_out[0, 1] > 0.5 and len(codes[0]) < len(fixed[0][0])
    assert L.decode_mixed(codes, [n], guides=[(G, 0.5)], main_weight=0.5, rate=rate) == [text]


def _snapshot(L):
    import lstm_hip
    return ([L.get_params(w).tobytes() for w in (lstm_hip.P_PARAMS, lstm_hip.P_GRADS, lstm_hip.P_MEM)]
            + [a.tobytes() for a in L.get_window()] + [L.get_cursors().tobytes(), L.optimizer_steps()])


def test_a_mixed_call_leaves_both_handles_as_they_were():
    import lstm_hip
    S, B = 6, 2
    text = np.random.RandomState(81).randint(97, 123, size=3000).astype(np.uint8)
    hs = []
    for n, seed in ((N, 5), (GN, 6)):
        L = lstm_hip.Lstm(n, S, B)
        L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(seed), n))
        L.set_text(text)
        L.set_cursors(lstm_hip.initial_cursors(text.size, S, B))
        L.train_windows(3, 0.1)
        hs.append(L)
    A, G = hs
    before = [_snapshot(A), _snapshot(G)]
    texts = [b"hello world", b"", b"ab"]
    codes, _ = A.encode_mixed(texts, guides=[(G, 0.5), (A, 0.25)], main_weight=0.5, rate=RATE)
    assert A.decode_mixed(codes, [len(t) for t in texts], guides=[(G, 0.5), (A, 0.25)], main_weight=0.5, rate=RATE) == texts
    assert [_snapshot(A), _snapshot(G)] == before
    la, lg = A.train_windows(2, 0.1), G.train_windows(2, 0.1)
    assert np.isfinite(la).all() and np.isfinite(lg).all()
    A.close()
    G.close()
