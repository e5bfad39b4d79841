"""-m gpu: lstm_hip_score_guided -- per-byte scores under a log-linear mix with other models (include/lstm_hip.h, DESIGN.md
section 3.24).

With the block NULL the call is lstm_hip_score byte for byte; weights (0, 1) give the guide handle's own scores; general
weights give the float32 reference (tests/guided_ref.py) on the device's own states, with and without a table, first 0 and 1;
a text scored in pieces with every model's state handed over is the one call; and the bytes of greedy guided generation are
the first alternatives of the guided score of prompt ++ out.

Against the float32 reference the ranks and the alternatives' bytes are compared exactly: they are functions of the mixed
logits, which the reference forms with the device's own operations.  Surprisal, entropy and the alternatives' bits pass
through expf and log2f, the device's here and the C library's in the reference, each good to about an ulp: a term of the
256-term sum may differ by 2^-23 relative and the two sequential sums may round apart at each of their 256 additions, so a
probability agrees to about 258 * 2^-24 = 1.6e-5 relative, 2.3e-5 bits, and log2f adds an ulp of a value near 10, 1e-6.  The
bound is score_ref.BOUND = 1e-4 bits, the margin the unguided scorer is held to (tests/test_score.py); what the guided call
adds ahead of expf is exact in the reference."""
import ctypes as C

import numpy as np
import pytest

import guided_ref as gr
import sampling_ref as sr
import score_ref as sc
from logits_ref import logits32 as _logits32
from oracle_lib import split_params

pytestmark = pytest.mark.gpu
M = 256
f32 = np.float32
N, GN, K = 16, 32, 20
PER_BYTE = ("surprisal", "entropy", "rank", "top_byte", "top_bits")


def _state(streams, n, seed):
    rs = np.random.RandomState(seed)
    return (rs.randn(streams, n) * 0.1).astype(f32), (rs.randn(streams, n) * 0.1).astype(f32)


@pytest.fixture(scope="module")
def models():
    import lstm_hip
    Ps = [sr.peaked_params(N, seed=7, gain=6.0), sr.peaked_params(GN, seed=8, gain=6.0)]
    hs = []
    for n, P in zip((N, GN), Ps):
        L = lstm_hip.Lstm(n, 2, 1)
        L.set_params(P)
        hs.append(L)
    yield list(zip(hs, Ps))
    for h in hs:
        h.close()


def _texts(rs, lo=97, hi=123):
    """texts of (3 s) % 7 letters: empty ones and one-byte ones occur"""
    return [rs.randint(lo, hi, size=(3 * s) % 7).astype(np.uint8) for s in range(K)]


def _same(a, b, keys=PER_BYTE + ("bits", "h", "c")):
    for k in keys:
        if isinstance(a[k], list):
            if not all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a[k], b[k])):
                return False
        elif np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes():
            return False
    return True


def _raw(L, fn, texts, h0, c0, first, top_n, table):
    """lstm_hip_score (fn = "score") or lstm_hip_score_guided with gd NULL through ctypes: Lstm.score's dict"""
    import lstm_hip
    p = lstm_hip._ptr
    parts = lstm_hip._bytes_list(texts)
    data, off = lstm_hip._offsets(parts)
    Kn, total = len(parts), int(off[-1])
    sur, ent, rank = np.zeros(total, f32), np.zeros(total, f32), np.zeros(total, np.uint8)
    tby, tbi = np.zeros((total, top_n), np.uint8), np.zeros((total, top_n), f32)
    bits, h, c, q1 = np.zeros(Kn), np.empty((Kn, L.N), f32), np.empty((Kn, L.N), f32), np.zeros(Kn, np.int32)
    con = None
    if table is not None:
        t = np.ascontiguousarray(table, np.uint16)
        con = lstm_hip._Constraint(C.sizeof(lstm_hip._Constraint), t.shape[0], p(t, C.c_uint16))
    opt = lstm_hip._Scoring(C.sizeof(lstm_hip._Scoring), int(first), top_n, C.pointer(con) if con is not None else None)
    out = lstm_hip._Scores(C.sizeof(lstm_hip._Scores), p(sur), p(ent), p(rank, C.c_uint8), p(tby, C.c_uint8), p(tbi), p(bits, C.c_double),
                           p(q1, C.c_int32) if con is not None else None)
    args = [L._h, C.c_int32(Kn), p(data, C.c_uint8), p(off, C.c_uint64), p(h0), p(c0), C.byref(opt), None, C.byref(out), p(h), p(c)]
    rc = L.lib.lstm_hip_score(*args) if fn == "score" else L.lib.lstm_hip_score_guided(*args, None)
    assert rc == 0, L.lib.lstm_hip_last_error()
    cut = lambda a: [a[int(off[s]):int(off[s + 1])] for s in range(Kn)]
    return {"surprisal": cut(sur), "entropy": cut(ent), "rank": cut(rank), "top_byte": cut(tby), "top_bits": cut(tbi), "bits": bits,
            "h": h, "c": c, "end_state": q1}


@pytest.mark.parametrize("with_table", [False, True])
def test_a_null_block_is_the_score_call(models, with_table):
    import lstm_hip
    L = models[0][0]
    texts = _texts(np.random.RandomState(3))
    h0, c0 = _state(K, N, seed=4)
    table = lstm_hip.dfa_utf8() if with_table else None
    for first in (0, 1):
        a, b = _raw(L, "score", texts, h0, c0, first, 3, table), _raw(L, "guided", texts, h0, c0, first, 3, table)
        assert _same(a, b) and np.array_equal(a["end_state"], b["end_state"]), first
        assert sum(float(x.sum()) for x in a["surprisal"]) > 0


def test_weights_0_1_are_the_guides_own_scores(models):
    import lstm_hip
    (L, _), (G, _) = models
    texts = _texts(np.random.RandomState(5))
    h0, c0 = _state(K, N, seed=6)
    gh0, gc0 = _state(K, GN, seed=7)
    for first, table in ((0, None), (1, None), (1, lstm_hip.dfa_utf8())):
        want = G.score(texts, h0=gh0, c0=gc0, first=first, top_n=3, constraint=table)
        got = L.score_guided(texts, h0=h0, c0=c0, first=first, top_n=3, constraint=table, guides=[(G, 1.0, gh0, gc0)], main_weight=0.0)
        assert _same(got, want, PER_BYTE + ("bits",)), first
        assert got["guide_h"][0].tobytes() == want["h"].tobytes() and got["guide_c"][0].tobytes() == want["c"].tobytes()
        alone = L.score(texts, h0=h0, c0=c0, first=first)
        assert got["h"].tobytes() == alone["h"].tobytes() and got["c"].tobytes() == alone["c"].tobytes()
        if table is not None:
            assert np.array_equal(got["end_state"], want["end_state"])


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("with_table", [False, True])
def test_general_weights_are_the_float32_reference(models, first, with_table):
    import lstm_hip
    (L, P), (G, Pg) = models
    a, b = 1.5, -0.5
    rs = np.random.RandomState(8 + first)
    table = lstm_hip.dfa_regex(b"(?:[a-m]x?|[n-z]{1,2}q)*", stop_byte=-1)[0] if with_table else None
    texts = []
    for s in range(K):  # texts the table takes
        q, t = 0, []
        for _ in range((3 * s) % 7):
            good = [x for x in range(97, 123) if table is None or table[q, x] != sc.FORBID]
            x = int(rs.choice(good))
            t.append(x)
            q = int(table[q, x]) if table is not None else 0
        texts.append(np.array(t, np.uint8))
    h0, c0 = _state(K, N, seed=9)
    gh0, gc0 = _state(K, GN, seed=10)
    got = L.score_guided(texts, h0=h0, c0=c0, first=first, top_n=3, constraint=table, guides=[(G, b, gh0, gc0)], main_weight=a)
    plain = L.score(texts, h0=h0, c0=c0, first=first, top_n=3, constraint=table)
    longest = max(t.size for t in texts)
    H = [L.generate([t[:j] for t in texts], count=0, h0=h0, c0=c0)[2] for j in range(longest + 1)]
    GH = [G.generate([t[:j] for t in texts], count=0, h0=gh0, c0=gc0) for j in range(longest + 1)]
    params = []
    for Pm, n in ((P, N), (Pg, GN)):
        sp = split_params(np.asarray(Pm, f32), n)
        params.append((np.asarray(sp["Why"], f32), np.asarray(sp["by"], f32).reshape(M)))
    scored = moved = 0
    worst = 0.0
    for s, t in enumerate(texts):
        q, bits = 0, 0.0
        for j in range(t.size):
            ok = None if table is None else np.asarray(table[q]) != sc.FORBID
            q = int(table[q, t[j]]) if table is not None else 0
            g = [np.asarray(got[k][s][j]) for k in PER_BYTE]
            if j == 0 and not first:
                assert not any(np.any(v != 0) for v in g), (s, j)
                continue
            z, zg = _logits32(*params[0], H[j][s]), _logits32(*params[1], GH[j][2][s])
            w = gr.statement32(z, [zg], a, [b], t[j], False, ok, 3)
            # rank and alternatives come from the mixed logits alone, which are the reference's bit for bit; the bits go through
            # expf and log2f, the device's on one side and the C library's on the other (see the module's docstring)
            assert int(g[2]) == w[2] and np.array_equal(g[3], w[3]), (s, j, g[2], w[2], g[3], w[3])
            worst = max(worst, abs(float(g[0]) - float(w[0])), abs(float(g[1]) - float(w[1])))
            fin = np.isfinite(w[4])
            assert np.array_equal(np.isfinite(g[4]), fin), (s, j)
            worst = max(worst, float(np.abs(g[4][fin] - w[4][fin]).max()))
            bits += float(g[0])
            scored += 1
            moved += abs(float(g[0]) - float(plain["surprisal"][s][j])) > 10 * sc.BOUND
        assert got["bits"][s] == bits, s  # the double sum, in text order, of the surprisals the call itself returned
        assert got["h"][s].tobytes() == H[t.size][s].tobytes(), s
        assert got["guide_h"][0][s].tobytes() == GH[t.size][2][s].tobytes() and got["guide_c"][0][s].tobytes() == GH[t.size][3][s].tobytes(), s
    print(f"first {first} table {with_table}: scored {scored}, the guide moved {moved}, largest difference {worst:.3g} bits")
    assert worst <= sc.BOUND, worst
    assert scored >= 40 and moved >= scored // 2, (scored, moved)


def test_pieces_chain(models):
    (L, _), (G, _) = models
    rs = np.random.RandomState(12)
    texts = [rs.randint(97, 123, size=4 + (5 * s) % 9).astype(np.uint8) for s in range(K)]
    cuts = [(2 * s) % (t.size + 1) for s, t in enumerate(texts)]  # empty first and second pieces occur
    h0, c0 = _state(K, N, seed=13)
    gh0, gc0 = _state(K, GN, seed=14)
    kw = dict(top_n=3, main_weight=0.6)
    one = L.score_guided(texts, h0=h0, c0=c0, first=True, guides=[(G, 0.4, gh0, gc0)], **kw)
    p1 = L.score_guided([t[:k] for t, k in zip(texts, cuts)], h0=h0, c0=c0, first=True, guides=[(G, 0.4, gh0, gc0)], **kw)
    p2 = L.score_guided([t[k:] for t, k in zip(texts, cuts)], h0=p1["h"], c0=p1["c"], first=True,
                 guides=[(G, 0.4, p1["guide_h"][0], p1["guide_c"][0])], **kw)
    for k in PER_BYTE:
        for s in range(K):
            joined = np.concatenate([p1[k][s], p2[k][s]])
            assert joined.tobytes() == np.asarray(one[k][s]).tobytes(), (k, s)
    for k in ("h", "c"):
        assert one[k].tobytes() == p2[k].tobytes()
    assert one["guide_h"][0].tobytes() == p2["guide_h"][0].tobytes() and one["guide_c"][0].tobytes() == p2["guide_c"][0].tobytes()


def test_greedy_guided_bytes_are_the_first_alternatives_of_the_guided_score(models):
    (L, _), (G, _) = models
    rs = np.random.RandomState(15)
    prompts = [rs.randint(97, 123, size=1 + (3 * s) % 5).astype(np.uint8) for s in range(K)]
    h0, c0 = _state(K, N, seed=16)
    gh0, gc0 = _state(K, GN, seed=17)
    count = 10
    g = dict(guides=[(G, -0.5, gh0, gc0)], main_weight=1.5)
    out = L.generate(prompts, count=count, temperature=0.0, h0=h0, c0=c0, **g)[0]
    plain = L.generate(prompts, count=count, temperature=0.0, h0=h0, c0=c0)[0]
    assert not np.array_equal(out, plain)
    got = L.score_guided([np.concatenate([prompts[s], out[:, s]]) for s in range(K)], h0=h0, c0=c0, top_n=1, **g)
    for s in range(K):
        n = prompts[s].size
        assert np.array_equal(got["top_byte"][s][n:, 0], out[:, s]), s
        assert (got["rank"][s][n:] == 0).all(), s
