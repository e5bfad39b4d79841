"""-m gpu: lstm_hip_score -- per-byte surprisal, entropy, rank and alternatives (include/lstm_hip.h).

Bit for bit: the streams' bits are lstm_hip_generate's prompt bits and the double sum of the surprisals; a batch is each of its
streams alone; wide batches (4 and 16 streams a workgroup) are batches of eight; two chained calls are the one call.  Against
the oracle every scored byte lies within 1e-4 bits of the float64 statement of tests/score_ref.py, ranks and alternatives
under its comparison rule (whose control is tests/test_score_cpu.py).  Greedy decoding scores at rank 0; a table masks, and
its refusals, the handle kinds, the trainer's state, non-finite parameters and the program behave as the contract says."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import score_ref as sc
import sampling_ref as sr
from test_pad_hidden import pad_cols, pad_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSTM = os.path.join(ROOT, "eigen-lstm_amd", "lstm")
GEN = os.path.join(ROOT, "eigen-lstm_amd", "lstm_generate")
PER_BYTE = ("surprisal", "entropy", "rank", "top_byte", "top_bits")
STABLE = 512  # LSTM_HIP_STABLE_SOFTMAX


def _state(streams, N, seed):
    rs = np.random.RandomState(seed)
    return (rs.randn(streams, N) * 0.1).astype(np.float32), (rs.randn(streams, N) * 0.1).astype(np.float32)


def _texts(lengths, seed):
    import gpu_util as gu
    data = gu.text_bytes(int(np.sum(lengths)) + 1, seed)
    cuts = np.concatenate([[0], np.cumsum(lengths)]).astype(int)
    return [data[cuts[i]:cuts[i + 1]] for i in range(len(lengths))]


def _same(a, b, keys=PER_BYTE + ("bits", "h", "c")):
    """two results of Lstm.score agree bit for bit"""
    for k in keys:
        x, y = a[k], b[k]
        if isinstance(x, list):
            if len(x) != len(y) or not all(np.asarray(p).tobytes() == np.asarray(q).tobytes() and np.asarray(p).shape == np.asarray(q).shape
                                           for p, q in zip(x, y)):
                return False
        elif np.asarray(x).tobytes() != np.asarray(y).tobytes():
            return False
    return True


def _pick(res, idx):
    """the streams `idx` of a result"""
    out = {k: [res[k][i] for i in idx] for k in PER_BYTE}
    out.update(bits=res["bits"][idx], h=res["h"][idx], c=res["c"][idx])
    return out


def _plain(L, texts, h0=None, c0=None, first=False):
    """lstm_hip_score asked for surprisal, entropy and bits only, which the head without the ranking serves (Lstm.score always
    asks for rank): the three flat arrays"""
    import lstm_hip
    p = lstm_hip._ptr
    data, off = lstm_hip._offsets(lstm_hip._bytes_list(texts))
    total, K = max(int(off[-1]), 1), len(texts)
    sur, ent, bits = np.zeros(total, np.float32), np.zeros(total, np.float32), np.zeros(K)
    opt = lstm_hip._Scoring(C.sizeof(lstm_hip._Scoring), int(first), 0, None)
    out = lstm_hip._Scores(C.sizeof(lstm_hip._Scores), p(sur), p(ent), None, None, None, p(bits, C.c_double), None)
    rc = L.lib.lstm_hip_score(L._h, C.c_int32(K), p(data, C.c_uint8), p(off, C.c_uint64), p(h0) if h0 is not None else None,
                              p(c0) if c0 is not None else None, C.byref(opt), None, C.byref(out), None, None)
    assert rc == 0, L.lib.lstm_hip_last_error()
    return sur[:int(off[-1])], ent[:int(off[-1])], bits


def _handle(N, P, flags=0):
    import lstm_hip
    L = lstm_hip.Lstm(N, 2, 1, flags=flags)
    L.set_params(P)
    return L


@pytest.mark.parametrize("N,scale", [(64, 0.2), (512, 0.04)])
@pytest.mark.parametrize("flags", [0, STABLE])
def test_bits_are_the_generators_prompt_bits(N, scale, flags):
    lengths = [0, 1, 2, 5, 17, 40, 33, 8, 3, 24]
    K = len(lengths)
    texts = _texts(lengths, seed=N)
    h0, c0 = _state(K, N, seed=N + 1)
    L = _handle(N, sr.peaked_params(N, seed=3, scale=scale), flags)
    _, bits, h, c = L.generate(texts, count=0, h0=h0, c0=c0, score=True)
    got = L.score(texts, h0=h0, c0=c0, top_n=2)
    assert np.isfinite(bits).all() and bits[5] > 0
    assert np.array_equal(got["bits"], bits) and np.array_equal(got["h"], h) and np.array_equal(got["c"], c)
    for first in (False, True):  # the instantiation without the ranking gives the same figures
        full = L.score(texts, h0=h0, c0=c0, first=first)
        sur, ent, pbits = _plain(L, texts, h0, c0, first)
        assert sur.tobytes() == np.concatenate(full["surprisal"]).tobytes() and ent.tobytes() == np.concatenate(full["entropy"]).tobytes()
        assert np.array_equal(pbits, full["bits"])
    # from a zero state bits / (L - 1) is the evaluator's figure, and first = 1 scores byte 0 in front of the same entries
    zero = L.score(texts)
    one = L.score(texts, first=True)
    for res in (got, zero, one):
        for s in range(K):
            total = 0.0
            for v in res["surprisal"][s]:  # the double sum in text order
                total += float(v)
            assert total == res["bits"][s], s
            assert np.isfinite(res["surprisal"][s]).all() and (res["surprisal"][s] >= 0).all() and (res["entropy"][s] >= 0).all()
            if lengths[s] and res is not one:
                assert res["surprisal"][s][0] == 0 and res["entropy"][s][0] == 0 and res["rank"][s][0] == 0 and not res["top_byte"][s][0].any()
    for s in (4, 5):
        assert abs(zero["bits"][s] / (lengths[s] - 1) - L.eval_bits(texts[s])) <= 1e-5, s
        assert np.array_equal(one["surprisal"][s][1:], zero["surprisal"][s][1:]) and one["surprisal"][s][0] > 0 and one["entropy"][s][0] > 0
    L.close()


@pytest.mark.parametrize("flags", [0, STABLE])
def test_the_batch_is_each_stream_alone(flags):
    N, lengths = 64, [7, 0, 1, 30, 12, 2]
    texts = _texts(lengths, seed=11)
    h0, c0 = _state(len(lengths), N, seed=12)
    L = _handle(N, sr.peaked_params(N, seed=13), flags)
    batch = L.score(texts, h0=h0, c0=c0, first=True, top_n=3)
    for s in range(len(lengths)):
        alone = L.score([texts[s]], h0=h0[s:s + 1], c0=c0[s:s + 1], first=True, top_n=3)
        assert _same(alone, _pick(batch, [s])), s
    L.close()


@pytest.mark.parametrize("K,n", [(1030, 8), (4096, 6)])
def test_wide_batches_match_batches_of_eight(K, n):
    """score_head puts 4 (1030 streams: a partial last group) and 16 (4096) streams into one workgroup: every stream must come
    out as it does in a batch of 8 (one stream per workgroup)."""
    import lstm_hip
    N = 64
    rs = np.random.RandomState(K)
    texts = list(_texts([n] * K, seed=K + 1))
    h0, c0 = _state(K, N, seed=K + 2)
    table = lstm_hip.dfa_restrict(np.zeros((1, 256), np.uint16), np.bincount(np.concatenate(texts), minlength=256) > 0)
    L = _handle(N, sr.peaked_params(N, seed=41))
    kw = dict(first=True, top_n=4) if K == 1030 else dict(top_n=8, constraint=table)
    wide = L.score(texts, h0=h0, c0=c0, **kw)
    if K == 1030:
        groups = [np.arange(g, min(g + 8, K)) for g in range(0, K, 8)]  # all of them
    else:  # the first and the last two workgroups' streams in every position, and a few more
        pick = np.unique(np.concatenate([np.arange(32), np.arange(K - 32, K), rs.choice(K, 16, replace=False)]))
        groups = [pick[g:g + 8] for g in range(0, pick.size, 8)]
    for g in groups:
        small = L.score([texts[i] for i in g], h0=h0[g], c0=c0[g], **kw)
        assert _same(small, _pick(wide, g)), g
    L.close()


@pytest.mark.parametrize("flags,constrained", [(0, False), (STABLE, True)])
def test_chained_calls_are_the_one_call(flags, constrained):
    import lstm_hip
    N, lengths = 64, [40, 1, 0, 17, 2, 33]
    K = len(lengths)
    if constrained:
        table = lstm_hip.dfa_utf8()
        text = ("één cyclus: ∮ 🙂 zwölf naïve 日本 " * 3).encode()
        texts = [np.frombuffer(text[:n], np.uint8) for n in lengths]  # (the cut may fall inside a character: no boundary is asked for)
        kw = dict(constraint=table)
    else:
        texts, kw = _texts(lengths, seed=21), dict()
    h0, c0 = _state(K, N, seed=22)
    L = _handle(N, sr.peaked_params(N, seed=23), flags)
    for first in (False, True):
        whole = L.score(texts, h0=h0, c0=c0, first=first, top_n=3, **kw)
        cut = [n // 2 for n in lengths]
        a = L.score([t[:n] for t, n in zip(texts, cut)], h0=h0, c0=c0, first=first, top_n=3, **kw)
        if constrained:
            kw2 = dict(kw, start_state=a["end_state"])
            assert any(a["end_state"] != 0)  # some stream was cut inside a character
        else:
            kw2 = kw
        b = L.score([t[n:] for t, n in zip(texts, cut)], h0=a["h"], c0=a["c"], first=True, top_n=3, **kw2)
        for s in range(K):
            for k in PER_BYTE:
                joined = np.concatenate([a[k][s], b[k][s]])
                if cut[s] == 0 and not first and lengths[s]:  # the one call leaves byte 0 unscored, the second piece scored it
                    assert joined[0].any() or k == "rank"
                    joined[0] = 0
                assert joined.tobytes() == whole[k][s].tobytes(), (first, s, k)
        assert np.array_equal(b["h"], whole["h"]) and np.array_equal(b["c"], whole["c"])
        if constrained:
            assert np.array_equal(b["end_state"], whole["end_state"])
    L.close()


@pytest.mark.parametrize("flags", [0, STABLE])
@pytest.mark.parametrize("first", [False, True])
def test_every_byte_against_the_oracle(oracle64, flags, first):
    """The control's case (tests/test_score_cpu.py): surprisal, entropy and the alternatives' bits within 1e-4 bits of the
    float64 statement, ranks and top-4 lists under its comparison rule."""
    N, P, texts, h0, c0 = sc.oracle_case()
    want = sc.score64(oracle64, N, P, texts, h0, c0, first=first, top_n=4)
    L = _handle(N, P, flags)
    got = L.score(list(texts), h0=h0, c0=c0, first=first, top_n=4)
    L.close()
    fig, fails = sc.compare(got, want, first, 4)
    print(f"flags {flags} first {first}: surprisal {fig['surprisal']:.3g} entropy {fig['entropy']:.3g} top_bits {fig['top_bits']:.3g} bits; "
          f"left out {fig['left_out_rank']} / {fig['left_out_top']} of {fig['scored']}")
    assert fails == [], fails[:5]
    assert fig["surprisal"] <= 1e-4 and fig["entropy"] <= 1e-4 and fig["top_bits"] <= 1e-4
    assert fig["scored"] == 8 * (48 if first else 47)


@pytest.mark.parametrize("constrained", [False, True])
def test_greedy_bytes_score_at_rank_zero(constrained):
    import lstm_hip
    N, Cn = 128, 60
    rs = np.random.RandomState(31)
    prompts = [rs.randint(97, 123, size=n).astype(np.uint8) for n in (3, 0, 17, 1, 9)]
    K = len(prompts)
    h0, c0 = _state(K, N, seed=32)
    L = _handle(N, sr.peaked_params(N, seed=31, scale=0.1))
    if constrained:
        table = lstm_hip.dfa_restrict(lstm_hip.dfa_utf8(), np.r_[np.zeros(97), np.ones(26), np.zeros(5), np.ones(128)])  # a-z and non-ASCII
        out, _, h, c, info = L.generate(prompts, count=Cn, temperature=0.0, h0=h0, c0=c0, info=True, constraint=table)
        free = L.generate(prompts, count=Cn, temperature=0.0, h0=h0, c0=c0)[0]
        assert not np.array_equal(free, out)  # the table changes the greedy text (a property of the seed)
        kw = dict(constraint=table)
    else:
        out, _, h, c = L.generate(prompts, count=Cn, temperature=0.0, h0=h0, c0=c0)
        kw = dict()
    texts = [np.concatenate([prompts[s], out[:, s]]) for s in range(K)]
    got = L.score(texts, h0=h0, c0=c0, first=True, top_n=1, **kw)
    for s in range(K):
        n = prompts[s].size
        assert not got["rank"][s][n:].any(), s
        assert np.array_equal(got["top_byte"][s][n:, 0], out[:, s]), s
        assert np.array_equal(got["top_bits"][s][n:, 0], got["surprisal"][s][n:]), s
    assert np.array_equal(got["h"], h) and np.array_equal(got["c"], c)
    if constrained:
        assert np.array_equal(got["end_state"], info["end_state"])
    assert any(r[:p.size].any() for r, p in zip(got["rank"], prompts))  # (the random prompts are not the model's guesses)
    L.close()


@pytest.mark.parametrize("flags", [0, STABLE])
def test_an_all_allowed_table_changes_nothing(flags):
    N, lengths = 64, [9, 0, 1, 25]
    texts = _texts(lengths, seed=41)
    h0, c0 = _state(len(lengths), N, seed=42)
    L = _handle(N, sr.peaked_params(N, seed=43), flags)
    for first in (False, True):
        free = L.score(texts, h0=h0, c0=c0, first=first, top_n=8)
        got = L.score(texts, h0=h0, c0=c0, first=first, top_n=8, constraint=np.zeros((1, 256), np.uint16))
        assert _same(free, got) and not got["end_state"].any()
    L.close()


def test_utf8_table_removes_the_forbidden_mass(oracle64):
    import lstm_hip
    table = lstm_hip.dfa_utf8()
    N = 64
    P = sr.peaked_params(N, seed=41)
    texts = [np.frombuffer(t.encode(), np.uint8) for t in ("één cyclus: ∮ 🙂.", "zwölf naïve 日本 🙂🙂", "plain ascii")]
    K = len(texts)
    h0, c0 = _state(K, N, seed=52)
    L = _handle(N, P)
    free = L.score(texts, h0=h0, c0=c0, first=True, top_n=8)
    con = L.score(texts, h0=h0, c0=c0, first=True, top_n=8, constraint=table)
    L.close()
    want = sc.score64(oracle64, N, P, texts, h0, c0, first=True)
    worst, states = 0.0, set()
    for s in range(K):
        q = 0
        for j, b in enumerate(texts[s]):
            ok = table[q] != sc.FORBID
            states.add(q)
            mass = np.exp(want["lnp"][s][j][ok]).sum()
            worst = max(worst, abs(float(con["surprisal"][s][j]) - float(free["surprisal"][s][j]) - np.log2(mass)))
            A = int(ok.sum())
            assert con["rank"][s][j] < A and con["rank"][s][j] <= free["rank"][s][j]
            assert ok[con["top_byte"][s][j]].all() and np.isfinite(con["top_bits"][s][j]).all()  # (every state allows 16 or more)
            q = int(table[q, b])
        assert con["end_state"][s] == 0
    print(f"constrained - unconstrained surprisal against log2 of the allowed mass: {worst:.3g} bits; states {sorted(states)}")
    assert worst <= 1e-4 and states >= {0, 1, 2, 6}


@pytest.mark.parametrize("flags", [0, STABLE])
def test_forbidden_alternatives_have_infinite_bits(flags):
    text = np.frombuffer("één cyclus: ∮ 🙂.\n".encode(), np.uint8)
    T = text.size
    table = np.full((T, 256), sc.FORBID, np.uint16)  # one allowed byte per state: the cycle forces its text
    table[np.arange(T), text] = (np.arange(T) + 1) % T
    N, K = 64, 3
    start = np.array([0, 7, T - 1], np.int32)
    texts = [text[(start[s] + np.arange(n)) % T] for s, n in enumerate((30, 5, 1))]
    h0, c0 = _state(K, N, seed=62)
    L = _handle(N, sr.peaked_params(N, seed=61), flags)
    got = L.score(texts, h0=h0, c0=c0, first=True, top_n=8, constraint=table, start_state=start)
    L.close()
    for s in range(K):
        n = texts[s].size
        assert not got["surprisal"][s].any() and not got["entropy"][s].any() and not got["rank"][s].any(), s  # p = 1
        assert np.array_equal(got["top_byte"][s][:, 0], texts[s]) and not got["top_bits"][s][:, 0].any()
        assert np.isposinf(got["top_bits"][s][:, 1:]).all()
        for j in range(n):  # the forbidden bytes follow in index order
            assert list(got["top_byte"][s][j, 1:]) == [b for b in range(9) if b != texts[s][j]][:7], (s, j)
        assert got["end_state"][s] == (start[s] + n) % T
    assert not got["bits"].any()


def test_bf16_padded_and_step_kernel_handles_match_their_twins():
    import lstm_hip
    table = lstm_hip.dfa_utf8()
    texts = [np.frombuffer(t.encode(), np.uint8) for t in ("een twee drie vier vijf", "", "é", "zwölf naïve 日本 🙂🙂 en verder")]
    K = len(texts)
    kw = dict(first=True, top_n=4, constraint=table)
    for twin, N in ((lstm_hip.BF16_RECURRENCE, 128), (lstm_hip.STEP_KERNELS, 64)):  # the scorer runs on the fp32 master weights
        P = sr.peaked_params(N, seed=73, scale=0.1)
        h0, c0 = _state(K, N, seed=74)
        res = []
        for flags in (0, twin):
            L = lstm_hip.Lstm(N, 2, 8, flags=flags)
            L.set_params(P)
            res.append(L.score(texts, h0=h0, c0=c0, **kw))
            L.close()
        assert _same(*res) and np.array_equal(res[0]["end_state"], res[1]["end_state"]), twin
    # N = 100 padded to 128 against an explicit 128 handle with zero-padded parameters and state
    N, Np = 100, 128
    P = sr.peaked_params(N, seed=75, scale=0.1)
    h0, c0 = _state(K, N, seed=76)
    A = _handle(N, P, lstm_hip.PAD_HIDDEN)
    ra = A.score(texts, h0=h0, c0=c0, **kw)
    A.close()
    Bh = _handle(Np, pad_params(P, N, Np))
    rb = Bh.score(texts, h0=pad_cols(h0, N, Np), c0=pad_cols(c0, N, Np), **kw)
    Bh.close()
    assert _same(ra, rb, PER_BYTE + ("bits",))
    assert np.array_equal(ra["h"], rb["h"][:, :N]) and np.array_equal(ra["c"], rb["c"][:, :N])
    assert ra["h"].shape == (K, N) and np.array_equal(ra["h"][1], h0[1])  # an empty stream ends in its start state


def _trainer(text, N, S, B):
    import lstm_hip
    L = lstm_hip.Lstm(N, S, B)
    L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(5), N))
    L.set_text(text)
    L.set_cursors(lstm_hip.initial_cursors(text.size, S, B))
    return L


def test_training_state_is_untouched_by_scoring():
    import lstm_hip
    N, S, B = 64, 8, 4
    text = np.random.RandomState(81).randint(97, 123, size=5000).astype(np.uint8)
    A, Bh = _trainer(text, N, S, B), _trainer(text, N, S, B)
    la = [A.train_windows(5, 0.1)]
    got = A.score([text[:50], text[100:103]], first=True, top_n=8, constraint=lstm_hip.dfa_utf8())
    assert got["surprisal"][0].shape == (50,)
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


def test_refusals_leave_a_usable_handle():
    import lstm_hip
    N, S, B = 32, 6, 2
    text = np.random.RandomState(91).randint(97, 123, size=2000).astype(np.uint8)
    L = _trainer(text, N, S, B)
    lib, p = L.lib, lstm_hip._ptr
    K = 3
    data = np.frombuffer(b"abcdefgh", np.uint8).copy()
    good_off = np.array([0, 2, 5, 8], np.uint64)
    utf8 = lstm_hip.dfa_utf8()
    bufs = dict(sur=np.zeros(8, np.float32), ent=np.zeros(8, np.float32), rank=np.zeros(8, np.uint8), tby=np.zeros(64, np.uint8),
                tbi=np.zeros(64, np.float32), bits=np.zeros(K), end=np.zeros(K, np.int32))

    def con(table, states=None, sz=C.sizeof(lstm_hip._Constraint), null=False):
        table = np.ascontiguousarray(table, np.uint16)
        c = lstm_hip._Constraint(sz, table.shape[0] if states is None else states, None if null else p(table, C.c_uint16))
        c._keep = table
        return c

    def call(first=0, top_n=2, c=None, start=None, opt_size=None, out_size=None, streams=K, off=good_off, text=data, top=True,
             end=False, null_opt=False):
        opt = lstm_hip._Scoring(C.sizeof(lstm_hip._Scoring) if opt_size is None else opt_size, first, top_n,
                                C.pointer(c) if c is not None else None)
        out = lstm_hip._Scores(C.sizeof(lstm_hip._Scores) if out_size is None else out_size, p(bufs["sur"]), p(bufs["ent"]),
                               p(bufs["rank"], C.c_uint8), p(bufs["tby"], C.c_uint8) if top else None, p(bufs["tbi"]) if top else None,
                               p(bufs["bits"], C.c_double), p(bufs["end"], C.c_int32) if end else None)
        return lib.lstm_hip_score(L._h, C.c_int32(streams), p(text, C.c_uint8) if text is not None else None,
                                  p(off, C.c_uint64) if off is not None else None, None, None, None if null_opt else C.byref(opt),
                                  p(start, C.c_int32) if start is not None else None, C.byref(out), None, None)

    def refused(words, **kw):
        rc = call(**kw)
        msg = lib.lstm_hip_last_error().decode()
        assert rc == lstm_hip.EINVAL, (words, rc, msg)
        assert msg.startswith("score:") and all(w in msg for w in words), (words, msg)

    assert call() == 0, lib.lstm_hip_last_error()
    refused(["null options"], null_opt=True)
    refused(["options of", "bytes"], opt_size=C.sizeof(lstm_hip._Scoring) - 8)
    refused(["options of", "bytes"], opt_size=0)
    refused(["outputs of", "bytes"], out_size=C.sizeof(lstm_hip._Scores) + 8)
    refused(["top_n", "[0, 8]"], top_n=9)
    refused(["top_n", "[0, 8]"], top_n=-1)
    refused(["first", "0 or 1"], first=2)
    refused(["first", "0 or 1"], first=-1)
    refused(["top_byte", "top_n = 0"], top_n=0)
    assert call(top_n=0, top=False) == 0
    starts = np.zeros(K, np.int32)
    refused(["start_state", "without a constraint"], start=starts)
    refused(["end_state", "without a constraint"], end=True)
    refused(["streams", "[1, 4096]"], streams=0)
    refused(["streams", "[1, 4096]"], streams=4097)
    refused(["null text_off"], off=None)
    refused(["text_off[0] must be 0"], off=np.array([1, 2, 5, 8], np.uint64))
    refused(["text_off decreases at stream 1"], off=np.array([0, 5, 2, 8], np.uint64))
    refused(["null text"], text=None)
    assert call(text=None, off=np.zeros(K + 1, np.uint64)) == 0  # nothing to score: no text is needed
    # the table checks of lstm_hip_generate_constrained
    refused(["constraint of", "bytes"], c=con(utf8, sz=12))
    refused(["states", "[1, 4096]"], c=con(utf8, states=0))
    refused(["states", "[1, 4096]"], c=con(utf8, states=4097))
    refused(["null table"], c=con(utf8, null=True))
    bad = utf8.copy()
    bad[5, 0x81] = 8
    refused(["next[5][129]", "0xFFFF"], c=con(bad))
    refused(["start_state[1]", "outside"], c=con(utf8), start=np.array([0, 8, 0], np.int32))
    dead = utf8.copy()
    dead[7, :] = sc.FORBID  # reached through F4 from state 0
    refused(["state 7", "no allowed byte"], c=con(dead))
    assert call(c=con(utf8), start=starts, end=True) == 0
    # a text the table rejects: the message names the stream and the offset
    with pytest.raises(lstm_hip.LstmHipError, match=r"score: stream 1: byte 0x80 at offset 2 is forbidden in state 0"):
        L.score([b"ab", b"ab\x80", b""], constraint=utf8)
    with pytest.raises(lstm_hip.LstmHipError, match=r"stream 2: byte 0x41 at offset 0 is forbidden in state 1"):
        L.score([b"ab", b"ab", b"A"], constraint=utf8, start_state=[0, 0, 1])
    with pytest.raises(lstm_hip.LstmHipError, match="without a constraint"):
        L.score([b"ab"], start_state=[0])
    losses = L.train_windows(3, 0.1)
    assert np.isfinite(losses).all()
    got = L.score([b"ab", "é".encode(), b""], first=True, top_n=1, constraint=utf8)  # and still scores
    assert 0x80 <= got["top_byte"][1][1, 0] <= 0xBF and list(got["end_state"]) == [0, 0, 0]
    L.close()


def test_non_finite_parameters_stay_in_range():
    N, lengths = 64, [12, 0, 5]
    texts = _texts(lengths, seed=95)
    P = sr.peaked_params(N, seed=96)
    good = _handle(N, P)
    want = good.score(texts, first=True, top_n=8)
    for poison in (np.nan, np.inf, -np.inf, 1e30):  # (1e30: expf overflows without the flag)
        for flags in (0, STABLE):
            bad = P.copy()
            bad[-256 - 40:-256:7] = poison  # a few entries of Why
            bad[-3] = poison                # and one of by
            L = _handle(N, bad, flags)
            got = L.score(texts, first=True, top_n=8)
            assert [a.shape for a in got["top_byte"]] == [(n, 8) for n in lengths] and got["bits"].shape == (3,)
            L.close()
    assert _same(good.score(texts, first=True, top_n=8), want)
    good.close()


def test_program_rows_and_closing_line(tmp_path):
    import lstm_hip
    rs = np.random.RandomState(101)
    words = ["één", "zwölf", "naïve", "abc", "xyz"]
    text = "".join(words[i] + " " for i in rs.randint(0, len(words), size=800)).encode()
    corpus = tmp_path / "corpus.txt"
    corpus.write_bytes(text)
    N = 64
    tr = subprocess.run([LSTM, str(corpus), str(N), "8", "4", "0.1", "--epochs", "1", "--windows", "30", "--sample", "0",
                         "--save", str(tmp_path / "ck"), "--quiet"], capture_output=True, text=True, errors="replace", timeout=300)
    assert tr.returncode == 0, tr.stderr
    piece = "zwölf abc één naïve xyz één abc zwölf ".encode()
    f = tmp_path / "t.txt"
    f.write_bytes(piece)
    data = np.frombuffer(piece, np.uint8)
    P = np.concatenate([np.loadtxt(tmp_path / f"ck_{k}.txt", ndmin=2).astype(np.float32).flatten(order="F")
                        for k in ("W", "U", "b", "Why", "by")])
    L = _handle(N, P, lstm_hip.PAD_HIDDEN)
    for extra, kw in (([], dict()), (["--top", "3"], dict(top_n=3)), (["--top", "2", "--utf8"], dict(top_n=2, first=True, constraint=lstm_hip.dfa_utf8()))):
        out = subprocess.run([GEN, "--load", str(tmp_path / "ck"), "--score-bytes", str(f)] + extra, capture_output=True, text=True,
                             errors="replace", timeout=300)
        assert out.returncode == 0, out.stderr
        want = L.score([data], **kw)
        lines = out.stdout.splitlines()
        assert len(lines) == data.size + 1
        top = kw.get("top_n", 0)
        for j, line in enumerate(lines[:-1]):
            cells = line.split("\t")
            assert len(cells) == 5 + 2 * top, line
            assert int(cells[0]) == j and int(cells[1], 16) == data[j] and int(cells[4]) == want["rank"][0][j], line
            assert abs(float(cells[2]) - want["surprisal"][0][j]) <= 1e-5 and abs(float(cells[3]) - want["entropy"][0][j]) <= 1e-5, line
            for r in range(top):
                assert int(cells[5 + 2 * r], 16) == want["top_byte"][0][j, r], line
                assert abs(float(cells[6 + 2 * r]) - want["top_bits"][0][j, r]) <= 1e-5, line
        scored = data.size if kw.get("first") else data.size - 1
        assert lines[-1] == f"{f}: {want['bits'][0] / scored:.5f} bits/char ({data.size} bytes)", lines[-1]
        if not extra:  # ... which is the --score line of the file
            ref = subprocess.run([GEN, "--load", str(tmp_path / "ck"), "--score", str(f)], capture_output=True, text=True, timeout=300)
            assert ref.returncode == 0 and ref.stdout.splitlines()[0] == lines[-1], ref.stdout
    L.close()
    bad = tmp_path / "bad.txt"
    bad.write_bytes(b"ab\xffcd")
    r = subprocess.run([GEN, "--load", str(tmp_path / "ck"), "--score-bytes", str(bad), "--utf8"], capture_output=True, timeout=300)
    assert r.returncode == 1 and b"stream 0: byte 0xff at offset 2 is forbidden in state 0" in r.stderr, r.stderr
