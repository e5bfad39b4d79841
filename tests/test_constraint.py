"""-m gpu: lstm_hip_generate_constrained -- generation under a byte automaton (include/lstm_hip.h).

Without a table the call is lstm_hip_generate_ex bit for bit; an all-allowed table leaves greedy decoding as it is; a table
with one allowed byte per state forces its text whatever the draws; under the UTF-8 automaton every output walks the table
and decodes strictly; against the oracle every drawn byte lies in the float64 reference's kept set of the masked
distribution (tests/constraint_ref.py), with the thresholds of test_filtered_draws_against_the_oracle; wide batches, chained
calls, the stop byte, the handle kinds and the refusals behave as the contract says."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import constraint_ref as cr
import sampling_ref as sr
from test_pad_hidden import pad_cols, pad_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 256
FILTERS = dict(top_k=40, top_p=0.9, temperature=0.8)
LSTM = os.path.join(ROOT, "eigen-lstm_amd", "lstm")
GEN = os.path.join(ROOT, "eigen-lstm_amd", "lstm_generate")


def _state(streams, N, seed):
    rs = np.random.RandomState(seed)
    return (rs.randn(streams, N) * 0.1).astype(np.float32), (rs.randn(streams, N) * 0.1).astype(np.float32)


def _prompts(lengths, seed):
    rs = np.random.RandomState(seed)
    return [rs.randint(32, 127, size=n).astype(np.uint8) for n in lengths]  # (ASCII: the UTF-8 table stays in state 0)


def _same(a, b):
    """the first four results (out, bits, h, c) agree bit for bit"""
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a[:4], b[:4]))


def _same_info(a, b):
    return _same(a, b) and all(np.array_equal(a[4][k], b[4][k]) for k in ("out_len", "kept", "end_state"))


def _utf8_starts(rs, K):
    """mixed start states of the UTF-8 table, every state present"""
    q = rs.randint(0, 8, size=K).astype(np.int32)
    q[:8] = np.arange(8)
    return q


def _raw_constrained(L, streams, opt, u, count, con, start, want_end, N):
    """lstm_hip_generate_constrained itself, without prompts or start state: (rc, out, h, c, out_len, kept, end_state)"""
    import lstm_hip
    out = np.zeros((count, streams), np.uint8)
    h, c = np.empty((streams, N), np.float32), np.empty((streams, N), np.float32)
    out_len, kept = np.zeros(streams, np.int32), np.zeros((count, streams), np.uint16)
    end = np.full(streams, -9, np.int32)
    p = lstm_hip._ptr
    rc = L.lib.lstm_hip_generate_constrained(
        L._h, C.c_int32(streams), None, None, None, None, opt, p(u, C.c_double) if u is not None else None, C.c_int32(count),
        p(out, C.c_uint8), None, p(h), p(c), p(out_len, C.c_int32), p(kept, C.c_uint16), con,
        p(start, C.c_int32) if start is not None else None, p(end, C.c_int32) if want_end else None)
    return rc, out, h, c, out_len, kept, end


@pytest.mark.parametrize("flags", [0, 512])  # 512: LSTM_HIP_STABLE_SOFTMAX
def test_no_constraint_is_generate_ex(flags):
    import lstm_hip
    N, K, Cn = 128, 7, 60
    P = sr.peaked_params(N, seed=3, scale=0.1)
    prompts = _prompts([0, 1, 2, 9, 40, 130, 5], seed=4)
    h0, c0 = _state(K, N, seed=5)
    u = np.random.RandomState(6).random_sample((Cn, K))
    L = lstm_hip.Lstm(N, 2, 1, flags=flags)
    L.set_params(P)
    data, off = lstm_hip._offsets(prompts)
    p = lstm_hip._ptr
    for tau in (1.0, 0.7, 0.0):
        for kw in (dict(), dict(top_k=40, top_p=0.9, stop_byte=101)):
            ex = L.generate(prompts, count=Cn, u=u, temperature=tau, h0=h0, c0=c0, score=True, info=True, **kw)
            assert _same(ex, L.generate(prompts, count=Cn, u=u, temperature=tau, h0=h0, c0=c0, score=True, constraint=None, **kw))
            opt = lstm_hip._Sampling(C.sizeof(lstm_hip._Sampling), tau, kw.get("top_k", 0), kw.get("top_p", 1.0), kw.get("stop_byte", -1))
            out = np.zeros((Cn, K), np.uint8)
            bits = np.zeros(K)
            h, c = np.empty((K, N), np.float32), np.empty((K, N), np.float32)
            out_len, kept = np.zeros(K, np.int32), np.zeros((Cn, K), np.uint16)
            rc = L.lib.lstm_hip_generate_constrained(
                L._h, C.c_int32(K), p(data, C.c_uint8), p(off, C.c_uint64), p(h0), p(c0), C.byref(opt), p(u, C.c_double),
                C.c_int32(Cn), p(out, C.c_uint8), p(bits, C.c_double), p(h), p(c), p(out_len, C.c_int32), p(kept, C.c_uint16),
                None, None, None)
            assert rc == 0, L.lib.lstm_hip_last_error()
            assert _same(ex, (out, bits, h, c)), (tau, kw)
            assert np.array_equal(ex[4]["out_len"], out_len) and np.array_equal(ex[4]["kept"], kept), (tau, kw)
    L.close()


def test_all_allowed_table_leaves_greedy_decoding_as_it_is():
    import lstm_hip
    N, K, Cn = 128, 9, 100
    P = sr.peaked_params(N, seed=11, scale=0.1)
    prompts = _prompts([3, 0, 17, 40, 1, 9, 2, 2, 60], seed=12)
    h0, c0 = _state(K, N, seed=13)
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(P)
    free = L.generate(prompts, count=Cn, temperature=0.0, h0=h0, c0=c0, score=True)
    got = L.generate(prompts, count=Cn, temperature=0.0, h0=h0, c0=c0, score=True, info=True, constraint=np.zeros((1, 256), np.uint16))
    assert _same(free, got)
    assert (got[4]["kept"] == 1).all() and (got[4]["end_state"] == 0).all() and (got[4]["out_len"] == Cn).all()
    # a tempered draw under the all-allowed table is a filtered draw that keeps everything
    u = np.random.RandomState(14).random_sample((Cn, K))
    warm = L.generate(prompts, count=Cn, u=u, temperature=0.8, h0=h0, c0=c0, info=True, constraint=np.zeros((1, 256), np.uint16))
    assert (warm[4]["kept"] == 256).all()
    L.close()


@pytest.mark.parametrize("N,flags,K", [(128, 0, 5), (100, 256, 5), (32, 0, 1030)])  # 256: LSTM_HIP_PAD_HIDDEN
def test_a_cycle_table_forces_its_text(N, flags, K):
    import lstm_hip
    text = np.frombuffer("één cyclus: ∮ 🙂.\n".encode(), np.uint8)
    T, Cn = text.size, 45  # (more than one turn of the cycle)
    table = np.full((T, 256), cr.FORBID, np.uint16)
    table[np.arange(T), text] = (np.arange(T) + 1) % T
    rs = np.random.RandomState(N + K)
    start = rs.randint(0, T, size=K).astype(np.int32)
    start[:3] = (0, T - 1, 7)
    lengths = rs.randint(0, 6, size=K)
    lengths[:2] = (0, 5)
    enter = (start - lengths) % T  # the prompt is the piece of the cycle before the stream's first draw
    prompts = [text[(enter[s] + np.arange(lengths[s])) % T] for s in range(K)]
    want = np.stack([text[(start[s] + np.arange(Cn)) % T] for s in range(K)], axis=1)
    P = sr.peaked_params(N, seed=21, scale=0.1)
    h0, c0 = _state(K, N, seed=22)
    u = rs.random_sample((Cn, K))
    L = lstm_hip.Lstm(N, 2, 1, flags=flags)
    L.set_params(P)
    ref = L.generate([np.concatenate([prompts[s], want[:, s]]) for s in range(K)], count=0, h0=h0, c0=c0)
    for kw in (dict(temperature=1.0), dict(temperature=0.0), dict(FILTERS), dict(temperature=1.7, top_k=3)):
        got = L.generate(prompts, count=Cn, u=u, h0=h0, c0=c0, info=True, constraint=table, start_state=enter, **kw)
        assert np.array_equal(got[0], want), kw
        assert (got[4]["kept"] == 1).all(), kw
        assert np.array_equal(got[4]["end_state"], (start + Cn) % T), kw
        assert np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3]), kw
    L.close()


def _cut(prompt, out, end_state, table):
    """prompt + output, cut back to the last character boundary when the stream ended inside a character"""
    data = bytes(prompt) + bytes(out)
    if end_state == 0:
        return data
    q, n = 0, 0
    for i, b in enumerate(data):
        q = int(table[q, b])
        if q == 0:
            n = i + 1
    return data[:n]


@pytest.mark.parametrize("top_k,top_p,tau", cr.ORACLE_SETTINGS)
def test_utf8_outputs_are_valid_and_match_the_oracle(top_k, top_p, tau, oracle32):
    """The eight-stream case (one stream per state of the UTF-8 automaton).  Validity: every stream's output walks the
    table from its post-prompt state to end_state, and prompt + output decodes strictly up to the last boundary.  Oracle
    comparison, as test_filtered_draws_against_the_oracle: the drawn bytes are fed back through the oracle, the float64
    reference masks, renormalises and filters each step's distribution; ambiguous draws (their share on oracle trajectories
    is what tests/test_constraint_cpu.py controls) are skipped, at most 5 % of them."""
    import lstm_hip
    table = lstm_hip.dfa_utf8()
    N, K, Cn = sr.ORACLE_N, cr.ORACLE_STREAMS, sr.ORACLE_COUNT
    P, prompts, u = cr.oracle_case()
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(P)
    out, _, _, _, info = L.generate(prompts, count=Cn, u=u, temperature=tau, top_k=top_k, top_p=top_p, info=True, constraint=table)
    L.close()
    kept = info["kept"]
    skipped = checked = inside = near = 0
    keeps, drawing = [], set()
    for s in range(K):
        q = cr.walk(table, 0, prompts[s])
        assert q == s
        assert cr.walk(table, q, out[:, s]) == info["end_state"][s], s
        _cut(prompts[s], out[:, s], info["end_state"][s], table).decode("utf-8", "strict")
        p1 = sr.replay(oracle32, N, P, prompts[s], out[:, s])
        for i in range(Cn):
            drawing.add(q)
            x = int(out[i, s])
            keep, mask, pp, p = cr.filter64(p1[i], table, q, tau, top_k, top_p)
            assert 1 <= int(kept[i, s]) <= cr.counts(table)[q]
            if cr.ambiguous(p, table, q, top_k, top_p):
                skipped += 1
            else:
                assert mask[x], (s, i, x, keep)
                assert int(kept[i, s]) == keep, (s, i, int(kept[i, s]), keep)
                keeps.append(keep)
                lo = pp[:x].sum()
                hi = lo + pp[x]
                checked += 1
                inside += lo <= u[i, s] < hi
                near += lo - 1e-5 <= u[i, s] < hi + 1e-5
            q = int(table[q, x])
    print(f"top_k {top_k} top_p {top_p} tau {tau}: skipped {skipped}, checked {checked}, inside {inside}, near {near}, "
          f"mean kept {np.mean(keeps):.2f}, drawing states {sorted(drawing)}")
    assert skipped <= 0.05 * K * Cn, skipped
    assert inside >= 0.99 * checked and near == checked, (inside, near, checked)
    assert drawing == set(range(8))


@pytest.mark.parametrize("tau", [1.0, 0.7])
def test_top_k_one_is_constrained_greedy(tau):
    import lstm_hip
    table = lstm_hip.dfa_restrict(lstm_hip.dfa_utf8(), np.r_[np.zeros(97), np.ones(26), np.zeros(5), np.ones(128)])  # a-z and non-ASCII
    N, K, Cn = 128, 9, 120
    P = sr.peaked_params(N, seed=31, scale=0.1)
    prompts = _prompts([3, 0, 17, 40, 1, 9, 2, 2, 60], seed=32)
    prompts = [np.clip(p, 97, 122) for p in prompts]
    h0, c0 = _state(K, N, seed=33)
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(P)
    greedy = L.generate(prompts, count=Cn, temperature=0.0, h0=h0, c0=c0, info=True, constraint=table)
    free = L.generate(prompts, count=Cn, temperature=0.0, h0=h0, c0=c0)
    assert not np.array_equal(free[0], greedy[0])  # the table changes the greedy text (a property of the seed)
    for s in range(K):
        assert cr.walk(table, 0, greedy[0][:, s]) == greedy[4]["end_state"][s]
    u = np.random.RandomState(34).random_sample((Cn, K))
    got = L.generate(prompts, count=Cn, u=u, temperature=tau, h0=h0, c0=c0, top_k=1, info=True, constraint=table)
    assert _same_info(got, greedy)
    L.close()


@pytest.mark.parametrize("K,kw", [(1024, dict()), (4096, FILTERS)])
def test_constrained_wide_batches_match_small_batches(K, kw):
    """gen_head puts 4 (1024 streams) and 16 (4096) streams into one workgroup: under the table every stream must come out
    as it does in a batch of 8 (one stream per workgroup) -- bytes, kept counts, final and end states."""
    import lstm_hip
    table = lstm_hip.dfa_utf8()
    N, Cn = 64, 24
    rs = np.random.RandomState(K)
    P = sr.peaked_params(N, seed=41)
    start = _utf8_starts(rs, K)
    h0, c0 = _state(K, N, seed=K + 2)
    u = rs.random_sample((Cn, K))
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(P)
    wide = L.generate(count=Cn, u=u, h0=h0, c0=c0, info=True, constraint=table, start_state=start, **kw)
    # every stream's bytes walk the table from its start state to its end state, and no draw keeps more than its state allows
    dead = np.vstack([table, np.full((1, 256), 8, np.uint16)])
    dead[dead == cr.FORBID] = 8  # (a rejected walk stays in row 8)
    q = start.astype(np.int64)
    for i in range(Cn):
        assert (wide[4]["kept"][i] <= cr.counts(table)[q]).all() and (wide[4]["kept"][i] >= 1).all(), i
        q = dead[q, wide[0][i]].astype(np.int64)
        assert (q < 8).all(), i
    assert np.array_equal(q, wide[4]["end_state"])
    if not kw:  # the table alone at temperature 1: a draw keeps exactly what its state allows
        assert np.array_equal(wide[4]["kept"][0], cr.counts(table)[start])
    if K == 1024:
        groups = [np.arange(g, g + 8) for g in range(0, K, 8)]  # all of them
    else:  # the first and the last two workgroups' streams in every position, and a few more
        pick = np.unique(np.concatenate([np.arange(32), np.arange(K - 32, K), rs.choice(K, 16, replace=False)]))
        groups = [pick[g:g + 8] for g in range(0, pick.size, 8)]
    for g in groups:
        small = L.generate(count=Cn, u=u[:, g], h0=h0[g], c0=c0[g], info=True, constraint=table, start_state=start[g], **kw)
        assert np.array_equal(wide[0][:, g], small[0]), g
        assert np.array_equal(wide[2][g], small[2]) and np.array_equal(wide[3][g], small[3]), g
        assert np.array_equal(wide[4]["kept"][:, g], small[4]["kept"]), g
        assert np.array_equal(wide[4]["end_state"][g], small[4]["end_state"]), g
    L.close()


def test_chained_calls_are_the_long_call():
    import lstm_hip
    table = lstm_hip.dfa_utf8()
    N, K, Cn = 64, 8, 80
    P, prompts, _ = cr.oracle_case()
    u = np.random.RandomState(51).random_sample((Cn, K))
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(P)
    for kw in (dict(), dict(FILTERS)):
        whole = L.generate(prompts, count=Cn, u=u, info=True, constraint=table, **kw)
        # split where some stream stands inside a character, if the run has such a place (else in the middle)
        inside = [n for n in range(20, 61) if any(cr.walk(table, s, whole[0][:n, s]) != 0 for s in range(K))]
        n = inside[0] if inside else 40
        a = L.generate(prompts, count=n, u=u[:n], info=True, constraint=table, **kw)
        b = L.generate(count=Cn - n, u=u[n:], h0=a[2], c0=a[3], info=True, constraint=table, start_state=a[4]["end_state"], **kw)
        assert np.array_equal(np.concatenate([a[0], b[0]]), whole[0])
        assert np.array_equal(np.concatenate([a[4]["kept"], b[4]["kept"]]), whole[4]["kept"])
        assert np.array_equal(b[2], whole[2]) and np.array_equal(b[3], whole[3])
        assert np.array_equal(b[4]["end_state"], whole[4]["end_state"])
        assert list(a[4]["end_state"]) == [cr.walk(table, s, whole[0][:n, s]) for s in range(K)]
        # count 0: end_state is the state after the prompt
        none = L.generate(prompts, count=0, info=True, constraint=table, **kw)
        assert list(none[4]["end_state"]) == list(range(8))
    L.close()


def test_stop_byte_under_a_constraint():
    import lstm_hip
    table = lstm_hip.dfa_utf8()
    N, K, Cn = 64, 24, 120
    P = sr.peaked_params(N, seed=61)
    prompts = _prompts([0, 1, 5, 30] * (K // 4), seed=62)
    h0, c0 = _state(K, N, seed=63)
    u = np.random.RandomState(64).random_sample((Cn, K))
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(P)
    for kw in (dict(), dict(FILTERS)):
        run = lambda **extra: L.generate(prompts, count=Cn, u=u, h0=h0, c0=c0, score=True, info=True, constraint=table, **kw, **extra)
        full = run()
        stop = int(np.bincount(full[0][:Cn // 2].ravel(), minlength=256).argmax())  # a byte many streams draw early
        cut = run(stop_byte=stop)
        stopped = 0
        for s in range(K):
            where = np.nonzero(full[0][:, s] == stop)[0]
            n = int(where[0]) + 1 if where.size else Cn
            stopped += n < Cn
            assert cut[4]["out_len"][s] == n, s
            assert np.array_equal(cut[0][:n, s], full[0][:n, s]) and not cut[0][n:, s].any(), s
            assert np.array_equal(cut[4]["kept"][:n, s], full[4]["kept"][:n, s]) and not cut[4]["kept"][n:, s].any(), s
            assert cut[4]["end_state"][s] == cr.walk(table, 0, cut[0][:n, s]), s  # the state after the stop byte
        assert stopped >= 1  # (the stop byte was drawn in the first half of some stream's run)
        assert np.array_equal(cut[1], full[1])  # the prompts' bits
        # a forbidden stop byte never comes (0xC0 and 0xFF are never well-formed; 0x80 is forbidden at a boundary only)
        for forbidden in (0xC0, 0xFF):
            assert _same_info(run(stop_byte=forbidden), full)
    # the prompts' bits ignore the constraint
    plain = L.generate(prompts, count=Cn, u=u, h0=h0, c0=c0, score=True)
    assert np.array_equal(plain[1], full[1])
    L.close()


def test_bf16_padded_and_step_kernel_handles_match_their_twins():
    import lstm_hip
    table = lstm_hip.dfa_utf8()
    K, Cn = 5, 80
    u = np.random.RandomState(71).random_sample((Cn, K))
    prompts = _prompts([0, 4, 60, 1, 200], seed=72)
    start = np.array([0, 0, 0, 0, 0], np.int32)
    kw = dict(count=Cn, u=u, score=True, info=True, stop_byte=101, constraint=table, start_state=start, **FILTERS)
    for twin in (lstm_hip.BF16_RECURRENCE, lstm_hip.STEP_KERNELS):  # the generator runs on the fp32 master weights
        N = 256 if twin == lstm_hip.BF16_RECURRENCE else 64
        P = sr.peaked_params(N, seed=73, scale=0.1)
        h0, c0 = _state(K, N, seed=74)
        res = []
        for flags in (0, twin):
            L = lstm_hip.Lstm(N, 2, 8, flags=flags)
            L.set_params(P)
            res.append(L.generate(prompts, h0=h0, c0=c0, **kw))
            L.close()
        assert _same_info(*res)
        assert res[0][4]["kept"].max() <= 40  # (top_k)
    # N = 500 padded to 512 against an explicit 512 handle with zero-padded parameters and state
    N, Np = 500, 512
    P = sr.peaked_params(N, seed=75, scale=0.1)
    h0, c0 = _state(K, N, seed=76)
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
    assert all(np.array_equal(ra[4][k], rb[4][k]) for k in ("out_len", "kept", "end_state"))


def _trainer(text, N, S, B):
    import lstm_hip
    L = lstm_hip.Lstm(N, S, B)
    L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(5), N))
    L.set_text(text)
    L.set_cursors(lstm_hip.initial_cursors(text.size, S, B))
    return L


def test_training_state_is_untouched_by_constrained_generation():
    import lstm_hip
    N, S, B = 64, 8, 4
    text = np.random.RandomState(81).randint(97, 123, size=5000).astype(np.uint8)
    A, Bh = _trainer(text, N, S, B), _trainer(text, N, S, B)
    la = [A.train_windows(5, 0.1)]
    got = A.generate(_prompts([3, 40], seed=82), count=50, u=np.random.RandomState(83).random_sample((50, 2)), score=True,
                     stop_byte=104, info=True, constraint=lstm_hip.dfa_utf8(), **FILTERS)
    assert got[0].shape == (50, 2)
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
    lib = L.lib
    K, Cn = 3, 4
    u = np.random.RandomState(92).random_sample((Cn, K))
    utf8 = lstm_hip.dfa_utf8()
    size = C.sizeof(lstm_hip._Constraint)
    opt = lstm_hip._Sampling(C.sizeof(lstm_hip._Sampling), 1.0, 0, 1.0, -1)

    def con(table, states=None, sz=size, null=False):
        table = np.ascontiguousarray(table, np.uint16)
        c = lstm_hip._Constraint(sz, table.shape[0] if states is None else states, None if null else lstm_hip._ptr(table, C.c_uint16))
        c._keep = table
        return C.byref(c)

    def refused(words, c, start=None, want_end=True, o=opt):
        rc = _raw_constrained(L, K, C.byref(o) if o is not None else None, u, Cn, c, start, want_end, N)[0]
        msg = lib.lstm_hip_last_error().decode()
        assert rc == lstm_hip.EINVAL, (words, rc)
        assert msg.startswith("generate:") and all(w in msg for w in words), (words, msg)

    starts = np.zeros(K, np.int32)
    refused(["start_state", "without a constraint"], None, start=starts, want_end=False)
    refused(["end_state", "without a constraint"], None, want_end=True)
    refused(["constraint of", "bytes"], con(utf8, sz=size - 4))
    refused(["constraint of", "bytes"], con(utf8, sz=0))
    refused(["states", "[1, 4096]"], con(utf8, states=0))
    refused(["states", "[1, 4096]"], con(utf8, states=4097))
    refused(["null table"], con(utf8, null=True))
    bad = utf8.copy()
    bad[5, 0x81] = 8
    refused(["next[5][129]", "0xFFFF"], con(bad))
    refused(["start_state[1]", "outside"], con(utf8), start=np.array([0, 8, 0], np.int32))
    refused(["start_state[2]", "outside"], con(utf8), start=np.array([0, 1, -1], np.int32))
    dead = utf8.copy()
    dead[7, :] = cr.FORBID  # reached through F4 from state 0
    refused(["state 7", "no allowed byte"], con(dead))
    refused(["top_k"], con(utf8), o=lstm_hip._Sampling(C.sizeof(lstm_hip._Sampling), 1.0, 300, 1.0, -1))  # what generate_ex refuses
    refused(["null sampling options"], con(utf8), o=None)
    # an unreachable empty row is no fault: without F4 nothing leads to state 7
    unreachable = dead.copy()
    unreachable[0, 0xF4] = cr.FORBID
    got = L.generate(count=Cn, u=u, info=True, constraint=unreachable)
    assert got[0].shape == (Cn, K)
    # ... until a stream starts there
    with pytest.raises(lstm_hip.LstmHipError, match="state 7"):
        L.generate(count=Cn, u=u, constraint=unreachable, start_state=[0, 7, 0])
    # a prompt byte the table rejects: the message names the stream and the offset
    with pytest.raises(lstm_hip.LstmHipError, match=r"generate: stream 1: prompt byte 0x80 at offset 2 is forbidden in state 0"):
        L.generate([b"ab", b"ab\x80", b""], count=Cn, u=u, constraint=utf8)
    with pytest.raises(lstm_hip.LstmHipError, match=r"stream 2: prompt byte 0x41 at offset 0 is forbidden in state 1"):
        L.generate([b"ab", b"ab", b"A"], count=Cn, u=u, constraint=utf8, start_state=[0, 0, 1])
    with pytest.raises(lstm_hip.LstmHipError, match="without a constraint"):
        L.generate(count=Cn, u=u, start_state=[0, 0, 0])
    losses = L.train_windows(3, 0.1)
    assert np.isfinite(losses).all()
    got = L.generate([b"ab", "é".encode()[:1], b""], count=10, u=np.random.RandomState(93).random_sample((10, K)), info=True,
                     constraint=utf8)  # and still generates
    assert got[0].shape == (10, K) and 0x80 <= got[0][0, 1] <= 0xBF
    L.close()


def test_program_utf8_allow_and_a_bad_prime(tmp_path):
    rs = np.random.RandomState(101)
    words = ["één", "zwölf", "naïve", "日本", "🙂", "abc", "xyz"]
    text = "".join(words[i] + ("\n" if rs.rand() < 0.3 else " ") for i in rs.randint(0, len(words), size=1500)).encode()
    corpus = tmp_path / "corpus.txt"
    corpus.write_bytes(text)
    tr = subprocess.run([LSTM, str(corpus), "64", "8", "4", "0.1", "--epochs", "1", "--windows", "100", "--sample", "0",
                         "--save", str(tmp_path / "ck"), "--quiet"], capture_output=True, text=True, errors="replace", timeout=300)
    assert tr.returncode == 0, tr.stderr
    run = lambda *extra: subprocess.run([GEN, "--load", str(tmp_path / "ck"), "--count", "150", "--streams", "4", "--seed", "3",
                                         *extra], capture_output=True, timeout=300)

    def samples(blob):
        parts = blob.split(b"== sample ")[1:]
        return [p.split(b" ==\n", 1)[1][:-1] for p in parts]  # (the program ends every sample with a newline of its own)

    # at temperature 2 a barely trained model draws malformed text; under --utf8 it cannot
    free, utf8 = run("--temperature", "2", "--prime", "é"), run("--temperature", "2", "--utf8", "--prime", "é")
    assert free.returncode == 0 and utf8.returncode == 0, (free.stderr, utf8.stderr)
    bad = 0
    for s in samples(free.stdout):
        try:
            s.decode("utf-8", "strict")
        except UnicodeDecodeError:
            bad += 1
    print(f"unconstrained samples that do not decode: {bad} of 4")  # (what --utf8 has to prevent; not asserted: the model decides)
    got = samples(utf8.stdout)
    assert len(got) == 4
    for s in got:
        assert s.decode("utf-8", "strict").startswith("é") and len(s) > 100
    only = run("--temperature", "2", "--allow", "0x61-0x7a,0x20")
    assert only.returncode == 0, only.stderr
    for s in samples(only.stdout):
        assert len(s) == 150 and set(s) <= set(range(0x61, 0x7B)) | {0x20}, s
    ban = run("--temperature", "2", "--utf8", "--ban", "0x80-0xff")
    assert ban.returncode == 0, ban.stderr
    for s in samples(ban.stdout):
        assert len(s) == 150 and max(s) < 0x80
    prime = tmp_path / "prime.bin"
    prime.write_bytes(b"ab\xc3")
    ok = run("--utf8", "--prime-file", str(prime))  # ends inside a character: the first draw completes it
    assert ok.returncode == 0, ok.stderr
    for s in samples(ok.stdout):
        s.decode("utf-8", "strict")
    prime.write_bytes(b"ab\xffcd")
    r = run("--utf8", "--prime-file", str(prime))
    assert r.returncode == 1 and b"prompt byte 0xff at offset 2 is forbidden in state 0" in r.stderr, r.stderr
