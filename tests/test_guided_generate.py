"""-m gpu: lstm_hip_generate_guided -- a log-linear mix of the logits of models fed the same bytes, in the batched generator
(include/lstm_hip.h).

With the block NULL the call is lstm_hip_generate_processed byte for byte; weights (1, 0) are the main model's own processed
call and (0, 1) the guide handle's; a model as its own guide with (2, -1) from the same start state is the unguided call; at
N = 16 with guides at N = 32 and N = 40 (padded) the bytes, kept counts, lengths and end states are those of the float32
reference (tests/guided_ref.py) on the device's own states; against the oracle every drawn byte lies in the float64 kept set of
the mixed distribution; a call in two pieces with every model's state handed over is the one long call; and neither the main
handle nor a guide is changed by a guided call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import constraint_ref as cr
import deadline_ref as dr
import guided_ref as gr
import logit_processor_ref as lr
import sampling_ref as sr
from logits_ref import logits32 as _logits32
from oracle_lib import split_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 256
f32 = np.float32
N, GN, K, Cn = 16, (32, 40), 20, 14
NAMES = ("out", "bits", "h", "c", "out_len", "kept", "end_state")


def _state(streams, n, seed):
    rs = np.random.RandomState(seed)
    return (rs.randn(streams, n) * 0.1).astype(f32), (rs.randn(streams, n) * 0.1).astype(f32)


def _same(a, b, names=NAMES):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]) for k in names)


def _group_rule():
    """gen_head_group of kernels.hip as a Python function of (N, streams), read from its text (as tests/test_logit_processors.py)"""
    text = open(os.path.join(ROOT, "eigen-lstm_amd", "csrc", "kernels.hip")).read()
    m = re.search(r"int gen_head_group\(int N, int streams\) \{\s*int sb = 1;[^\n]*\n\s*while \((.*?)\) sb \*= 2;\s*return sb;", text)
    assert m, "gen_head_group has changed its shape"
    cond = m.group(1).replace("(size_t)", "").replace("&&", " and ")
    assert re.fullmatch(r"[\w\s<>=*()]+", cond), cond

    def group(n, streams):
        sb = 1
        while eval(cond, {}, dict(sb=sb, N=n, streams=streams)):
            sb *= 2
        return sb
    return group


def _handle(n, P, flags=0, S=2, B=1):
    import lstm_hip
    L = lstm_hip.Lstm(n, S, B, flags=flags)
    L.set_params(P)
    return L


@pytest.fixture(scope="module")
def models():
    """the main model at N = 16, guides at N = 32 and at N = 40 padded: (handle, parameters) each"""
    import lstm_hip
    Ps = [sr.peaked_params(N, seed=7, gain=6.0), sr.peaked_params(GN[0], seed=8, gain=6.0), sr.peaked_params(GN[1], seed=9, gain=6.0)]
    hs = [_handle(N, Ps[0]), _handle(GN[0], Ps[1]), _handle(GN[1], Ps[2], lstm_hip.PAD_HIDDEN)]
    yield list(zip(hs, Ps))
    for h in hs:
        h.close()


def _prompts(K, rs, table=None, F=None, count=0):
    """prompts of (3 s) % 5 letters (so empty ones occur) that the table takes"""
    prompts = []
    for s in range(K):
        q, p = 0, []
        for _ in range((3 * s) % 5):
            good = [b for b in range(97, 123) if table is None or (table[q, b] != cr.FORBID and (F is None or F[count][table[q, b]]))]
            b = int(rs.choice(good))
            p.append(b)
            q = int(table[q, b]) if table is not None else 0
        prompts.append(np.array(p, np.uint8))
    return prompts


def _raw(L, fn, prompts, count, u, temperature, h0, c0, table=None, accept=None, top_k=0, top_p=1.0, stop_byte=-1, bias=None):
    """lstm_hip_generate_processed (fn = "processed") or lstm_hip_generate_guided with gd NULL, through ctypes: the seven results"""
    import lstm_hip
    p = lstm_hip._ptr
    Kn, n = len(prompts), L.N
    data, off = lstm_hip._offsets(lstm_hip._bytes_list(prompts))
    opt = lstm_hip._Sampling(C.sizeof(lstm_hip._Sampling), temperature, top_k, top_p, stop_byte)
    out, bits = np.zeros((count, Kn), np.uint8), np.zeros(Kn)
    h, c = np.empty((Kn, n), f32), np.empty((Kn, n), f32)
    out_len, kept, end = np.zeros(Kn, np.int32), np.zeros((count, Kn), np.uint16), np.zeros(Kn, np.int32)
    bc = None
    if table is not None:
        t = np.ascontiguousarray(table, np.uint16)
        con = lstm_hip._Constraint(C.sizeof(lstm_hip._Constraint), t.shape[0], p(t, C.c_uint16))
        acc = None if accept is None else np.ascontiguousarray(accept, np.uint8)
        bc = lstm_hip._BeamConstraint(C.sizeof(lstm_hip._BeamConstraint), C.pointer(con), p(acc, C.c_uint8) if acc is not None else None)
    lp = lstm_hip._LogitProcessors(C.sizeof(lstm_hip._LogitProcessors), p(bias) if bias is not None else None, 0.0, 0, None, None)
    args = [L._h, C.c_int32(Kn), p(data, C.c_uint8), p(off, C.c_uint64), p(h0), p(c0), C.byref(opt), p(u, C.c_double),
            C.c_int32(count), p(out, C.c_uint8), p(bits, C.c_double), p(h), p(c), p(out_len, C.c_int32), p(kept, C.c_uint16),
            C.byref(bc) if bc is not None else None, None, p(end, C.c_int32) if bc is not None else None, C.byref(lp)]
    rc = L.lib.lstm_hip_generate_processed(*args) if fn == "processed" else L.lib.lstm_hip_generate_guided(*args, None)
    assert rc == 0, L.lib.lstm_hip_last_error()
    return dict(zip(NAMES, (out, bits, h, c, out_len, kept, end if bc is not None else None)))


@pytest.mark.parametrize("which", ["plain", "table", "accepting"])
def test_a_null_block_is_the_processed_call(models, which):
    import lstm_hip
    L = models[0][0]
    rs = np.random.RandomState(4)
    table = accept = None
    stop = -1
    if which == "table":
        table = lstm_hip.dfa_utf8()
    if which == "accepting":
        table, accept = lstm_hip.dfa_regex(b"[a-z ]*", stop_byte=10)
        stop = 10
    prompts = _prompts(K, rs)
    h0, c0 = _state(K, N, seed=5)
    u = rs.random_sample((Cn, K))
    bias = (rs.randn(M) * 0.5).astype(f32)
    for tau in (1.0, 0.7, 0.0):
        for b in (None, bias):
            run = lambda fn: _raw(L, fn, prompts, Cn, u, tau, h0, c0, table, accept, top_k=40, top_p=0.9, stop_byte=stop, bias=b)
            assert _same(run("processed"), run("guided")), (which, tau, b is None)


def test_weights_1_0_are_the_main_models_processed_call(models):
    (L, _), (G, _), _ = models
    rs = np.random.RandomState(11)
    prompts = _prompts(K, rs)
    h0, c0 = _state(K, N, seed=12)
    gh0, gc0 = _state(K, GN[0], seed=13)
    u = rs.random_sample((Cn, K))
    for kw in (dict(temperature=0.8, top_k=40, top_p=0.9), dict(temperature=0.0), dict(temperature=1.0, stop_byte=101)):
        want = L.generate(prompts, count=Cn, u=u, h0=h0, c0=c0, score=True, info=True, logit_bias=np.zeros(M, f32), **kw)
        got = L.generate(prompts, count=Cn, u=u, h0=h0, c0=c0, score=True, info=True, guides=[(G, 0.0, gh0, gc0)], main_weight=1.0, **kw)
        for i in range(4):
            assert np.array_equal(want[i], got[i]), (kw, i)
        assert np.array_equal(want[4]["kept"], got[4]["kept"]) and np.array_equal(want[4]["out_len"], got[4]["out_len"]), kw


def test_weights_0_1_are_the_guides_own_call(models):
    (L, _), (G, _), (G2, _) = models
    rs = np.random.RandomState(21)
    prompts = _prompts(K, rs)
    h0, c0 = _state(K, N, seed=22)
    for guide, n, stop in ((G, GN[0], 101), (G2, GN[1], None), (G, GN[0], None)):
        gh0, gc0 = _state(K, n, seed=23)
        u = rs.random_sample((Cn, K))
        kw = dict(temperature=0.9, top_k=50, stop_byte=stop)
        want = guide.generate(prompts, count=Cn, u=u, h0=gh0, c0=gc0, info=True, logit_bias=np.zeros(M, f32), **kw)
        got = L.generate(prompts, count=Cn, u=u, h0=h0, c0=c0, score=True, info=True, guides=[(guide, 1.0, gh0, gc0)], main_weight=0.0, **kw)
        assert np.array_equal(want[0], got[0])
        assert np.array_equal(want[4]["kept"], got[4]["kept"]) and np.array_equal(want[4]["out_len"], got[4]["out_len"])
        assert got[4]["guide_h"][0].tobytes() == want[2].tobytes() and got[4]["guide_c"][0].tobytes() == want[3].tobytes()
        if stop is not None:
            assert (got[4]["out_len"] < Cn).any() and (got[4]["out_len"] == Cn).any()
        # the main model was fed the guide's bytes: its state is the one a call that draws nothing reaches over prompt ++ out
        fed = [np.concatenate([prompts[s], got[0][:got[4]["out_len"][s], s]]) for s in range(K)]
        alone = L.generate(fed, count=0, h0=h0, c0=c0)
        assert got[2].tobytes() == alone[2].tobytes() and got[3].tobytes() == alone[3].tobytes()
        # and the prompt bits are the main model's own
        assert np.array_equal(got[1], L.generate(prompts, count=0, h0=h0, c0=c0, score=True)[1])


def test_a_model_as_its_own_guide(models):
    """(2, -1) with the same weights and the same start state is the unguided call: 2z - z is exact.  From another start state
    for the guide the bytes are others."""
    L = models[0][0]
    rs = np.random.RandomState(31)
    prompts = _prompts(K, rs)
    h0, c0 = _state(K, N, seed=32)
    u = rs.random_sample((Cn, K))
    for kw in (dict(temperature=0.8), dict(temperature=0.0), dict(temperature=1.0, top_p=0.9)):
        want = L.generate(prompts, count=Cn, u=u, h0=h0, c0=c0, info=True, logit_bias=np.zeros(M, f32), **kw)
        got = L.generate(prompts, count=Cn, u=u, h0=h0, c0=c0, info=True, guides=[(L, -1.0, h0, c0)], main_weight=2.0, **kw)
        assert np.array_equal(want[0], got[0]) and np.array_equal(want[4]["kept"], got[4]["kept"]), kw
        assert got[2].tobytes() == want[2].tobytes() and got[4]["guide_h"][0].tobytes() == want[2].tobytes(), kw
        assert got[4]["guide_c"][0].tobytes() == want[3].tobytes(), kw
        other = L.generate(prompts, count=Cn, u=u, h0=h0, c0=c0, guides=[(L, -1.0, *_state(K, N, seed=33))], main_weight=2.0, **kw)
        assert not np.array_equal(other[0], want[0]), kw


# (temperature, top_k, top_p, stop byte, table (0 none, 1 table, 2 accepting), bias, min_p, n, weights (a, b_1, ..))
REFERENCE_CASES = {
    "two_guides_table_bias_n2": (0.9, 40, 0.9, -1, 1, True, 0.0, 2, (1.5, -0.75, 0.25)),
    "one_guide_greedy": (0.0, 0, 1.0, -1, 0, False, 0.0, 0, (1.5, -0.5)),
    "accepting_stop": (0.8, 0, 1.0, 10, 2, False, 0.05, 0, (1.5, -0.75, 0.25)),
    "padded_guide_temperature_1": (1.0, 0, 1.0, 101, 0, True, 0.0, 0, (0.5, 0.0, 0.5)),
}


def _check_against_the_reference(models, Kn, count, name, pick):
    import lstm_hip
    tau, top_k, top_p, stop, tmode, biased, min_p, n, w = REFERENCE_CASES[name]
    a, weights = w[0], list(w[1:])
    L, P = models[0]
    guides = models[1:1 + len(weights)]
    rs = np.random.RandomState(len(name) + Kn)
    table = accept = F = None
    if tmode == 1:
        table = lstm_hip.dfa_regex(b"(?:[a-m]x?|[n-z]{1,2}q)*", stop_byte=-1)[0]
    if tmode == 2:
        table, accept = lstm_hip.dfa_regex(b"(?:ab|[c-f]{2,3}|g)+", stop_byte=stop)
        F = dr.f_table(table, accept, stop, count)
    prompts = _prompts(Kn, rs, table, F, count)
    bias = (rs.randint(-48, 49, size=M) / 16).astype(f32) if biased else None
    h0, c0 = _state(Kn, N, seed=Kn)
    g0 = [_state(Kn, g.N, seed=Kn + 1 + k) for k, (g, _) in enumerate(guides)]
    u = rs.random_sample((count, Kn))
    u[1, 1] = 1.5  # past every edge
    kw = dict(temperature=tau, top_k=top_k, top_p=top_p, stop_byte=None if stop < 0 else stop, constraint=table, accept=accept)
    got = L.generate(prompts, count=count, u=u, h0=h0, c0=c0, info=True, logit_bias=bias, min_p=min_p, no_repeat_ngram=n,
                     guides=[(g, b, *g0[k]) for k, ((g, _), b) in enumerate(zip(guides, weights))], main_weight=a, **kw)
    out, info = got[0], got[4]
    # every model's state before every draw: the stream's prompt ++ its first i bytes fed by a call that draws nothing
    fed = [[np.concatenate([prompts[s], out[:i, s]]) for s in range(Kn)] for i in range(count)]
    H = [L.generate(fed[i], count=0, h0=h0, c0=c0)[2] for i in range(count)]
    GH = [[g.generate(fed[i], count=0, h0=g0[k][0], c0=g0[k][1])[2] for i in range(count)] for k, (g, _) in enumerate(guides)]
    params = []
    for h, Pm in [models[0]] + list(guides):
        sp = split_params(np.asarray(Pm, f32), h.N)
        params.append((np.asarray(sp["Why"], f32), np.asarray(sp["by"], f32).reshape(M)))
    mode = 2 if tau == 0.0 else 0 if tau == 1.0 else 1
    moved = 0
    for s in pick:
        q = cr.walk(table, 0, prompts[s]) if table is not None else 0
        T = bytes(prompts[s])
        n_end = count
        for i in range(count):
            V = lr.valid(table, q, accept, F, stop, count - i)
            z = _logits32(*params[0], H[i][s])
            zs = [_logits32(*params[1 + k], GH[k][i][s]) for k in range(len(guides))]
            x, k, _, _ = gr.draw32(z, zs, a, weights, V, T, mode, tau, top_k, top_p, u[i, s], bias, min_p, n)
            assert (int(out[i, s]), int(info["kept"][i, s])) == (x, k), (name, s, i, int(out[i, s]), int(info["kept"][i, s]), x, k)
            moved += (x, k) != lr.draw32(z, V, T, mode, tau, top_k, top_p, u[i, s], bias, min_p, n)[:2]
            T += bytes([x])
            q = int(table[q, x]) if table is not None else 0
            if x == stop:
                n_end = i + 1
                break
        assert info["out_len"][s] == n_end and not out[n_end:, s].any() and not info["kept"][n_end:, s].any(), (name, s)
        if table is not None:
            assert info["end_state"][s] == q, (name, s)
        if accept is not None:
            assert accept[q], (name, s)
        # every model's end state is its state after the stream's last input
        text = np.concatenate([prompts[s], out[:n_end, s]])
        assert got[2][s].tobytes() == L.generate([text], count=0, h0=h0[s:s + 1], c0=c0[s:s + 1])[2].tobytes(), (name, s)
        for kk, (g, _) in enumerate(guides):
            want = g.generate([text], count=0, h0=g0[kk][0][s:s + 1], c0=g0[kk][1][s:s + 1])
            assert info["guide_h"][kk][s].tobytes() == want[2].tobytes() and info["guide_c"][kk][s].tobytes() == want[3].tobytes(), (name, s, kk)
    return moved


@pytest.mark.parametrize("name", sorted(REFERENCE_CASES))
def test_device_draws_are_the_float32_reference(models, name):
    """20 streams, one a workgroup (SB = 1): bytes, kept, out_len, end_state and every model's end state against
    tests/guided_ref.py on the device's own states"""
    assert _group_rule()(N, K) == 1 and _group_rule()(max(GN) + 8, K) == 1
    moved = _check_against_the_reference(models, K, Cn, name, range(K))
    print(f"{name}: draws the guides moved {moved}")
    assert moved >= 5


def test_two_streams_a_workgroup_draw_the_float32_reference(models):
    """the smallest stream count that gen_head_group maps to SB = 2 at N = 16 (read from the function); the guides' kernel takes
    its group size from the widest guide by the same rule"""
    group = _group_rule()
    Kn = next(k for k in range(1, 4097) if group(N, k) == 2)
    assert group(N, Kn - 1) == 1 and group(48, Kn) == 2
    pick = sorted(set(list(range(6)) + list(range(Kn - 6, Kn)) + list(range(100, 108))))
    moved = _check_against_the_reference(models, Kn, 5, "two_guides_table_bias_n2", pick)
    assert moved >= 5


@pytest.mark.parametrize("a,b", gr.ORACLE_WEIGHTS)
@pytest.mark.parametrize("min_p,biased,top_k,top_p,tau", lr.ORACLE_SETTINGS)
def test_guided_draws_against_the_oracle(min_p, biased, top_k, top_p, tau, a, b, oracle32):
    """As test_processed_draws_against_the_oracle: the drawn bytes are fed back through the oracle, for both models, and the
    float64 rule is applied to each step's mixed distribution.  Ambiguous draws (their share on oracle trajectories is what
    tests/test_guided_cpu.py controls) are skipped, at most 5 % of them.  The CDF slack is that test's 1e-5 times |a| + |b|: a
    mixed logit carries that multiple of one logit's rounding."""
    Nm, Kn, count = sr.ORACLE_N, sr.ORACLE_STREAMS, sr.ORACLE_COUNT
    P, prompts, u = sr.oracle_case()
    Pg = gr.oracle_guide()
    bias = lr.oracle_bias() if biased else None
    L, G = _handle(Nm, P), _handle(gr.ORACLE_GUIDE_N, Pg)
    out, _, _, _, info = L.generate(prompts, count=count, u=u, temperature=tau, top_k=top_k, top_p=top_p, info=True,
                                    logit_bias=bias, min_p=min_p, guides=[(G, b)], main_weight=a)
    L.close()
    G.close()
    kept = info["kept"]
    S = np.ones(M, bool)
    slack = 1e-5 * (abs(a) + abs(b))
    skipped = checked = inside = near = 0
    keeps = []
    for s in range(Kn):
        p1 = sr.replay(oracle32, Nm, P, prompts[s], out[:, s])
        pg = sr.replay(oracle32, gr.ORACLE_GUIDE_N, Pg, prompts[s], out[:, s])
        for i in range(count):
            keep, mask, q, p = gr.filter64(p1[i], [pg[i]], a, [b], S, tau, top_k, top_p, min_p, bias)
            if lr.ambiguous(p, S, top_k, top_p, min_p):
                skipped += 1
                continue
            x = int(out[i, s])
            assert mask[x], (s, i, x, keep)
            assert int(kept[i, s]) == keep, (s, i, int(kept[i, s]), keep)
            keeps.append(keep)
            lo = q[:x].sum()
            hi = lo + q[x]
            checked += 1
            inside += lo <= u[i, s] < hi
            near += lo - slack <= u[i, s] < hi + slack
    print(f"weights ({a}, {b}) min_p {min_p} bias {biased} top_k {top_k} top_p {top_p} tau {tau}: skipped {skipped}, "
          f"checked {checked}, inside {inside}, near {near}, mean kept {np.mean(keeps):.2f}")
    assert skipped <= 0.05 * Kn * count, skipped
    assert inside >= 0.99 * checked and near == checked, (inside, near, checked)


@pytest.mark.parametrize("with_table", [False, True])
def test_two_calls_with_every_state_handed_over_are_the_one_call(models, with_table):
    import lstm_hip
    (L, _), (G, _), (G2, _) = models
    first = 6
    rs = np.random.RandomState(32)
    table = lstm_hip.dfa_utf8() if with_table else None
    prompts = _prompts(K, rs)
    histories = [rs.randint(97, 123, size=(5 * s) % 7).astype(np.uint8) for s in range(K)]
    h0, c0 = _state(K, N, seed=33)
    g0 = [_state(K, GN[0], seed=34), _state(K, GN[1], seed=35)]
    u = rs.random_sample((Cn, K))
    bias = (rs.randn(M) * 0.5).astype(f32)
    gl = lambda st: [(G, -0.75, *st[0]), (G2, 0.25, *st[1])]
    for kw in (dict(temperature=0.0, no_repeat_ngram=2), dict(temperature=0.8, no_repeat_ngram=3, min_p=0.05, logit_bias=bias),
               dict(temperature=1.0, top_k=40, top_p=0.9)):
        hist = histories if "no_repeat_ngram" in kw else None
        run = lambda **x: L.generate(info=True, constraint=table, main_weight=1.5, **kw, **x)
        one = run(prompts=prompts, count=Cn, u=u, h0=h0, c0=c0, history=hist, guides=gl(g0))
        p1 = run(prompts=prompts, count=first, u=u[:first], h0=h0, c0=c0, history=hist, guides=gl(g0))
        handed = [np.concatenate([histories[s], prompts[s], p1[0][:, s]]) for s in range(K)] if hist is not None else None
        mid = list(zip(p1[4]["guide_h"], p1[4]["guide_c"]))
        p2 = run(prompts=None, count=Cn - first, u=u[first:], h0=p1[2], c0=p1[3], streams=K, history=handed, guides=gl(mid),
                 start_state=p1[4]["end_state"] if with_table else None)
        assert np.array_equal(one[0], np.concatenate([p1[0], p2[0]])), kw
        assert np.array_equal(one[4]["kept"], np.concatenate([p1[4]["kept"], p2[4]["kept"]])), kw
        assert one[2].tobytes() == p2[2].tobytes() and one[3].tobytes() == p2[3].tobytes(), kw
        for k in range(2):
            assert one[4]["guide_h"][k].tobytes() == p2[4]["guide_h"][k].tobytes(), (kw, k)
            assert one[4]["guide_c"][k].tobytes() == p2[4]["guide_c"][k].tobytes(), (kw, k)
        if with_table:
            assert np.array_equal(one[4]["end_state"], p2[4]["end_state"]), kw


def _snapshot(L):
    import lstm_hip
    return ([L.get_params(w).tobytes() for w in (lstm_hip.P_PARAMS, lstm_hip.P_GRADS, lstm_hip.P_MEM)]
            + [a.tobytes() for a in L.get_window()] + [L.get_cursors().tobytes(), L.optimizer_steps()])


def test_a_guided_call_leaves_both_handles_as_they_were():
    import lstm_hip
    S, B = 6, 2
    text = np.random.RandomState(81).randint(97, 123, size=3000).astype(np.uint8)
    hs = []
    for n, seed in ((N, 5), (GN[0], 6)):
        L = lstm_hip.Lstm(n, S, B)
        L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(seed), n))
        L.set_text(text)
        L.set_cursors(lstm_hip.initial_cursors(text.size, S, B))
        L.train_windows(3, 0.1)
        hs.append(L)
    A, G = hs
    before = [_snapshot(A), _snapshot(G)]
    u = np.random.RandomState(82).random_sample((8, 3))
    out = A.generate([b"ab", b"", b"abc"], count=8, u=u, temperature=0.9, guides=[(G, -0.5), (A, 0.25)], main_weight=1.25)[0]
    assert out.shape == (8, 3)
    A.score_guided([b"hello", b"", b"ab"], first=True, top_n=2, guides=[(G, 0.5)], main_weight=0.5)
    assert [_snapshot(A), _snapshot(G)] == before
    la, lg = A.train_windows(2, 0.1), G.train_windows(2, 0.1)
    assert np.isfinite(la).all() and np.isfinite(lg).all()
    A.close()
    G.close()


def test_program_takes_guides(tmp_path):
    """lstm_generate: --score under (0, 1) is the guide checkpoint's own score line; --guidance 0 prints the unguided greedy
    samples and another G prints samples of the same shape; a guide of another width draws under a table"""
    import subprocess
    lstm, gen = os.path.join(ROOT, "eigen-lstm_amd", "lstm"), os.path.join(ROOT, "eigen-lstm_amd", "lstm_generate")
    rs = np.random.RandomState(81)
    text = b"".join(bytes(rs.randint(97, 110, size=rs.randint(3, 13)).astype(np.uint8)) + b"\n" for _ in range(500))
    corpus, held = tmp_path / "corpus.txt", tmp_path / "held.txt"
    corpus.write_bytes(text)
    held.write_bytes(text[:300])
    for hidden, name in (("64", "big"), ("24", "small")):
        tr = subprocess.run([lstm, str(corpus), hidden, "8", "4", "0.1", "--epochs", "1", "--windows", "150", "--sample", "0",
                             "--save", str(tmp_path / name), "--quiet"], capture_output=True, text=True, errors="replace", timeout=300)
        assert tr.returncode == 0, tr.stderr
    big, small = str(tmp_path / "big"), str(tmp_path / "small")
    run = lambda *a: subprocess.run([gen, *a], capture_output=True, timeout=300)
    line = lambda res: res.stdout.split(b"\n")[0].split(b": ", 1)[1]
    own = run("--load", small, "--score", str(held))
    mixed = run("--load", big, "--score", str(held), "--guide", small, "--guide-weight", "1", "--main-weight", "0")
    half = run("--load", big, "--score", str(held), "--guide", small, "--guide-weight", "0.5", "--main-weight", "0.5")
    assert own.returncode == 0 and mixed.returncode == 0 and half.returncode == 0, (own.stderr, mixed.stderr, half.stderr)
    assert line(own) == line(mixed) and line(half) != line(own), (own.stdout, mixed.stdout, half.stdout)
    rows = run("--load", big, "--score-bytes", str(held), "--top", "2", "--guide", small, "--guide-weight", "1", "--main-weight", "0")
    assert rows.returncode == 0 and rows.stdout.split(b"\n")[-2].split(b": ", 1)[1] == line(own), rows.stderr

    def samples(res):
        assert res.returncode == 0, res.stderr
        parts = res.stdout.split(b"== sample ")[1:]
        assert len(parts) == 3
        return [p.split(b" ==\n", 1)[1][:-1] for p in parts]

    common = ["--load", big, "--count", "60", "--streams", "3", "--prime", "ab", "--temperature", "0"]
    plain = samples(run(*common))
    assert samples(run(*common, "--guidance", "0", "--negative-prime", "zz")) == plain  # weights (1, -0)
    for extra in (["--guidance", "1.5"], ["--guidance", "1.5", "--negative-prime", "k\n", "--no-repeat-ngram", "4"],
                  ["--guide", small, "--guide-weight", "-0.5", "--main-weight", "1.5", "--allow", "97-109,10"]):
        got = samples(run(*common, *extra))
        assert all(len(t) == 62 and t.startswith(b"ab") for t in got), (extra, got)
        if "--allow" in extra:
            assert all(set(t) <= set(range(97, 110)) | {10} for t in got), got
        if "--no-repeat-ngram" in extra:
            assert not any(lr.repeats_ngram(t, 4) for t in got), got
