"""-m gpu: lstm_hip_generate_processed -- an additive bias, min-p and the no-repeat n-gram rule in the batched generator
(include/lstm_hip.h).

With the block NULL or all off the call is lstm_hip_generate_accepting byte for byte; at N = 16 the device's bytes, kept counts,
lengths and end states are those of the float32 reference (tests/logit_processor_ref.py) on the device's own states; against
the oracle every drawn byte lies in the float64 kept set; greedy decoding that cycles stops cycling under no_repeat_ngram and is
the oracle's masked argmax; a call in two pieces with the history handed over is the one long call; and under a pattern that
needs a repeated byte the ban gives way and every sample still matches."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import constraint_ref as cr
import deadline_ref as dr
import logit_processor_ref as lr
import sampling_ref as sr
from logits_ref import logits32 as _logits32
from oracle_lib import split_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 256
f32 = np.float32
NAMES = ("out", "bits", "h", "c", "out_len", "kept", "end_state")


def _state(streams, N, seed):
    rs = np.random.RandomState(seed)
    return (rs.randn(streams, N) * 0.1).astype(f32), (rs.randn(streams, N) * 0.1).astype(f32)


def _same(a, b, names=NAMES):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]) for k in names)


def _raw(L, fn, prompts, count, u, temperature, h0, c0, table=None, accept=None, top_k=0, top_p=1.0, stop_byte=-1, lp="absent"):
    """lstm_hip_generate_accepting (fn = "accepting") or lstm_hip_generate_processed with lp NULL (None) or a block (a tuple
    bias, min_p, no_repeat) through ctypes: the seven results"""
    import lstm_hip
    p = lstm_hip._ptr
    K, N = len(prompts), L.N
    data, off = lstm_hip._offsets(lstm_hip._bytes_list(prompts))
    opt = lstm_hip._Sampling(C.sizeof(lstm_hip._Sampling), temperature, top_k, top_p, stop_byte)
    out, bits = np.zeros((count, K), np.uint8), np.zeros(K)
    h, c = np.empty((K, N), f32), np.empty((K, N), f32)
    out_len, kept, end = np.zeros(K, np.int32), np.zeros((count, K), np.uint16), np.zeros(K, np.int32)
    bc = None
    if table is not None:
        t = np.ascontiguousarray(table, np.uint16)
        con = lstm_hip._Constraint(C.sizeof(lstm_hip._Constraint), t.shape[0], p(t, C.c_uint16))
        acc = None if accept is None else np.ascontiguousarray(accept, np.uint8)
        bc = lstm_hip._BeamConstraint(C.sizeof(lstm_hip._BeamConstraint), C.pointer(con), p(acc, C.c_uint8) if acc is not None else None)
    args = [L._h, C.c_int32(K), p(data, C.c_uint8), p(off, C.c_uint64), p(h0), p(c0), C.byref(opt), p(u, C.c_double),
            C.c_int32(count), p(out, C.c_uint8), p(bits, C.c_double), p(h), p(c), p(out_len, C.c_int32), p(kept, C.c_uint16),
            C.byref(bc) if bc is not None else None, None, p(end, C.c_int32) if bc is not None else None]
    if fn == "accepting":
        rc = L.lib.lstm_hip_generate_accepting(*args)
    else:
        block = None
        if lp is not None:
            bias, min_p, n = lp
            block = lstm_hip._LogitProcessors(C.sizeof(lstm_hip._LogitProcessors), p(bias) if bias is not None else None,
                                              min_p, n, None, None)
        rc = L.lib.lstm_hip_generate_processed(*args, C.byref(block) if block is not None else None)
    assert rc == 0, L.lib.lstm_hip_last_error()
    return dict(zip(NAMES, (out, bits, h, c, out_len, kept, end if bc is not None else None)))


@pytest.mark.parametrize("which", ["plain", "constrained", "accepting"])
def test_off_is_the_old_call(which):
    import lstm_hip
    N, K, Cn = 64, 7, 40
    P = sr.peaked_params(N, seed=3)
    rs = np.random.RandomState(4)
    prompts = [rs.randint(97, 123, size=n).astype(np.uint8) for n in [0, 1, 2, 9, 40, 13, 5]]
    h0, c0 = _state(K, N, seed=5)
    u = rs.random_sample((Cn, K))
    table = accept = None
    stop = -1
    if which == "constrained":
        table = lstm_hip.dfa_utf8()
    if which == "accepting":
        table, accept = lstm_hip.dfa_regex(b"[a-z ]*", stop_byte=10)
        stop = 10
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(P)
    for tau in (1.0, 0.7, 0.0):
        for kw in (dict(), dict(top_k=40, top_p=0.9)):
            run = lambda fn, **extra: _raw(L, fn, prompts, Cn, u, tau, h0, c0, table, accept, stop_byte=stop, **kw, **extra)
            old = run("accepting")
            assert _same(old, run("processed", lp=None)), (tau, kw)
            assert _same(old, run("processed", lp=(None, 0.0, 0))), (tau, kw)
            # and a processor that is on is another call (the block is not ignored)
            on = run("processed", lp=(None, 0.0, 1))
            assert not np.array_equal(on["out"], old["out"]), (tau, kw)
    L.close()


def _group_rule():
    """gen_head_group of kernels.hip as a Python function of (N, streams), read from its text"""
    text = open(os.path.join(ROOT, "eigen-lstm_amd", "csrc", "kernels.hip")).read()
    m = re.search(r"int gen_head_group\(int N, int streams\) \{\s*int sb = 1;[^\n]*\n\s*while \((.*?)\) sb \*= 2;\s*return sb;", text)
    assert m, "gen_head_group has changed its shape"
    cond = m.group(1).replace("(size_t)", "").replace("&&", " and ")
    assert re.fullmatch(r"[\w\s<>=*()]+", cond), cond

    def group(N, streams):
        sb = 1
        while eval(cond, {}, dict(sb=sb, N=N, streams=streams)):
            sb *= 2
        return sb
    return group


# (temperature, top_k, top_p, stop byte, table (0 none, 1 table, 2 accepting), bias, min_p, n, history)
REFERENCE_CASES = {
    "bias_tempered": (0.8, 0, 1.0, -1, 0, True, 0.0, 0, False),
    "min_p_top_k_nucleus": (1.3, 30, 0.95, -1, 0, False, 0.1, 0, False),
    "min_p_temperature_1_bias": (1.0, 0, 1.0, -1, 0, True, 0.2, 0, False),
    "n3_greedy_history": (0.0, 0, 1.0, -1, 0, False, 0.0, 3, True),
    "n1_tempered_stop": (0.6, 0, 1.0, 101, 0, False, 0.0, 1, False),
    "n2_table_all": (0.9, 40, 0.9, -1, 1, True, 0.1, 2, True),
    "n2_accepting_greedy": (0.0, 0, 1.0, 10, 2, False, 0.0, 2, True),
}


def _check_against_the_reference(L, P, N, K, Cn, name, pick):
    import lstm_hip
    tau, top_k, top_p, stop, tmode, biased, min_p, n, with_history = REFERENCE_CASES[name]
    rs = np.random.RandomState(len(name) + K)
    table = accept = F = None
    if tmode == 1:
        table = lstm_hip.dfa_regex(b"(?:[a-m]x?|[n-z]{1,2}q)*", stop_byte=-1)[0]
    if tmode == 2:
        table, accept = lstm_hip.dfa_regex(b"(?:ab|[c-f]{2,3}|g)+", stop_byte=stop)
        F = dr.f_table(table, accept, stop, Cn)
    lengths = [(3 * s) % 5 for s in range(K)]
    prompts = []
    for L_s in lengths:
        q, p = 0, []
        for _ in range(L_s):
            good = [b for b in range(97, 123) if table is None or (table[q, b] != cr.FORBID and (F is None or F[Cn][table[q, b]]))]
            b = int(rs.choice(good))
            p.append(b)
            q = int(table[q, b]) if table is not None else 0
        prompts.append(np.array(p, np.uint8))
    histories = [rs.randint(97, 101, size=(7 * s) % 11).astype(np.uint8) for s in range(K)] if with_history else None
    bias = (rs.randint(-48, 49, size=M) / 16).astype(f32) if biased else None
    h0, c0 = _state(K, N, seed=K)
    u = rs.random_sample((Cn, K))
    u[1, 1] = 1.5  # past every edge
    kw = dict(temperature=tau, top_k=top_k, top_p=top_p, stop_byte=None if stop < 0 else stop, constraint=table, accept=accept)
    got = L.generate(prompts, count=Cn, u=u, h0=h0, c0=c0, info=True, logit_bias=bias, min_p=min_p, no_repeat_ngram=n,
                     history=histories, **kw)
    out, info = got[0], got[4]
    # the state before every draw: the stream's prompt ++ its first i bytes fed by a call that draws nothing
    H = [L.generate([np.concatenate([prompts[s], out[:i, s]]) for s in range(K)], count=0, h0=h0, c0=c0)[2] for i in range(Cn)]
    sp = split_params(np.asarray(P, f32), N)
    Why, by = np.asarray(sp["Why"], f32), np.asarray(sp["by"], f32).reshape(M)
    mode = 2 if tau == 0.0 else 0 if tau == 1.0 else 1
    bit = drops = cut = 0
    for s in pick:
        q = cr.walk(table, 0, prompts[s]) if table is not None else 0
        T = (bytes(histories[s]) if histories else b"") + bytes(prompts[s])
        n_end = Cn
        for i in range(Cn):
            V = lr.valid(table, q, accept, F, stop, Cn - i)
            z = _logits32(Why, by, H[i][s])
            x, k, b, dropped = lr.draw32(z, V, T, mode, tau, top_k, top_p, u[i, s], bias, min_p, n)
            assert (int(out[i, s]), int(info["kept"][i, s])) == (x, k), (name, s, i, int(out[i, s]), int(info["kept"][i, s]), x, k)
            bit += b
            drops += dropped
            cut += k < int(V.sum())
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
    return bit, drops, cut


@pytest.mark.parametrize("name", sorted(REFERENCE_CASES))
def test_device_draws_are_the_float32_reference(name):
    """20 streams, one a workgroup (SB = 1): bytes, kept, out_len and end_state equal tests/logit_processor_ref.py on the
    device's own states"""
    import lstm_hip
    N, K, Cn = 16, 20, 14
    assert _group_rule()(N, K) == 1
    P = sr.peaked_params(N, seed=7, gain=6.0)
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(P)
    bit, drops, cut = _check_against_the_reference(L, P, N, K, Cn, name, range(K))
    L.close()
    n, min_p = REFERENCE_CASES[name][7], REFERENCE_CASES[name][6]
    print(f"{name}: draws with a valid byte banned {bit}, with the ban dropped {drops}, with keep below the valid bytes {cut}")
    if n > 0:
        assert bit >= 1
    if min_p > 0:
        assert cut >= 1


def test_two_streams_a_workgroup_draw_the_float32_reference():
    """the smallest stream count that gen_head_group maps to SB = 2 at N = 16 (read from the function)"""
    import lstm_hip
    N, Cn = 16, 6
    group = _group_rule()
    K = next(k for k in range(1, 4097) if group(N, k) == 2)
    assert group(N, K - 1) == 1
    P = sr.peaked_params(N, seed=7, gain=6.0)
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(P)
    pick = sorted(set(list(range(8)) + list(range(K - 8, K)) + list(range(100, 116))))
    bit, _, cut = _check_against_the_reference(L, P, N, K, Cn, "n2_table_all", pick)
    L.close()
    assert bit >= 1 and cut >= 1


@pytest.mark.parametrize("min_p,biased,top_k,top_p,tau", lr.ORACLE_SETTINGS)
def test_processed_draws_against_the_oracle(min_p, biased, top_k, top_p, tau, oracle32):
    """As test_filtered_draws_against_the_oracle: the drawn bytes are fed back through the oracle and the float64 rule is
    applied to each step's distribution.  Ambiguous draws (tests/logit_processor_ref.py; their share on oracle trajectories
    is what tests/test_logit_processors_cpu.py controls) are skipped, at most 5 % of them."""
    import lstm_hip
    N, K, Cn = sr.ORACLE_N, sr.ORACLE_STREAMS, sr.ORACLE_COUNT
    P, prompts, u = sr.oracle_case()
    bias = lr.oracle_bias() if biased else None
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(P)
    out, _, _, _, info = L.generate(prompts, count=Cn, u=u, temperature=tau, top_k=top_k, top_p=top_p, info=True,
                                    logit_bias=bias, min_p=min_p)
    L.close()
    kept = info["kept"]
    S = np.ones(M, bool)
    skipped = checked = inside = near = 0
    keeps = []
    for s in range(K):
        p1 = sr.replay(oracle32, N, P, prompts[s], out[:, s])
        for i in range(Cn):
            keep, mask, q, p = lr.filter64(p1[i], S, tau, top_k, top_p, min_p, bias)
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
            near += lo - 1e-5 <= u[i, s] < hi + 1e-5
    print(f"min_p {min_p} bias {biased} top_k {top_k} top_p {top_p} tau {tau}: skipped {skipped}, checked {checked}, "
          f"inside {inside}, near {near}, mean kept {np.mean(keeps):.2f}")
    assert skipped <= 0.05 * K * Cn, skipped
    assert inside >= 0.99 * checked and near == checked, (inside, near, checked)


def test_no_repeat_ngram_ends_the_loops_of_greedy_decoding(oracle32):
    """The peaked parameters cycle under greedy decoding (tests/test_logit_processors_cpu.py checks it on the oracle).  With
    no_repeat_ngram = 4 no 4-gram occurs twice in history ++ prompt ++ out, and every byte is the oracle replay's argmax
    over the bytes the rule leaves, wherever the top two of them are more than 1e-4 apart in logit."""
    import lstm_hip
    N, K, Cn, n = sr.ORACLE_N, sr.ORACLE_STREAMS, 60, 4
    P, prompts, _ = sr.oracle_case()
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(P)
    free = L.generate(prompts, count=Cn, temperature=0.0)[0]
    assert all(lr.repeats_ngram(bytes(prompts[s]) + free[:, s].tobytes(), n) for s in range(K))
    # the history: the free run's first bytes, which the stream is then kept from saying again (never fed, never scored)
    histories = []
    for s in range(K):
        k = 12
        while lr.repeats_ngram(free[:k, s].tobytes() + bytes(prompts[s]), n):
            k -= 1
        histories.append(free[:k, s].copy())
    assert sum(h.size for h in histories) >= 4 * K
    out, _, _, _, info = L.generate(prompts, count=Cn, temperature=0.0, info=True, no_repeat_ngram=n, history=histories)
    L.close()
    assert (info["kept"] == 1).all() and (info["out_len"] == Cn).all()
    compared = 0
    for s in range(K):
        T = bytes(histories[s]) + bytes(prompts[s])
        assert not lr.repeats_ngram(T + out[:, s].tobytes(), n), s
        assert not np.array_equal(out[:, s], free[:, s]), s
        p1 = sr.replay(oracle32, N, P, prompts[s], out[:, s])
        for i in range(Cn):
            B = lr.ngram_banned(T, n)
            z = np.where(B, -np.inf, np.log(p1[i]))
            top = np.sort(z)[::-1]
            if top[0] - top[1] > 1e-4:
                assert int(out[i, s]) == int(np.argmax(z)), (s, i)
                compared += 1
            assert not B[out[i, s]], (s, i)
            T += bytes([out[i, s]])
    assert compared >= 0.9 * K * Cn, compared


@pytest.mark.parametrize("with_table", [False, True])
def test_two_calls_with_the_history_handed_over_are_the_one_call(with_table):
    import lstm_hip
    N, K, Cn, first = 64, 9, 24, 10
    P = sr.peaked_params(N, seed=31)
    rs = np.random.RandomState(32)
    prompts = [rs.randint(97, 123, size=m).astype(np.uint8) for m in [0, 1, 2, 9, 4, 13, 5, 0, 3]]
    histories = [rs.randint(97, 123, size=m).astype(np.uint8) for m in [4, 0, 7, 1, 0, 20, 2, 0, 9]]
    h0, c0 = _state(K, N, seed=33)
    u = rs.random_sample((Cn, K))
    bias = (rs.randn(M) * 0.5).astype(f32)
    table = lstm_hip.dfa_utf8() if with_table else None
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(P)
    for kw in (dict(temperature=0.0, no_repeat_ngram=2), dict(temperature=0.8, no_repeat_ngram=3, min_p=0.05, logit_bias=bias),
               dict(temperature=1.0, no_repeat_ngram=1, top_k=40, top_p=0.9)):
        one = L.generate(prompts, count=Cn, u=u, h0=h0, c0=c0, info=True, constraint=table, history=histories, **kw)
        a = L.generate(prompts, count=first, u=u[:first], h0=h0, c0=c0, info=True, constraint=table, history=histories, **kw)
        handed = [np.concatenate([histories[s], prompts[s], a[0][:, s]]) for s in range(K)]
        b = L.generate(None, count=Cn - first, u=u[first:], h0=a[2], c0=a[3], streams=K, info=True, constraint=table,
                       start_state=a[4]["end_state"] if with_table else None, history=handed, **kw)
        assert np.array_equal(one[0], np.concatenate([a[0], b[0]])), kw
        assert np.array_equal(one[4]["kept"], np.concatenate([a[4]["kept"], b[4]["kept"]])), kw
        assert np.array_equal(one[2], b[2]) and np.array_equal(one[3], b[3]), kw
        if with_table:
            assert np.array_equal(one[4]["end_state"], b[4]["end_state"]), kw
        # the rule did something: without it the bytes are others
        free = L.generate(prompts, count=Cn, u=u, h0=h0, c0=c0, constraint=table,
                          **{k: v for k, v in kw.items() if k not in ("no_repeat_ngram",)})
        assert not np.array_equal(free[0], one[0]), kw
    L.close()


def test_program_takes_the_three_flags(tmp_path):
    import subprocess
    lstm, gen = os.path.join(ROOT, "eigen-lstm_amd", "lstm"), os.path.join(ROOT, "eigen-lstm_amd", "lstm_generate")
    rs = np.random.RandomState(81)
    text = b"".join(bytes(rs.randint(97, 110, size=rs.randint(3, 13)).astype(np.uint8)) + b"\n" for _ in range(500))
    corpus = tmp_path / "corpus.txt"
    corpus.write_bytes(text)
    tr = subprocess.run([lstm, str(corpus), "64", "8", "4", "0.1", "--epochs", "1", "--windows", "200", "--sample", "0",
                         "--save", str(tmp_path / "ck"), "--quiet"], capture_output=True, text=True, errors="replace", timeout=300)
    assert tr.returncode == 0, tr.stderr
    run = lambda *extra: subprocess.run([gen, "--load", str(tmp_path / "ck"), "--count", "80", "--streams", "3", "--prime", "ab",
                                         *extra], capture_output=True, timeout=300)

    def samples(res):
        assert res.returncode == 0, res.stderr
        parts = res.stdout.split(b"== sample ")[1:]
        assert len(parts) == 3
        return [p.split(b" ==\n", 1)[1][:-1] for p in parts]  # (the program ends every sample with a newline of its own)

    greedy = samples(run("--temperature", "0"))
    assert all(lr.repeats_ngram(t, 4) for t in greedy)  # the loop of greedy decoding
    free = samples(run("--temperature", "0", "--no-repeat-ngram", "4"))
    assert all(len(t) == 82 and t.startswith(b"ab") and not lr.repeats_ngram(t, 4) for t in free), free
    common = bytes([np.bincount(np.frombuffer(greedy[0][2:], np.uint8), minlength=256).argmax()])
    pushed = samples(run("--temperature", "0", "--logit-bias", f"{common[0]}:-100"))
    assert all(common not in t[2:] for t in pushed), (common, pushed)
    drawn, cut = samples(run("--seed", "3", "--temperature", "1.5")), samples(run("--seed", "3", "--temperature", "1.5", "--min-p", "0.5"))
    assert drawn != cut


def test_the_table_wins_over_the_ban():
    """[0-9]{3}-[0-9]{4} and a newline with no_repeat_ngram = 1.  Seven different digits exist, so without a history the ban
    holds at every draw and the digits of a sample all differ.  With a history that holds every digit, the hyphen and the
    newline, the ban leaves no byte at any draw: it must be dropped for a match to be finished.  Either way every sample fully
    matches and ends in an accepting state."""
    import lstm_hip
    N, K, Cn = 64, 40, 12
    table, accept = lstm_hip.dfa_regex(b"[0-9]{3}-[0-9]{4}", stop_byte=10)
    P = sr.peaked_params(N, seed=41)
    h0, c0 = _state(K, N, seed=42)
    u = np.random.RandomState(43).random_sample((Cn, K))
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(P)
    for tau, history in ((1.5, None), (0.0, None), (1.5, [b"0123456789-\n"] * K)):
        out, _, _, _, info = L.generate(count=Cn, u=u, temperature=tau, h0=h0, c0=c0, streams=K, stop_byte=10, info=True,
                                        constraint=table, accept=accept, no_repeat_ngram=1, history=history)
        texts = set()
        for s in range(K):
            m = int(info["out_len"][s])
            text = out[:m, s].tobytes()
            assert re.fullmatch(rb"[0-9]{3}-[0-9]{4}\n", text), (tau, s, text)
            assert accept[info["end_state"][s]] and not out[m:, s].any()
            if history is None:  # the ban holds: no byte comes twice
                assert len(set(text)) == len(text), (s, text)
            texts.add(text)
        if tau > 0:
            assert len(texts) >= 2
    L.close()
