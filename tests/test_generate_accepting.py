"""-m gpu: lstm_hip_generate_accepting -- sampling under a byte automaton with accepting states and a deadline
(include/lstm_hip.h), and lstm_hip_dfa_regex as the source of its tables.

Without accepting states the call is lstm_hip_generate_constrained bit for bit, and without a constraint lstm_hip_generate_ex;
a deadline that rules nothing out changes nothing; under a compiled pattern every stream is a whole match, where the same draws
without accepting states end inside the pattern; a language with one string of the asked length forces it; against the oracle
every drawn byte lies in the float64 reference's kept set of the bytes that exist (tests/deadline_ref.py), with the thresholds
of test_utf8_outputs_are_valid_and_match_the_oracle; wide batches, a padded handle and the average as source agree with
small batches and a second handle; non-finite parameters still end in accepting states; the program and beam search take the
compiler's tables."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import beam_constraint_ref as bcr
import constraint_ref as cr
import deadline_ref as dr
import sampling_ref as sr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSTM = os.path.join(ROOT, "eigen-lstm_amd", "lstm")
GEN = os.path.join(ROOT, "eigen-lstm_amd", "lstm_generate")
FILTERS = dict(top_k=40, top_p=0.9)
NAMES = ("out", "bits", "h", "c", "out_len", "kept", "end_state")


def _state(streams, N, seed):
    rs = np.random.RandomState(seed)
    return (rs.randn(streams, N) * 0.1).astype(np.float32), (rs.randn(streams, N) * 0.1).astype(np.float32)


def _seven(res):
    """the seven results of Lstm.generate(score=True, info=True) as a dict"""
    return dict(zip(NAMES, list(res[:4]) + [res[4].get(k) for k in NAMES[4:]]))


def _same(a, b, names=NAMES):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]) for k in names)


def _raw(L, prompts, count, u, temperature, h0, c0, table, accept, start=None, top_k=0, top_p=1.0, stop_byte=-1, no_bc=False):
    """lstm_hip_generate_accepting itself (the wrapper takes the old entry point when accept is None): the seven results"""
    import lstm_hip
    p = lstm_hip._ptr
    K, N = len(prompts), L.N
    data, off = lstm_hip._offsets(lstm_hip._bytes_list(prompts))
    opt = lstm_hip._Sampling(C.sizeof(lstm_hip._Sampling), temperature, top_k, top_p, stop_byte)
    out, bits = np.zeros((count, K), np.uint8), np.zeros(K)
    h, c = np.empty((K, N), np.float32), np.empty((K, N), np.float32)
    out_len, kept, end = np.zeros(K, np.int32), np.zeros((count, K), np.uint16), np.zeros(K, np.int32)
    t = np.ascontiguousarray(table, np.uint16)
    con = lstm_hip._Constraint(C.sizeof(lstm_hip._Constraint), t.shape[0], p(t, C.c_uint16))
    acc = None if accept is None else np.ascontiguousarray(accept, np.uint8)
    bc = lstm_hip._BeamConstraint(C.sizeof(lstm_hip._BeamConstraint), C.pointer(con), p(acc, C.c_uint8) if acc is not None else None)
    rc = L.lib.lstm_hip_generate_accepting(
        L._h, C.c_int32(K), p(data, C.c_uint8), p(off, C.c_uint64), p(h0), p(c0), C.byref(opt), p(u, C.c_double), C.c_int32(count),
        p(out, C.c_uint8), p(bits, C.c_double), p(h), p(c), p(out_len, C.c_int32), p(kept, C.c_uint16), None if no_bc else C.byref(bc),
        None if start is None or no_bc else p(start, C.c_int32), None if no_bc else p(end, C.c_int32))
    assert rc == 0, L.lib.lstm_hip_last_error()
    return dict(zip(NAMES, (out, bits, h, c, out_len, kept, None if no_bc else end)))


@pytest.mark.parametrize("flags", [0, 512])  # 512: LSTM_HIP_STABLE_SOFTMAX
def test_without_accepting_states_the_call_is_generate_constrained(flags):
    import lstm_hip
    N, K, Cn = 128, 7, 60
    P = sr.peaked_params(N, seed=3, scale=0.1)
    rs = np.random.RandomState(4)
    prompts = [rs.randint(32, 127, size=n).astype(np.uint8) for n in [0, 1, 2, 9, 40, 130, 5]]
    h0, c0 = _state(K, N, seed=5)
    u = rs.random_sample((Cn, K))
    table = lstm_hip.dfa_utf8()
    L = lstm_hip.Lstm(N, 2, 1, flags=flags)
    L.set_params(P)
    for tau in (1.0, 0.7, 0.0):
        for kw in (dict(), dict(FILTERS), dict(stop_byte=101), dict(FILTERS, stop_byte=101)):
            old = _seven(L.generate(prompts, count=Cn, u=u, temperature=tau, h0=h0, c0=c0, score=True, info=True, constraint=table, **kw))
            assert _same(old, _raw(L, prompts, Cn, u, tau, h0, c0, table, None, **kw)), (tau, kw)
            assert _same(old, _seven(L.generate(prompts, count=Cn, u=u, temperature=tau, h0=h0, c0=c0, score=True, info=True,
                                                constraint=table, accept=None, **kw))), (tau, kw)
            # and a null beam constraint is lstm_hip_generate_ex
            ex = _seven(L.generate(prompts, count=Cn, u=u, temperature=tau, h0=h0, c0=c0, score=True, info=True, **kw))
            assert _same(ex, _raw(L, prompts, Cn, u, tau, h0, c0, table, None, no_bc=True, **kw), NAMES[:6]), (tau, kw)
    L.close()


@pytest.mark.parametrize("which", ["all_allowed", "utf8"])
def test_a_deadline_that_rules_nothing_out_changes_nothing(which):
    import lstm_hip
    N, K, Cn = 100, 9, 50
    table = np.zeros((1, 256), np.uint16) if which == "all_allowed" else lstm_hip.dfa_utf8()
    P = sr.peaked_params(N, seed=11, scale=0.1)
    rs = np.random.RandomState(12)
    prompts = [rs.randint(32, 127, size=n).astype(np.uint8) for n in [3, 0, 17, 40, 1, 9, 2, 2, 60]]
    h0, c0 = _state(K, N, seed=13)
    u = rs.random_sample((Cn, K))
    L = lstm_hip.Lstm(N, 2, 1, flags=lstm_hip.PAD_HIDDEN)
    L.set_params(P)
    ones = np.ones(table.shape[0], np.uint8)
    for kw in (dict(temperature=1.0), dict(temperature=0.7, **FILTERS), dict(temperature=0.0)):
        run = lambda acc: _seven(L.generate(prompts, count=Cn, u=u, h0=h0, c0=c0, score=True, info=True, constraint=table, accept=acc, **kw))
        assert _same(run(None), run(ones)), kw
    L.close()


def test_streams_under_a_compiled_pattern_are_whole_matches():
    import lstm_hip
    N, K = 128, 64
    table, accept = lstm_hip.dfa_regex(b"[ab]{1,3}", stop_byte=10)
    P = sr.peaked_params(N, seed=21, scale=0.1)
    h0, c0 = _state(K, N, seed=22)
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(P)
    for Cn in (2, 4, 7):
        u = np.random.RandomState(23 + Cn).random_sample((Cn, K))
        kw = dict(count=Cn, u=u, temperature=1.5, h0=h0, c0=c0, stop_byte=10, info=True, constraint=table)
        got = L.generate(accept=accept, **kw)
        language = dict(bcr.strings(table, 0, Cn, 10, accept))
        assert language and all(re.fullmatch(rb"[ab]{1,3}\n", t) for t in language)
        texts = set()
        for s in range(K):
            n = int(got[4]["out_len"][s])
            text = got[0][:n, s].tobytes()
            assert text in language and not got[0][n:, s].any(), (Cn, s, text)
            assert got[4]["end_state"][s] == language[text] and accept[got[4]["end_state"][s]]
            assert (got[4]["kept"][:n, s] >= 1).all() and (got[4]["kept"][:n, s] <= 3).all() and not got[4]["kept"][n:, s].any()
            texts.add(text)
        assert len(texts) >= 2  # (the draws do decide)
        if Cn == 2:  # the same draws without accepting states: some stream is cut off inside the pattern
            free = L.generate(**kw)
            inside = [s for s in range(K) if not accept[free[4]["end_state"][s]]]
            print(f"count 2 without accepting states: {len(inside)} of {K} streams end inside the pattern")
            assert len(inside) >= 1
    L.close()


@pytest.mark.parametrize("tau", [1.0, 1.7, 0.0])
def test_a_language_with_one_string_of_that_length_forces_it(tau):
    import lstm_hip
    N, K, Cn = 100, 6, 5
    table, accept = lstm_hip.dfa_regex(b"hello|[a-z]{1,4}|[a-z]{6,}")  # (no match ends where nothing can follow: no empty row)
    assert table.shape[0] > 6 and cr.counts(table)[0] == 26  # the table alone allows every letter
    P = sr.peaked_params(N, seed=31, scale=0.1)
    h0, c0 = _state(K, N, seed=32)
    u = np.random.RandomState(33).random_sample((Cn, K))
    L = lstm_hip.Lstm(N, 2, 1, flags=lstm_hip.PAD_HIDDEN)
    L.set_params(P)
    got = L.generate(count=Cn, u=u, temperature=tau, h0=h0, c0=c0, info=True, constraint=table, accept=accept, **(FILTERS if tau == 1.7 else {}))
    for s in range(K):
        assert got[0][:, s].tobytes() == b"hello" and got[4]["out_len"][s] == Cn and accept[got[4]["end_state"][s]]
    assert (got[4]["kept"] == 1).all()
    # after the prompt "he" three more bytes are forced too; four are not
    got = L.generate([b"he"] * K, count=3, u=u[:3], temperature=tau, info=True, constraint=table, accept=accept)
    assert all(got[0][:, s].tobytes() == b"llo" for s in range(K))
    L.close()


@pytest.mark.parametrize("name", dr.ORACLE_TABLES)
@pytest.mark.parametrize("top_k,top_p,tau", cr.ORACLE_SETTINGS)
def test_outputs_are_accepted_and_match_the_oracle(top_k, top_p, tau, name, oracle32):
    """The structure and thresholds of test_utf8_outputs_are_valid_and_match_the_oracle (tests/test_constraint.py), the float64
    reference masking with the bytes that exist; ambiguous draws (their share on oracle trajectories is what
    tests/test_accepting_cpu.py controls) are skipped, at most 5 % of them."""
    import lstm_hip
    P, prompts, u, table, accept, stop = dr.oracle_case(name, lstm_hip.dfa_utf8())
    N, K, Cn = sr.ORACLE_N, len(prompts), dr.ORACLE_COUNT
    F = dr.f_table(table, accept, stop, Cn)
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(P)
    out, _, _, _, info = L.generate(prompts, count=Cn, u=u, temperature=tau, top_k=top_k, top_p=top_p, info=True, constraint=table,
                                    accept=accept, stop_byte=None if stop < 0 else stop)
    L.close()
    kept = info["kept"]
    skipped = checked = inside = near = late = draws = 0
    drawing = set()
    for s in range(K):
        q = cr.walk(table, 0, prompts[s])
        n = int(info["out_len"][s])
        assert cr.walk(table, q, out[:n, s]) == info["end_state"][s] and accept[info["end_state"][s]], s
        assert n == Cn or out[n - 1, s] == stop
        p1 = sr.replay(oracle32, N, P, prompts[s], out[:n, s])
        for i in range(n):
            R = Cn - i
            drawing.add(q)
            late += R <= 3
            draws += 1
            x = int(out[i, s])
            ex = dr.exists(table, accept, F, stop, q, R)
            assert ex[x] and 1 <= int(kept[i, s]) <= ex.sum(), (s, i, x)
            keep, mask, pp, p = dr.filter64(p1[i], table, accept, F, stop, q, R, tau, top_k, top_p)
            if dr.ambiguous(p, table, accept, F, stop, q, R, top_k, top_p):
                skipped += 1
            else:
                assert mask[x], (s, i, x, keep)
                assert int(kept[i, s]) == keep, (s, i, int(kept[i, s]), keep)
                lo = pp[:x].sum()
                hi = lo + pp[x]
                checked += 1
                inside += lo <= u[i, s] < hi
                near += lo - 1e-5 <= u[i, s] < hi + 1e-5
            q = int(table[q, x])
    print(f"{name} top_k {top_k} top_p {top_p} tau {tau}: draws {draws}, skipped {skipped}, checked {checked}, inside {inside}, "
          f"near {near}, drawing states {sorted(drawing)}, draws with R <= 3: {late}")
    assert skipped <= 0.05 * draws, skipped
    assert inside >= 0.99 * checked and near == checked, (inside, near, checked)
    assert drawing == set(range(table.shape[0])) and late >= 1


@pytest.mark.parametrize("kind", ["plain", "padded", "average"])
def test_wide_batches_match_small_batches(kind):
    """gen_head puts 4 streams into one workgroup at 1030 streams: under the deadline every stream must come out as it does in
    a batch of 5 (one stream per workgroup) -- bytes, kept counts, lengths, final and end states.  Prompts differ in length, so
    the streams of one workgroup stand at different distances from their deadline."""
    import lstm_hip
    table = lstm_hip.dfa_utf8()
    accept = np.zeros(8, np.uint8)
    accept[0] = 1
    N, K, Cn = (30 if kind == "padded" else 32), 1030, 12
    rs = np.random.RandomState(41)
    P = sr.peaked_params(N, seed=42)
    start = rs.randint(0, 8, size=K).astype(np.int32)
    start[:8] = np.arange(8)
    pieces = ([], [0x41], [0xC3], [0xE2, 0x82])  # (from the character boundary only: a prompt must walk the table)
    prompts = [np.array(pieces[i % 4 if q == 0 else 0], np.uint8) for i, q in enumerate(start)]
    assert len({len(p) for p in prompts}) == 3
    h0, c0 = _state(K, N, seed=43)
    u = rs.random_sample((Cn, K))
    L = lstm_hip.Lstm(N, 2, 1, flags=lstm_hip.PAD_HIDDEN if kind == "padded" else 0)
    if kind == "average":  # the average as the inference source equals a second handle loaded with the average
        L.set_params(sr.peaked_params(N, seed=44))
        L.set_averaging(lstm_hip.AVG_EMA, 0.9, 1)
        L.set_average(P)
        L.set_averaging_counts(1, 1)
        L.set_inference_source(lstm_hip.SRC_AVERAGE)
    else:
        L.set_params(P)
    kw = dict(count=Cn, temperature=0.9, info=True, constraint=table, accept=accept, **FILTERS)
    wide = L.generate(prompts, u=u, h0=h0, c0=c0, start_state=start, **kw)
    assert (accept[wide[4]["end_state"]] == 1).all() and (wide[4]["out_len"] == Cn).all()
    if kind == "average":
        twin = lstm_hip.Lstm(N, 2, 1)
        twin.set_params(P)
        other = twin.generate(prompts, u=u, h0=h0, c0=c0, start_state=start, **kw)
        twin.close()
        assert all(np.array_equal(wide[i], other[i]) for i in (0, 2, 3)) and _same(wide[4], other[4], NAMES[4:])
    pick = np.unique(np.concatenate([np.arange(40), np.arange(K - 40, K), rs.choice(K, 30, replace=False)]))
    for g in (pick[i:i + 5] for i in range(0, pick.size, 5)):
        small = L.generate([prompts[s] for s in g], u=u[:, g], h0=h0[g], c0=c0[g], start_state=start[g], **kw)
        assert np.array_equal(wide[0][:, g], small[0]), g
        assert np.array_equal(wide[2][g], small[2]) and np.array_equal(wide[3][g], small[3]), g
        assert all(np.array_equal(np.asarray(wide[4][k])[..., g], small[4][k]) for k in NAMES[4:]), g
    L.close()


def test_non_finite_parameters_still_end_in_accepting_states():
    """The documented contract, as for the other heads: with a NaN row in Why the call returns 0, the output walks the table
    and every stream ends in an accepting state."""
    import lstm_hip
    from oracle_lib import split_params
    N, K, Cn = 64, 16, 9
    table = lstm_hip.dfa_utf8()
    accept = np.zeros(8, np.uint8)
    accept[0] = 1
    P = np.array(sr.peaked_params(N, seed=51), np.float32, copy=True)
    split_params(P, N)["Why"][7] = np.nan  # (a view into P) byte 7 is allowed at a character boundary: its logit is NaN there
    assert np.isnan(P).sum() == N
    rs = np.random.RandomState(52)
    start = (np.arange(K) % 8).astype(np.int32)
    u = rs.random_sample((Cn, K))
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(P)
    got = L.generate(count=Cn, u=u, temperature=1.0, info=True, constraint=table, accept=accept, start_state=start)
    L.close()
    for s in range(K):
        n = int(got[4]["out_len"][s])
        assert n == Cn and cr.walk(table, int(start[s]), got[0][:n, s]) == got[4]["end_state"][s] == 0, s


def test_beam_search_under_a_compiled_pattern_returns_the_brute_force_best():
    import lstm_hip
    N, W, Cn = 64, 8, 4
    table, accept = lstm_hip.dfa_regex(b"[ab]{1,2}|c", stop_byte=10)
    L = lstm_hip.Lstm(N, 2, 1, flags=lstm_hip.STABLE_SOFTMAX)
    L.set_params(bcr.control_params())
    found = bcr.strings(table, 0, Cn, 10, accept)
    assert sorted(t for t, _ in found) == sorted(x + b"\n" for x in (b"a", b"b", b"c", b"aa", b"ab", b"ba", b"bb"))
    sc = L.score([t for t, _ in found], constraint=table, first=True)
    rows = []
    for (t, q), sur in zip(found, sc["surprisal"]):
        total = 0.0
        for v in sur:
            total += float(v)
        rows.append((total, t, q))
    want = sorted(rows)
    res, raw = L.beam_search([b""], count=Cn, beams=W, stop_byte=10, trace=True, constraint=table, accept=accept)
    L.close()
    finite = [(t, b) for t, b in res[0] if np.isfinite(b)]
    assert [t for t, _ in finite] == [t for _, t, _ in want]
    assert np.array([b for _, b in finite]).tobytes() == np.array([c for c, _, _ in want]).tobytes()
    assert all(accept[q] for q in raw["end_state"][0, :len(want)]) and res[0][len(want):] == [(b"", float("inf"))]


def test_program_draws_and_searches_under_a_pattern(tmp_path):
    rs = np.random.RandomState(61)
    corpus = tmp_path / "corpus.txt"
    lines = ["%03d-%04d" % (rs.randint(1000), rs.randint(10000)) if rs.rand() < 0.7 else rs.choice(["één", "zwölf", "abc"]) for _ in range(400)]
    corpus.write_text("\n".join(lines) + "\n", encoding="utf-8")
    tr = subprocess.run([LSTM, str(corpus), "64", "8", "4", "0.1", "--epochs", "1", "--windows", "60", "--sample", "0",
                         "--save", str(tmp_path / "ck"), "--quiet"], capture_output=True, text=True, errors="replace", timeout=300)
    assert tr.returncode == 0, tr.stderr
    run = lambda *extra: subprocess.run([GEN, "--load", str(tmp_path / "ck"), "--seed", "3", *extra], capture_output=True, timeout=300)
    texts = lambda o: [t[:-1] for t in re.split(rb"== sample \d+[^\n]*==\n", o.stdout)[1:]]  # (the program's own newline)
    phone = "[0-9]{3}-[0-9]{4}"
    r = run("--regex", phone, "--stop-byte", "10", "--streams", "16", "--count", "12", "--temperature", "1.5")
    assert r.returncode == 0, r.stderr
    assert len(texts(r)) == 16 and all(re.fullmatch(rb"[0-9]{3}-[0-9]{4}\n", t) for t in texts(r)), texts(r)
    assert len(set(texts(r))) > 1
    short = run("--regex", phone, "--stop-byte", "10", "--count", "8")  # the match and its stop byte need nine
    assert short.returncode == 1 and b"no accepted string of 8 bytes or fewer" in short.stderr, short.stderr
    exact = run("--regex", "[a-z]{2,}|" + phone + "[0-9]*", "--count", "8", "--streams", "8", "--temperature", "2")  # no stop byte: exactly --count
    assert exact.returncode == 0 and all(re.fullmatch(rb"[a-z]{8}|[0-9]{3}-[0-9]{4}", t) for t in texts(exact)), (texts(exact), exact.stderr)
    assert len(texts(exact)) == 8
    ends = run("--regex", phone, "--count", "8")  # without a stop byte a match must be one that can go on
    assert ends.returncode == 1 and b"--regex without --stop-byte" in ends.stderr and b"give --stop-byte" in ends.stderr, ends.stderr
    wide = run("--regex", "[a-z\\x80-\\xff]+", "--utf8", "--count", "10", "--streams", "8", "--temperature", "2")
    assert wide.returncode == 0, wide.stderr
    assert len(texts(wide)) == 8
    for t in texts(wide):
        assert len(t) == 10 and len(t.decode("utf-8", "strict")) <= 10 and all(b >= 0x80 or 0x61 <= b <= 0x7A for b in t), t
    search = lambda *extra: subprocess.run([GEN, "--load", str(tmp_path / "ck"), *extra], capture_output=True, timeout=300)
    beams = search("--regex", phone, "--stop-byte", "10", "--count", "12", "--beams", "4", "--nbest", "4", "--constrain-search")
    assert beams.returncode == 0, beams.stderr
    assert 1 <= len(texts(beams)) <= 4 and all(re.fullmatch(rb"[0-9]{3}-[0-9]{4}\n", t) for t in texts(beams)), texts(beams)
    assert search("--regex", phone, "--count", "8", "--beams", "4").returncode == 2  # not without --constrain-search
    bad = run("--regex", "[0-9]{3}-[0-9]{4", "--count", "8")
    assert bad.returncode == 1 and b"{ at byte 14 does not start a quantifier" in bad.stderr, bad.stderr
