"""-m gpu: lstm_hip_beam_search_constrained (include/lstm_hip.h).

Under a table that allows everything the call is lstm_hip_beam_search, bit for bit; against the float64 rule through the
oracle (tests/beam_constraint_ref.py, whose margins tests/test_beam_constraint_cpu.py controls) hypotheses, lengths and end
states are equal and costs agree within 1e-4 bits; a hypothesis's cost is the double sum of the surprisals the
LSTM_HIP_STABLE_SOFTMAX scorer gives its bytes under the same table, bit for bit; and on tables that accept at most W strings
the search returns all of them in the order of their costs, then slots that stand for no hypothesis."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import beam_constraint_ref as bcr
import beam_ref as br
import constraint_ref as cr
from test_beam_search import _handle, _params, _prompts, _state, _trainer
from test_pad_hidden import pad_cols, pad_params, padded_width

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def _utf8():
    import lstm_hip
    t = lstm_hip.dfa_utf8()
    acc = np.zeros(t.shape[0], np.uint8)
    acc[0] = 1
    return t, acc


def _same(a, b, names=("out", "out_len", "parent", "byte", "end_state")):
    assert a["bits"].tobytes() == b["bits"].tobytes(), (a["bits"], b["bits"])
    for name in names:
        if name in a or name in b:
            assert np.array_equal(a[name], b[name]), name


@pytest.mark.parametrize("W", [1, 4, 5])
def test_a_table_that_allows_everything_is_the_unconstrained_search(W):
    N, count = 64, 12
    prompts = _prompts([0, 3, 5], seed=3)
    h0, c0 = _state(3, N, seed=4)
    L = _handle(N, br.control_params())
    for stop in (-1, 101):
        _, free = L.beam_search(prompts, count=count, beams=W, stop_byte=stop, h0=h0, c0=c0, trace=True)
        _, got = L.beam_search(prompts, count=count, beams=W, stop_byte=stop, h0=h0, c0=c0, trace=True,
                               constraint=bcr.trivial_table())
        assert np.isfinite(free["bits"]).all()  # (W candidates of finite cost at every selection: absent slots never show)
        _same(free, got, ("out", "out_len", "parent", "byte"))
        assert not got["end_state"].any()
    L.close()


@pytest.mark.parametrize("name", bcr.ORACLE_TABLES)
@pytest.mark.parametrize("W", br.CONTROL_BEAMS)
def test_hypotheses_against_the_float64_rule(W, name, oracle64):
    import lstm_hip
    utf8 = lstm_hip.dfa_utf8()
    N, count, P = br.CONTROL_N, br.CONTROL_COUNT, bcr.control_params()
    prompts = [np.array([b], np.uint8) for b in br.CONTROL_PROMPTS]
    table, accept, stop = bcr.oracle_table(name, utf8)
    L = _handle(N, P)
    got, raw = L.beam_search(prompts, count=count, beams=W, stop_byte=stop, trace=True, constraint=table, accept=accept)
    L.close()
    worst, inside = 0.0, 0
    for s, p in enumerate(prompts):
        want = bcr.beam64(oracle64, N, P, p, W, count, table, 0, stop, accept)
        assert [t for t, _ in got[s]] == want["hyps"], s
        assert list(raw["out_len"][s]) == want["length"] and list(raw["end_state"][s]) == want["state"], s
        diff = np.abs(raw["bits"][s] - np.array(want["bits"])).max()
        print("stream %d: largest cost difference to float64 %.3g bits" % (s, diff))
        worst = max(worst, diff)
        assert diff <= 1e-4, (s, diff)
        inside += sum(q != 0 for q in want["state"])
    # what the case is for, by the reference (tests/test_beam_constraint_cpu.py asserts both over all cases; here once, on
    # the widest search): the unconstrained search of these prompts returns text that is not well-formed UTF-8, and the UTF-8
    # search without accepting states ends hypotheses inside a character (with them, none)
    if name == "utf8" and W == 8:
        assert inside >= 1
        assert any(not bcr.well_formed_utf8(t, utf8) for p in prompts for t in br.beam64(oracle64, N, P, p, W, count)["hyps"])
    if name == "utf8_accept":
        assert inside == 0


@pytest.mark.parametrize("name", ["utf8_accept", "ascii_stop", "utf8"])
def test_costs_are_the_constrained_scorers_sums(name):
    import lstm_hip
    N, W, count = br.CONTROL_N, 4, 16
    table, accept, stop = bcr.oracle_table(name, lstm_hip.dfa_utf8())
    prompts = [np.array([b], np.uint8) for b in br.CONTROL_PROMPTS] + [np.frombuffer(b"a b" if name == "ascii_stop" else "aé".encode(), np.uint8)]
    L = _handle(N, bcr.control_params(), flags=lstm_hip.STABLE_SOFTMAX)
    res, raw = L.beam_search(prompts, count=count, beams=W, stop_byte=stop, trace=True, constraint=table, accept=accept)
    texts = [bytes(prompts[s]) + t for s in range(len(prompts)) for t, _ in res[s]]
    sc = L.score(texts, constraint=table)
    L.close()
    assert np.isfinite(raw["bits"]).all()
    for i, text in enumerate(texts):
        s, r = divmod(i, W)
        total = 0.0
        for v in sc["surprisal"][i][len(prompts[s]):]:
            total += float(v)
        assert np.float64(total).tobytes() == raw["bits"][s, r].tobytes(), (s, r, total, raw["bits"][s, r])
        assert sc["end_state"][i] == raw["end_state"][s, r], (s, r)


def _brute(L, table, found, first):
    """the accepted strings in the order of their costs: [(bits, bytes, end state)], costs by the scorer under the table"""
    sc = L.score([t for t, _ in found], constraint=table, first=first)
    rows = []
    for (t, q), sur in zip(found, sc["surprisal"]):
        total = 0.0
        for v in sur:
            total += float(v)
        rows.append((total, t, q))
    return sorted(rows)


def test_a_search_wider_than_the_language_returns_all_of_it_in_cost_order():
    import lstm_hip
    N = 64
    L = _handle(N, bcr.control_params(), flags=lstm_hip.STABLE_SOFTMAX)
    chain = bcr.chain_table([(97, 0xC3), (98, 120), (32, 0xA9), (101, 10)])  # five states, two bytes per position
    want = _brute(L, chain, bcr.strings(chain, 0, 4), True)
    assert len(want) == 16
    for W in (16, 32):
        res, raw = L.beam_search([b""], count=4, beams=W, trace=True, constraint=chain)
        assert [t for t, _ in res[0][:16]] == [t for _, t, _ in want]
        assert raw["bits"][0, :16].tobytes() == np.array([c for c, _, _ in want]).tobytes()
        assert list(raw["end_state"][0, :16]) == [4] * 16 and list(raw["out_len"][0, :16]) == [4] * 16
        # then slots that stand for no hypothesis
        assert list(raw["bits"][0, 16:]) == [INF] * (W - 16) and not raw["out_len"][0, 16:].any()
        assert not raw["end_state"][0, 16:].any() and not raw["out"][0, 16:].any()
    table, accept = bcr.pattern_ab_newline()  # [ab]{1,3}\n
    want = _brute(L, table, bcr.strings(table, 0, 5, 10, accept), True)
    assert len(want) == 14
    res, raw = L.beam_search([b""], count=5, beams=16, stop_byte=10, trace=True, constraint=table, accept=accept)
    L.close()
    assert [t for t, _ in res[0][:14]] == [t for _, t, _ in want]
    assert all(t.endswith(b"\n") and 2 <= len(t) <= 4 and re.fullmatch(rb"[ab]{1,3}\n", t) for t, _ in res[0][:14])
    assert raw["bits"][0, :14].tobytes() == np.array([c for c, _, _ in want]).tobytes()
    assert list(raw["end_state"][0]) == [4] * 14 + [0, 0] and list(raw["out_len"][0, 14:]) == [0, 0]
    assert list(raw["bits"][0, 14:]) == [INF, INF] and res[0][14:] == [(b"", INF)] * 2


def test_a_stream_alone_and_in_a_batch():
    N, W, count = 64, 8, 12
    table, accept = _utf8()
    # other start states, other prompt lengths: a prompt continues the character its start state is in
    prompts = [b"", b"\xa9abc", b"\x80", "héllo".encode(), b"\x9f\x80"]
    start = [0, 1, 5, 0, 4]  # (the third stream's prompt ends inside a character: its slots start in state 2)
    h0, c0 = _state(len(prompts), N, seed=13)
    L = _handle(N, bcr.control_params())
    _, wide = L.beam_search(prompts, count=count, beams=W, stop_byte=32, h0=h0, c0=c0, trace=True, constraint=table,
                            accept=accept, start_state=start)
    assert not wide["end_state"][np.isfinite(wide["bits"])].any()
    for k in range(len(prompts)):
        _, one = L.beam_search(prompts[k:k + 1], count=count, beams=W, stop_byte=32, h0=h0[k:k + 1], c0=c0[k:k + 1], trace=True,
                               constraint=table, accept=accept, start_state=start[k:k + 1])
        assert wide["bits"][k].tobytes() == one["bits"][0].tobytes(), k
        for name in ("out", "out_len", "end_state"):
            assert np.array_equal(wide[name][k], one[name][0]), (k, name)
        for name in ("parent", "byte"):
            assert np.array_equal(wide[name][:, k * W:(k + 1) * W], one[name]), (k, name)
    L.close()


def test_the_widest_beam_at_the_lds_limit_alone_and_in_a_batch():
    """N = 512 with 32 beams: 64 KB of h in LDS"""
    import sampling_ref as sr
    N, W, count = 512, 32, 4
    table, accept = _utf8()
    prompts, start = [b"\xa9", b"ab"], [1, 0]
    L = _handle(N, sr.peaked_params(N, seed=43, scale=0.05, gain=4.0))
    _, wide = L.beam_search(prompts, count=count, beams=W, trace=True, constraint=table, accept=accept, start_state=start)
    assert np.isfinite(wide["bits"]).all() and not wide["end_state"].any()
    for k in range(2):
        _, one = L.beam_search(prompts[k:k + 1], count=count, beams=W, trace=True, constraint=table, accept=accept,
                               start_state=start[k:k + 1])
        assert wide["bits"][k].tobytes() == one["bits"][0].tobytes(), k
        assert np.array_equal(wide["out"][k], one["out"][0]) and np.array_equal(wide["end_state"][k], one["end_state"][0]), k
        assert len(set(one["out"][0].tobytes()[i * count:(i + 1) * count] for i in range(W))) == W
    L.close()


def test_bf16_padded_and_step_kernel_handles_match_their_twins():
    import lstm_hip
    W, count = 4, 20
    table, accept = _utf8()
    prompts = _prompts([0, 4, 30, 1], seed=51)

    def run(N, P, flags, B, h0, c0):
        L = _handle(N, P, flags=flags, B=B)
        res, raw = L.beam_search(prompts, count=count, beams=W, h0=h0, c0=c0, trace=True, constraint=table, accept=accept)
        L.close()
        return res, raw["end_state"].tolist()
    N = 256
    P = _params(N, seed=53, scale=0.1)
    h0, c0 = _state(4, N, seed=54)
    assert run(N, P, 0, 8, h0, c0) == run(N, P, lstm_hip.BF16_RECURRENCE, 8, h0, c0)
    N = 64
    P = bcr.control_params()
    h0, c0 = _state(4, N, seed=55)
    assert run(N, P, 0, 1, h0, c0) == run(N, P, lstm_hip.STEP_KERNELS, 1, h0, c0)
    N = 50
    Np = padded_width(N, lstm_hip.PAD_HIDDEN)
    P = _params(N, seed=56, scale=0.3)
    h0, c0 = _state(4, N, seed=57)
    assert run(N, P, lstm_hip.PAD_HIDDEN, 1, h0, c0) == run(Np, pad_params(P, N, Np), 0, 1, pad_cols(h0, N, Np), pad_cols(c0, N, Np))


def test_training_state_is_untouched_by_a_constrained_search():
    import lstm_hip
    N, S, B = 64, 8, 4
    table, accept = _utf8()
    text = np.random.RandomState(61).randint(97, 123, size=5000).astype(np.uint8)
    A, Bh = _trainer(text, N, S, B), _trainer(text, N, S, B)
    la = [A.train_windows(5, 0.1)]
    A.beam_search(_prompts([3, 40], seed=62), count=30, beams=5, stop_byte=101, constraint=table, accept=accept)
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
    import lstm_hip
    N = 64
    L = _handle(N, bcr.control_params())
    lib = L.lib
    big = 1 << 16
    out, n_out, bits, ends = np.zeros(big + 64, np.uint8), np.zeros(64, np.int32), np.zeros(64, np.float64), np.zeros(64, np.int32)
    op, lp, bp, ep = (out.ctypes.data_as(C.POINTER(C.c_uint8)), n_out.ctypes.data_as(C.POINTER(C.c_int32)),
                      bits.ctypes.data_as(C.POINTER(C.c_double)), ends.ctypes.data_as(C.POINTER(C.c_int32)))
    u16 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint16))
    utf8, acc8 = _utf8()
    pat, pat_acc = bcr.pattern_ab_newline()
    bad_entry = utf8.copy()
    bad_entry[3, 0xA0] = 8
    empty = utf8.copy()
    empty[2] = 0xFFFF                       # a state that can be reached and allows nothing
    wide = np.zeros((4096, 256), np.uint16)  # 4096 states, everything allowed
    wide_acc = np.ones(4096, np.uint8)
    prompt = np.frombuffer(b"a\xffb", np.uint8).copy()
    off = np.array([0, 3], np.uint64)
    three, minus = np.array([8], np.int32), np.array([-1], np.int32)
    keep = []

    def con(table, states=None, size=None, null=False):
        c = lstm_hip._Constraint(C.sizeof(lstm_hip._Constraint) if size is None else size,
                                 table.shape[0] if states is None else states, None if null else u16(table))
        keep.append((c, table))
        return c

    def bc(c, accept=None, size=None):
        b = lstm_hip._BeamConstraint(C.sizeof(lstm_hip._BeamConstraint) if size is None else size,
                                     C.pointer(c) if c is not None else None,
                                     accept.ctypes.data_as(C.POINTER(C.c_uint8)) if accept is not None else None)
        keep.append((b, accept))
        return b
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    cases = [  # (beam constraint, start_state, end_state, count, stop, prompts?, what the message says)
        (None, i32(three), None, 4, -1, False, "without a constraint"),
        (None, None, ep, 4, -1, False, "without a constraint"),
        (bc(con(utf8), size=8), None, ep, 4, -1, False, "beam constraint of 8 bytes"),
        (bc(None), None, ep, 4, -1, False, "null constraint"),
        (bc(con(utf8, size=12)), None, ep, 4, -1, False, "constraint of 12 bytes"),
        (bc(con(utf8, states=0)), None, ep, 4, -1, False, "states must be in"),
        (bc(con(utf8, states=4097)), None, ep, 4, -1, False, "states must be in"),
        (bc(con(utf8, null=True)), None, ep, 4, -1, False, "null table"),
        (bc(con(bad_entry)), None, ep, 4, -1, False, "neither a state"),
        (bc(con(utf8)), i32(three), ep, 4, -1, False, "start_state[0] = 8"),
        (bc(con(utf8)), i32(minus), ep, 4, -1, False, "start_state[0] = -1"),
        (bc(con(empty)), None, ep, 4, -1, False, "has no allowed byte"),
        (bc(con(utf8)), None, ep, 4, -1, True, "stream 0: prompt byte 0xff at offset 1"),
        (bc(con(utf8), acc8), i32(np.array([5], np.int32)), ep, 2, -1, False, "stream 0: no accepted string of 2 bytes"),
        (bc(con(pat), pat_acc), None, ep, 1, 10, False, "stream 0: no accepted string of 1 bytes"),  # the shortest has two
        (bc(con(pat), pat_acc), None, ep, 0, 10, False, "stream 0: no accepted string of 0 bytes"),  # count 0: q0 must accept
        (bc(con(wide), wide_acc), None, ep, big, -1, False, "above 2^28"),
    ]
    good = lstm_hip._Beam(C.sizeof(lstm_hip._Beam), 1, -1)
    for i, (b, q0, q1, count, stop, with_prompt, says) in enumerate(cases):
        opt = lstm_hip._Beam(C.sizeof(lstm_hip._Beam), 1, stop)
        rc = lib.lstm_hip_beam_search_constrained(
            L._h, 1, prompt.ctypes.data_as(C.POINTER(C.c_uint8)) if with_prompt else None,
            off.ctypes.data_as(C.POINTER(C.c_uint64)) if with_prompt else None, None, None, C.byref(opt), count, op, lp, bp, None,
            None, C.byref(b) if b is not None else None, q0, q1)
        msg = lib.lstm_hip_last_error().decode()
        assert rc == lstm_hip.EINVAL, (i, rc, msg)
        assert msg.startswith("beam_search:") and says in msg, (i, msg)
        # ... and the same handle searches at once
        ok = bc(con(utf8), acc8)
        assert lib.lstm_hip_beam_search_constrained(L._h, 1, None, None, None, None, C.byref(good), 3, op, lp, bp, None, None,
                                                    C.byref(ok), None, ep) == 0, (i, lib.lstm_hip_last_error())
        assert n_out[0] == 3 and ends[0] == 0 and np.isfinite(bits[0]), i
    # the refusals of lstm_hip_beam_search hold with a constraint, and count 0 returns the start
    bad = lstm_hip._Beam(C.sizeof(lstm_hip._Beam), 33, -1)
    ok = bc(con(utf8), acc8)
    assert lib.lstm_hip_beam_search_constrained(L._h, 1, None, None, None, None, C.byref(bad), 3, op, lp, bp, None, None,
                                                C.byref(ok), None, ep) == lstm_hip.EINVAL
    four = lstm_hip._Beam(C.sizeof(lstm_hip._Beam), 4, -1)
    seven = np.array([7], np.int32)
    plain = bc(con(utf8))
    assert lib.lstm_hip_beam_search_constrained(L._h, 1, None, None, None, None, C.byref(four), 0, None, lp, bp, None, None,
                                                C.byref(plain), i32(seven), ep) == 0
    assert list(ends[:4]) == [7] * 4 and list(n_out[:4]) == [0] * 4 and list(bits[:4]) == [0.0, INF, INF, INF]
    res, info = L.beam_search([b"ab"], count=5, beams=31, constraint=utf8, accept=acc8)  # (no trace: the end states come anyway)
    assert info["end_state"].shape == (1, 31) and not info["end_state"][np.isfinite(info["bits"])].any()
    assert len(res[0]) == 31 and all(bcr.well_formed_utf8(t, utf8) for t, _ in res[0])
    L.close()


def test_non_finite_parameters_still_give_bytes_and_states_inside_the_tables():
    N, W, count = 64, 8, 10
    table, accept = _utf8()
    P = bcr.control_params().copy()
    P[-256 + 7] = np.nan      # by[7]: every cost is NaN
    P[-256 + 9] = np.inf
    P[-256 + 0xC3] = np.inf
    L = _handle(N, P)
    prompts = [np.array([b], np.uint8) for b in br.CONTROL_PROMPTS]
    for acc in (accept, None):
        res, raw = L.beam_search(prompts, count=count, beams=W, stop_byte=10, trace=True, constraint=table, accept=acc)
        assert raw["parent"].max() < W and raw["out_len"].max() <= count and raw["out_len"].min() >= 0
        assert raw["end_state"].min() >= 0 and raw["end_state"].max() < table.shape[0]
        for s in range(4):
            for r, (t, b) in enumerate(res[s]):
                assert len(t) <= count
                if np.isfinite(b):  # still a walk of the table, ending where the call says (accepting, if asked for)
                    assert cr.walk(table, 0, t) == raw["end_state"][s, r] and (acc is None or acc[raw["end_state"][s, r]])
    L.close()


LSTM = os.path.join(ROOT, "eigen-lstm_amd", "lstm")
GEN = os.path.join(ROOT, "eigen-lstm_amd", "lstm_generate")


def test_program_searches_under_the_constraint_options(tmp_path):
    """lstm_generate --beams W --constrain-search with --utf8 / --allow / --ban (without --constrain-search the program
    refuses the three with --beams, as tests/test_constraint_cpu.py requires)"""
    rs = np.random.RandomState(81)
    corpus = tmp_path / "corpus.txt"
    letters = ["a", "b", "c", "d", " ", "é", "ü", "€"]  # one-, two- and three-byte characters
    corpus.write_text("".join(letters[i] for i in rs.randint(0, len(letters), size=2500)), encoding="utf-8")
    tr = subprocess.run([LSTM, str(corpus), "64", "8", "4", "0.1", "--epochs", "1", "--windows", "30", "--sample", "0",
                         "--save", str(tmp_path / "ck"), "--quiet"], capture_output=True, text=True, errors="replace", timeout=300)
    assert tr.returncode == 0, tr.stderr
    run = lambda *extra: subprocess.run([GEN, "--load", str(tmp_path / "ck"), "--count", "21", "--streams", "2", "--prime", "ab ",
                                         *extra], capture_output=True, timeout=300)
    texts = lambda o: re.split(rb"== sample \d+[^\n]*==\n", o.stdout)[1:]
    beams = run("--beams", "4", "--nbest", "4", "--utf8", "--constrain-search")
    assert beams.returncode == 0, beams.stderr
    assert len(texts(beams)) == 8
    for t in texts(beams):
        t.decode("utf-8")  # (raises on anything that is not well-formed)
        assert t.startswith(b"ab ") and len(t) > 4
    spec = "0x61-0x64,0x20"
    greedy, beam = run("--temperature", "0", "--allow", spec), run("--beams", "1", "--allow", spec, "--constrain-search")
    assert greedy.returncode == 0 and beam.returncode == 0, (greedy.stderr, beam.stderr)
    assert len(texts(beam)) == 2 and texts(beam) == texts(greedy)
    assert all(set(t[:-1]) <= set(b"abcd ") for t in texts(beam))
    # a table with fewer strings than beams: only the hypotheses that exist are printed
    few = run("--beams", "8", "--nbest", "8", "--allow", "0x61", "--count", "3", "--streams", "1", "--prime", "a", "--constrain-search")
    assert few.returncode == 0 and texts(few) == [b"aaaa\n"], (few.stdout, few.stderr)
    assert run("--beams", "4", "--utf8").returncode == 2  # not without --constrain-search
