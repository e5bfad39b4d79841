"""CPU: lstm_hip_dfa_regex (include/lstm_hip.h) through ctypes, against Python's re.fullmatch on
bytes patterns: the verdict of the compiled table on enumerated, random and table-walked strings, the table's own properties
(entries, trimmed, minimal by a partition refinement written here, breadth-first numbering, equal languages give equal
bytes), the terminator form, every refusal with its error_pos, sizing and the bounded blow-up.  Needs no device."""
import ctypes as C
import itertools
import re
import time
import warnings

import numpy as np
import pytest

import beam_constraint_ref as bc
import lstm_hip

FORBID = 0xFFFF

# (pattern, alphabet): at most 6 bytes, at least one of which the pattern never mentions
CASES = [
    (b"", b"ab"),
    (b"a", b"ab"),
    (b"abc", b"abcd"),
    (b"a|b", b"abc"),
    (b"[ab]", b"abc"),
    (b"a*", b"ab"),
    (b"a+", b"ab"),
    (b"aa*", b"ab"),
    (b"a?", b"ab"),
    (b"a|", b"ab"),
    (b"|a", b"ab"),
    (b"a{0,1}", b"ab"),
    (b"a{,1}", b"ab"),
    (b"a{2}", b"ab"),
    (b"a{2,}", b"ab"),
    (b"aaa*", b"ab"),
    (b"a{1,3}", b"ab"),
    (b"a{0}", b"ab"),
    (b"(ab)*", b"abc"),
    (b"(?:ab)*", b"abc"),
    (b"(a|b)*c", b"abcd"),
    (b"[ab]*c", b"abcd"),
    (b"(?:a|bc){1,2}", b"abcd"),
    (b"((a|b){2}c){1,2}", b"abcd"),
    (b"(?:(?:ab){1,2}|c){0,2}", b"abcd"),
    (b"(?:a{2}){2}", b"ab"),
    (b"a{4}", b"ab"),
    (b".", b"a\nb"),
    (b"[^\\n]", b"a\nb"),
    (b".*", b"a\nb"),
    (b"a.c", b"abc\n"),
    (b"\\d", b"09a"),
    (b"[0-9]", b"09a"),
    (b"[^\\D]", b"09a"),
    (b"\\D", b"0a\xff"),
    (b"\\w+", b"a_0 -"),
    (b"[A-Za-z0-9_]+", b"a_0 -"),
    (b"\\W", b"a_ \x80"),
    (b"\\s*", b" \t\na\x0b"),
    (b"\\S\\s", b" \ta\x0c"),
    (b"[^\\s\\d]", b" 0a\n"),
    (b"[\\d\\s]+", b" 0a\n"),
    (b"(?:\\d|\\s)+", b" 0a\n"),
    (b"[^a-c]", b"abcd\x00\xff"),
    (b"[\\x00-\\x1f]+", b"\x00\x1f a"),
    (b"[\\x80-\\xff]", b"\x7f\x80\xffa"),
    (b"\\x41\\x42", b"ABC"),
    (b"\xc3\xa9+", b"\xc3\xa9a"),
    (b"(?:\xc3\xa9)+", b"\xc3\xa9a"),
    (b"[a-]", b"a-b"),
    (b"[-a]", b"a-b"),
    (b"[a\\-]", b"a-b"),
    (b"[\\w-]", b"a-b "),
    (b"[\\]]", b"]a["),
    (b"[\\[\\]]+", b"]a["),
    (b"\\.", b".a"),
    (b"\\*\\+\\?", b"*+?a"),
    (b"\\(a\\)", b"(a)b"),
    (b"a\\|b", b"a|bc"),
    (b"\\{1\\}", b"{1}a"),
    (b"\\^\\$", b"^$a"),
    (b"\\\\", b"\\a"),
    (b"\\n\\r\\t", b"\n\r\tn"),
    (b"[\\n\\r]", b"\n\rn"),
    (b"\\f|\\v", b"\x0c\x0bfv"),
    (b"(a|b|c|d)", b"abcde"),
    (b"[a-d]", b"abcde"),
    (b"(|a)(|b)", b"abc"),
    (b"a?b?", b"abc"),
    (b"(a||b)", b"abc"),
    (b"[ab]{1,3}", b"abc"),
    (b"(a*)*", b"ab"),
    (b"(a*)+b", b"abc"),
    (b"(a|ab)(c|bcd)", b"abcde"),
    (b"(ab|a)*", b"abc"),
    (b"x{2,3}y{0,2}", b"xyz"),
    (b"[0-9]{3}-[0-9]{4}", b"05-a"),
]
# patterns with the same language: their tables must be the same bytes
EQUAL = [
    (b"a|b", b"[ab]"), (b"a+", b"aa*"), (b"a?", b"a|", b"|a", b"a{0,1}", b"a{,1}"), (b"a{2,}", b"aaa*"),
    (b"(ab)*", b"(?:ab)*"), (b"(a|b)*c", b"[ab]*c"), (b"(?:a{2}){2}", b"a{4}"), (b".", b"[^\\n]"),
    (b"\\d", b"[0-9]", b"[^\\D]"), (b"\\w+", b"[A-Za-z0-9_]+"), (b"[\\d\\s]+", b"(?:\\d|\\s)+"), (b"[a-]", b"[-a]", b"[a\\-]"),
    (b"(a|b|c|d)", b"[a-d]"), (b"(|a)(|b)", b"a?b?"), (b"a*", b"(a*)*"), (b"", b"a{0}"),
]


def test_the_case_table_is_what_the_issue_asks_for():
    assert len(CASES) >= 60 and len({p for p, _ in CASES}) == len(CASES)
    for pat, alpha in CASES:
        assert 2 <= len(set(alpha)) == len(alpha) <= 6
        assert any(bytes([b]) not in pat and b"\\x%02x" % b not in pat for b in alpha), pat
    known = {p for p, _ in CASES}
    assert all(p in known for group in EQUAL for p in group)


def accepts(table, accept, s):
    q = 0
    for b in s:
        q = int(table[q, b])
        if q == FORBID:
            return False
    return bool(accept[q])


def py(pat):
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # a pattern Python itself finds doubtful has no place in the table
        return re.compile(pat)


def distance_to_accept(table, accept):
    Q = table.shape[0]
    dist = np.where(accept != 0, 0, -1).astype(np.int64)
    for d in range(1, Q + 1):
        grew = False
        for q in range(Q):
            if dist[q] < 0 and any(nx != FORBID and dist[nx] == d - 1 for nx in set(table[q].tolist())):
                dist[q] = d
                grew = True
        if not grew:
            break
    return dist


def walked(table, accept, rs, n):
    """n strings read off the table: a random walk, then the shortest way into an accepting state"""
    dist = distance_to_accept(table, accept)
    out = []
    for _ in range(n):
        q, s = 0, []
        for _ in range(rs.randint(0, 9)):
            allowed = np.nonzero(table[q] != FORBID)[0]
            if allowed.size == 0:
                break
            b = int(rs.choice(allowed))
            s.append(b)
            q = int(table[q, b])
        while not accept[q]:
            allowed = [b for b in range(256) if table[q, b] != FORBID and dist[table[q, b]] == dist[q] - 1]
            b = int(rs.choice(allowed))
            s.append(b)
            q = int(table[q, b])
        out.append(bytes(s))
    return out


def check_properties(table, accept):
    Q = table.shape[0]
    assert 1 <= Q <= 4096 and table.shape == (Q, 256) and accept.shape == (Q,)
    assert ((table < Q) | (table == FORBID)).all() and set(accept.tolist()) <= {0, 1}
    # breadth-first numbering from state 0, bytes ascending; every state reachable
    order = [0]
    for q in order:
        for b in range(256):
            nx = int(table[q, b])
            if nx != FORBID and nx not in order:
                order.append(nx)
    assert order == list(range(Q)), order
    assert (distance_to_accept(table, accept) >= 0).all()  # every state can reach an accepting one
    # minimal: refine {accepting, not} by successor blocks until stable; every state must end alone in its block
    block = accept.astype(np.int64)
    cols = [b for b in range(256) if b == 0 or (table[:, b] != table[:, b - 1]).any()]  # (one byte per run of equal columns)
    while True:
        succ = np.where(table[:, cols] == FORBID, -1, block[np.minimum(table[:, cols], Q - 1)])
        sig = {}
        new = np.array([sig.setdefault((int(block[q]),) + tuple(succ[q].tolist()), len(sig)) for q in range(Q)])
        if len(sig) == len(set(block.tolist())):
            break
        block = new
    assert len(set(block.tolist())) == Q, "two states are equivalent"


@pytest.fixture(scope="module")
def compiled():
    return {pat: lstm_hip.dfa_regex(pat) for pat, _ in CASES}


@pytest.mark.parametrize("pat,alpha", CASES, ids=[repr(p) for p, _ in CASES])
def test_the_table_decides_as_re_fullmatch(compiled, pat, alpha):
    table, accept = compiled[pat]
    check_properties(table, accept)
    rx = py(pat)
    rs = np.random.RandomState(len(pat) * 131 + sum(pat))
    strings = [bytes(t) for n in range(5) for t in itertools.product(alpha, repeat=n)]
    strings += [bytes(rs.choice(list(alpha), size=rs.randint(0, 13)).tolist()) for _ in range(2000)]
    verdicts = set()
    for s in strings:
        want = rx.fullmatch(s) is not None
        assert accepts(table, accept, s) == want, (pat, s)
        verdicts.add(want)
    assert verdicts == {True, False}, pat
    for s in walked(table, accept, rs, 200):
        assert rx.fullmatch(s) is not None, (pat, s)


@pytest.mark.parametrize("group", EQUAL, ids=[repr(g[0]) for g in EQUAL])
def test_equal_languages_give_identical_tables(compiled, group):
    t0, a0 = compiled[group[0]]
    for pat in group[1:]:
        t, a = compiled[pat]
        assert t.tobytes() == t0.tobytes() and a.tobytes() == a0.tobytes(), pat


@pytest.mark.parametrize("pat,alpha", [(b"[ab]{1,3}", b"abc"), (b"(?:a|bc){1,2}", b"abcd"), (b"", b"ab"), (b"[^\\n]*", b"a\xff"),
                                       (b"[0-9]{3}-[0-9]{4}", b"05-a")], ids=repr)
def test_the_terminator_form(pat, alpha):
    stop = 10
    table, accept = lstm_hip.dfa_regex(pat, stop_byte=stop)
    base, _ = lstm_hip.dfa_regex(pat)
    check_properties(table, accept)
    assert table.shape[0] == base.shape[0] + 1
    (fin,) = np.nonzero(accept)[0].tolist()  # one accepting state
    assert [b for b in range(256) if table[fin, b] != FORBID] == [stop] and table[fin, stop] == fin
    assert (bc.cr.counts(table) >= 1).all()  # no empty row: the generator, the scorer and beam search take it as it is
    rx, loop = py(pat), py(b"(?:" + pat + b")\\n+")
    for n in range(6):
        for t in itertools.product(alpha + bytes([stop]), repeat=n):
            s = bytes(t)
            got = accepts(table, accept, s)
            assert got == (loop.fullmatch(s) is not None), s
            if stop not in s[:-1]:  # a stream ends at its first stop byte: the language is L followed by it
                assert got == (s[-1:] == bytes([stop]) and rx.fullmatch(s[:-1]) is not None), s


def test_the_compiled_ab_newline_accepts_what_the_hand_written_table_accepts():
    table, accept = lstm_hip.dfa_regex(b"[ab]{1,3}", stop_byte=10)
    hand, hacc = bc.pattern_ab_newline()
    seen = set()
    for n in range(7):
        for t in itertools.product(b"ab\nc", repeat=n):
            s = bytes(t)
            got = accepts(table, accept, s)
            assert got == accepts(hand, hacc, s), s
            seen.add(got)
    assert seen == {True, False}
    for count in (2, 4, 7):  # and, as a generator sees it: the same strings within a deadline
        mine = {s for s, _ in bc.strings(table, 0, count, 10, accept)}
        assert mine == {s for s, _ in bc.strings(hand, 0, count, 10, hacc)} and mine


REFUSED = [  # (pattern, error_pos)
    (b"a**", 2), (b"a*?", 2), (b"a*+", 2), (b"a+?", 2), (b"a??", 2), (b"a{2}{3}", 4), (b"a{2}?", 4), (b"a{1000}{5}", 7),
    (b"^a", 0), (b"a$", 1), (b"(?=a)", 0), (b"(?P<n>a)", 0), (b"(?i)a", 0), (b"(?", 0), (b"(a", 0), (b"a)", 1), (b"(a))", 3),
    (b"[a", 0), (b"[]a]", 1), (b"[^]a]", 2), (b"[z-a]", 1), (b"[\\d-z]", 1), (b"[a-\\d]", 3), (b"[\xe9]", 1), (b"[a-\xe9]", 3),
    (b"[a[b]", 2), (b"\\q", 0), (b"\\1", 0), (b"\\b", 0), (b"\\A", 0), (b"\\ ", 0), (b"\\\xe9", 0), (b"a\\", 1), (b"\\x4", 0),
    (b"\\xg1", 0), (b"[\\x4]", 1), (b"*a", 0), (b"(*a)", 1), (b"a|*", 2), (b"+", 0), (b"{2}", 0), (b"a{", 1), (b"a{x}", 1),
    (b"a{,}", 1), (b"a{1", 1), (b"a{3,2}", 1), (b"a{5000}", 1), (b"a{1,5000}", 1), (b"a]", 1), (b"a}", 1),
    (b"(" * 201 + b")" * 201, 200),
    (b"[^\\x00-\\xff]", -1), (b"a[^\\x00-\\xff]", -1),  # an empty language
    (b"(?:a{1000}){5}", -1),  # 5001 states
]


@pytest.mark.parametrize("pat,pos", REFUSED, ids=[repr(p[:12]) for p, _ in REFUSED])
def test_every_refusal_names_its_byte(pat, pos):
    with pytest.raises(lstm_hip.LstmHipError) as e:
        lstm_hip.dfa_regex(pat)
    assert e.value.error_pos == pos, str(e.value)
    msg = str(e.value)
    assert msg.startswith("lstm_hip error -1: dfa_regex: ")
    if pos >= 0:
        assert f"byte {pos}" in msg, msg
    lib = lstm_hip.load_library()  # error_pos may be NULL
    buf = np.frombuffer(pat, np.uint8)
    assert lib.lstm_hip_dfa_regex(buf.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_size_t(len(pat)), C.c_int32(-1), None, None,
                                  C.c_int32(0), None) == -1


def test_refusals_without_a_position_say_what_is_wrong():
    def message(pat, **kw):
        with pytest.raises(lstm_hip.LstmHipError) as e:
            lstm_hip.dfa_regex(pat, **kw)
        assert e.value.error_pos == -1
        return str(e.value)

    assert message(b"[^\\x00-\\xff]") == "lstm_hip error -1: dfa_regex: empty language: the pattern matches no string"
    assert message(b"(?:a{1000}){5}") == "lstm_hip error -1: dfa_regex: too many states: the minimal automaton has 5001, above 4096"
    assert message(b"a{4095}", stop_byte=10) == ("lstm_hip error -1: dfa_regex: too many states: the minimal automaton has 4097, "
                                                 "above 4096")
    assert message(b"a.b", stop_byte=0x41) == ("lstm_hip error -1: dfa_regex: the pattern can match the stop byte 0x41: a stream "
                                              "ends at its first drawn stop byte")
    assert "the pattern can match the stop byte 0x0a" in message(b"\\s+", stop_byte=10)
    assert message(b"a", stop_byte=256) == "lstm_hip error -1: dfa_regex: stop_byte must be -1 or in [0, 255] (got 256)"
    lstm_hip.dfa_regex(b".*", stop_byte=10)  # . never matches a newline
    lstm_hip.dfa_regex(b"a|[^\\x00-\\xff]\n", stop_byte=10)  # the newline is on a branch that trimming removes
    # cap below Q, and one array without the other
    lib = lstm_hip.load_library()
    pat = np.frombuffer(b"abc", np.uint8)
    ptr = pat.ctypes.data_as(C.POINTER(C.c_uint8))
    nxt, acc, pos = np.zeros((4, 256), np.uint16), np.zeros(4, np.uint8), C.c_int32(5)
    args = (nxt.ctypes.data_as(C.POINTER(C.c_uint16)), acc.ctypes.data_as(C.POINTER(C.c_uint8)))
    assert lib.lstm_hip_dfa_regex(ptr, C.c_size_t(3), C.c_int32(-1), None, None, C.c_int32(-3), C.byref(pos)) == 4 and pos.value == -1
    pos.value = 5
    assert lib.lstm_hip_dfa_regex(ptr, C.c_size_t(3), C.c_int32(-1), *args, C.c_int32(3), C.byref(pos)) == -1 and pos.value == -1
    assert lib.lstm_hip_last_error() == b"dfa_regex: cap 3 is below the 4 states of the result"
    assert not nxt.any()  # nothing was written
    assert lib.lstm_hip_dfa_regex(ptr, C.c_size_t(3), C.c_int32(-1), args[0], None, C.c_int32(4), None) == -1
    assert lib.lstm_hip_dfa_regex(ptr, C.c_size_t(3), C.c_int32(-1), *args, C.c_int32(4), None) == 4
    assert accepts(nxt, acc, b"abc") and not accepts(nxt, acc, b"ab")


def test_sizing():
    table, accept = lstm_hip.dfa_regex(b"a{4000}")
    assert table.shape[0] == 4001 and accept.sum() == 1 and accept[4000] == 1
    assert (table[np.arange(4000), ord("a")] == np.arange(1, 4001)).all() and (table != FORBID).sum() == 4000
    with pytest.raises(lstm_hip.LstmHipError, match="a quantifier at byte 7 follows a quantifier") as e:
        lstm_hip.dfa_regex(b"a{1000}{5}")
    assert e.value.error_pos == 7
    with pytest.raises(lstm_hip.LstmHipError, match="too many states: the minimal automaton has 5001") as e:
        lstm_hip.dfa_regex(b"(?:a{1000}){5}")
    assert e.value.error_pos == -1
    assert lstm_hip.dfa_regex(b"a{0,4095}")[0].shape[0] == 4096  # the largest result there is


@pytest.mark.parametrize("pat", [b"[ab]*a[ab]{20}", b"(?:(?:(?:a{1000}){1000}){1000}){1000}", b"(.*a){30}.{30}"], ids=repr)
def test_a_blow_up_is_refused_quickly(pat):
    t0 = time.monotonic()
    with pytest.raises(lstm_hip.LstmHipError, match="too many states") as e:
        lstm_hip.dfa_regex(pat)
    assert e.value.error_pos == -1
    assert time.monotonic() - t0 < 20.0  # (a bound on "does not hang or eat the machine", not a tuned figure)
