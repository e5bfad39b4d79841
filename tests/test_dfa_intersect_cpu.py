"""CPU: lstm_hip_dfa_intersect (include/lstm_hip.h): the product table accepts exactly what both
walks accept, by enumeration; its table has the properties of lstm_hip_dfa_regex's results; refusals.  Needs no device."""
import ctypes as C
import itertools

import numpy as np
import pytest

import lstm_hip
from test_regex_cpu import FORBID, accepts, check_properties


def both(a, acc_a, b, acc_b, s):
    ones = lambda t, acc: np.ones(t.shape[0], np.uint8) if acc is None else acc
    return accepts(a, ones(a, acc_a), s) and accepts(b, ones(b, acc_b), s)


def enumerate_against(table, accept, a, acc_a, b, acc_b, alpha, longest):
    seen = set()
    for n in range(longest + 1):
        for t in itertools.product(alpha, repeat=n):
            s = bytes(t)
            want = both(a, acc_a, b, acc_b, s)
            assert accepts(table, accept, s) == want, s
            seen.add(want)
    assert seen == {True, False}


def test_regex_and_utf8():
    utf8 = lstm_hip.dfa_utf8()
    boundary = np.zeros(8, np.uint8)
    boundary[0] = 1
    rx, acc = lstm_hip.dfa_regex(b"[a\\x80-\\xff]{1,4}")
    table, accept = lstm_hip.dfa_intersect(rx, acc, utf8, boundary)
    check_properties(table, accept)
    enumerate_against(table, accept, rx, acc, utf8, boundary, b"a\xc3\xa9\xe2\x82", 4)
    assert accepts(table, accept, "aé".encode()) and accepts(table, accept, "€a".encode()) and accepts(table, accept, "𝄞".encode())
    assert not accepts(table, accept, b"\xc3") and not accepts(table, accept, b"a\xa9")
    # the order of the operands does not matter: the numbering is canonical
    t2, a2 = lstm_hip.dfa_intersect(utf8, boundary, rx, acc)
    assert t2.tobytes() == table.tobytes() and a2.tobytes() == accept.tobytes()


def test_two_regexes():
    a, acc_a = lstm_hip.dfa_regex(b"(?:ab|c)*")
    b, acc_b = lstm_hip.dfa_regex(b"[abc]{2,5}")
    table, accept = lstm_hip.dfa_intersect(a, acc_a, b, acc_b)
    check_properties(table, accept)
    enumerate_against(table, accept, a, acc_a, b, acc_b, b"abcd", 6)
    # a language met with itself, and with everything, is itself: the same bytes
    for other, acc_o in ((a, acc_a), lstm_hip.dfa_regex(b"(?:.|\\n)*")):
        t, ac = lstm_hip.dfa_intersect(a, acc_a, other, acc_o)
        assert t.tobytes() == a.tobytes() and ac.tobytes() == acc_a.tobytes()


def test_a_null_accept_array_accepts_everywhere():
    a, acc_a = lstm_hip.dfa_regex(b"ab*c")
    b, _ = lstm_hip.dfa_regex(b"a[bc]{0,3}d")  # as a table without accepting states: every prefix of a match
    table, accept = lstm_hip.dfa_intersect(a, acc_a, b, None)
    check_properties(table, accept)
    enumerate_against(table, accept, a, acc_a, b, None, b"abcd", 5)
    assert accepts(table, accept, b"abbc") and not accepts(table, accept, b"abbbbc")
    t2, a2 = lstm_hip.dfa_intersect(a, None, b, None)  # both: the common prefixes
    check_properties(t2, a2)
    assert a2.all()
    enumerate_against(t2, a2, a, None, b, None, b"abcd", 5)


def test_refusals():
    a, acc_a = lstm_hip.dfa_regex(b"a+")
    b, acc_b = lstm_hip.dfa_regex(b"b+")
    with pytest.raises(lstm_hip.LstmHipError) as e:
        lstm_hip.dfa_intersect(a, acc_a, b, acc_b)
    assert str(e.value) == "lstm_hip error -1: dfa_intersect: empty language: no string is accepted by both tables"
    bad = a.copy()
    bad[1, 7] = 2
    with pytest.raises(lstm_hip.LstmHipError) as e:
        lstm_hip.dfa_intersect(a, acc_a, bad, acc_a)
    assert str(e.value) == ("lstm_hip error -1: dfa_intersect: entry next[1][7] = 2 of table b is neither a state below 2 nor 0xFFFF")
    lib = lstm_hip.load_library()
    lib.lstm_hip_dfa_intersect.restype = C.c_int32
    p16 = lambda t: t.ctypes.data_as(C.POINTER(C.c_uint16))
    p8 = lambda t: t.ctypes.data_as(C.POINTER(C.c_uint8))
    assert lib.lstm_hip_dfa_intersect(None, 2, None, p16(a), 2, None, None, None, 0) == -1
    assert lib.lstm_hip_last_error() == b"dfa_intersect: null table"
    assert lib.lstm_hip_dfa_intersect(p16(a), 0, None, p16(a), 2, None, None, None, 0) == -1
    assert lib.lstm_hip_last_error() == b"dfa_intersect: states must be in [1, 4096] (got 0)"
    assert lib.lstm_hip_dfa_intersect(p16(a), 2, None, p16(a), 4097, None, None, None, 0) == -1
    assert lib.lstm_hip_last_error() == b"dfa_intersect: states must be in [1, 4096] (got 4097)"
    assert lib.lstm_hip_dfa_intersect(p16(a), 2, p8(acc_a), p16(a), 2, p8(acc_a), None, None, -1) == 2  # the size; cap ignored
    nxt, acc = np.zeros((2, 256), np.uint16), np.zeros(2, np.uint8)
    assert lib.lstm_hip_dfa_intersect(p16(a), 2, p8(acc_a), p16(a), 2, p8(acc_a), p16(nxt), p8(acc), 1) == -1
    assert lib.lstm_hip_last_error() == b"dfa_intersect: cap 1 is below the 2 states of the result"
    # more than 4096 states: two long counters with coprime periods
    x, ax = lstm_hip.dfa_regex(b"(?:a{67})*")
    y, ay = lstm_hip.dfa_regex(b"(?:a{71})*")
    with pytest.raises(lstm_hip.LstmHipError) as e:
        lstm_hip.dfa_intersect(x, ax, y, ay)
    assert str(e.value) == "lstm_hip error -1: dfa_intersect: too many states: the minimal automaton has 4757, above 4096"
    assert FORBID == 0xFFFF
