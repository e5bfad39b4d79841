"""-m gpu: the argument refusals of the inference calls, return code and the whole text of lstm_hip_last_error().

lstm_hip_generate_constrained, lstm_hip_beam_search_constrained, lstm_hip_score, lstm_hip_encode and lstm_hip_decode refuse a
bad argument before anything is launched.  Every such refusal is reached here through ctypes on the loaded library (the Python
wrapper builds valid offsets and structs itself), on one handle at hidden 32, window 4, one stream.  The expected texts are
written out from the source of the calls as it stood before their preambles were shared, so that a shared validator cannot
change one silently.  Not reached: the hidden-width refusals (hidden above 16384, hidden x beams above 16384), which no handle of
this size can meet.  Nothing here launches a kernel."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = 0xFFFF
U8, U16, I32, U64, F64 = C.c_uint8, C.c_uint16, C.c_int32, C.c_uint64, C.c_double


@pytest.fixture(scope="module")
def L():
    import lstm_hip
    handle = lstm_hip.Lstm(32, 4, 1)
    yield handle
    handle.close()


def _p(a, t):
    return None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.POINTER(t))


def _off(values):
    return None if values is None else np.array(values, np.uint64)


def _table(states=1, allowed=((0, 0x61, 0),)):
    """a (states, 256) table, everything forbidden but the (state, byte, next) triples"""
    t = np.full((states, 256), NONE, np.uint16)
    for q, b, to in allowed:
        t[q, b] = to
    return t


def _con(table, size=None, states=None, null=False):
    import lstm_hip
    t = np.ascontiguousarray(table, dtype=np.uint16)
    con = lstm_hip._Constraint(C.sizeof(lstm_hip._Constraint) if size is None else size, t.shape[0] if states is None else states,
                               None if null else _p(t, U16))
    con._keep = t
    return con


def _refused(L, rc, text):
    import lstm_hip
    assert rc == lstm_hip.EINVAL, (rc, L.lib.lstm_hip_last_error().decode())
    assert L.lib.lstm_hip_last_error().decode() == text


SOME = object()  # "a valid buffer of this call's size"


def generate(L, streams=1, prompts=None, off=None, opt=SOME, u=None, count=0, out=SOME, con=None, start=None, end=None,
             size=None, temperature=0.0, top_k=0, top_p=1.0, stop_byte=-1):
    import lstm_hip
    o = lstm_hip._Sampling(C.sizeof(lstm_hip._Sampling) if size is None else size, temperature, top_k, top_p, stop_byte)
    cells = max(count, 1) * max(streams, 1)
    return L.lib.lstm_hip_generate_constrained(
        L._h, I32(streams), _p(prompts, U8), _p(_off(off), U64), None, None, C.byref(o) if opt is SOME else None, _p(u, F64),
        I32(count), _p(np.zeros(cells, np.uint8), U8) if out is SOME else None, None, None, None, None, None,
        C.byref(con) if con is not None else None, _p(start, I32), _p(end, I32))


def beam(L, streams=1, prompts=None, off=None, opt=SOME, count=0, out=SOME, out_len=SOME, bits=SOME, bc=None, con=None,
         accept=None, start=None, end=None, size=None, beams=2, stop_byte=-1, bc_size=None):
    import lstm_hip
    o = lstm_hip._Beam(C.sizeof(lstm_hip._Beam) if size is None else size, beams, stop_byte)
    if con is not None or bc_size is not None:
        bc = lstm_hip._BeamConstraint(C.sizeof(lstm_hip._BeamConstraint) if bc_size is None else bc_size,
                                      C.pointer(con) if con is not None else None, _p(accept, U8))
    cols = max(streams, 1) * max(beams, 1)
    return L.lib.lstm_hip_beam_search_constrained(
        L._h, I32(streams), _p(prompts, U8), _p(_off(off), U64), None, None, C.byref(o) if opt is SOME else None, I32(count),
        _p(np.zeros(8, np.uint8), U8) if out is SOME else None,  # (no case gets as far as writing `out`)
        _p(np.zeros(cols, np.int32), I32) if out_len is SOME else None, _p(np.zeros(cols, np.float64), F64) if bits is SOME else None,
        None, None, C.byref(bc) if bc is not None else None, _p(start, I32), _p(end, I32))


def score(L, streams=1, text=None, off=(0, 0), opt=SOME, out=SOME, con=None, start=None, size=None, out_size=None, first=0,
          top_n=0, top_byte=None, top_bits=None, end=None):
    import lstm_hip
    o = lstm_hip._Scoring(C.sizeof(lstm_hip._Scoring) if size is None else size, first, top_n,
                          C.pointer(con) if con is not None else None)
    res = lstm_hip._Scores(C.sizeof(lstm_hip._Scores) if out_size is None else out_size, None, None, None, _p(top_byte, U8),
                           _p(top_bits, C.c_float), None, _p(end, I32))
    return L.lib.lstm_hip_score(L._h, I32(streams), _p(text, U8), _p(_off(off), U64), None, None,
                                C.byref(o) if opt is SOME else None, _p(start, I32), C.byref(res) if out is SOME else None, None, None)


def encode(L, streams=1, text=None, off=(0, 0), code=SOME, cap=64, code_off=SOME):
    return L.lib.lstm_hip_encode(L._h, I32(streams), _p(text, U8), _p(_off(off), U64),
                                 _p(np.zeros(64, np.uint8), U8) if code is SOME else None, U64(cap),
                                 _p(np.zeros(max(streams, 1) + 1, np.uint64), U64) if code_off is SOME else None, None, None)


def decode(L, streams=1, code=None, code_off=(0, 0), text_off=(0, 0), text=None):
    return L.lib.lstm_hip_decode(L._h, I32(streams), _p(code, U8), _p(_off(code_off), U64), _p(_off(text_off), U64), _p(text, U8))


ABC = np.frombuffer(b"abc", np.uint8)
I1 = np.zeros(1, np.int32)


def _constraint_cases(what):
    """(keyword arguments, text) for every refusal of the table checks, under the call's name"""
    ok = _table()
    high = _table()
    high[0, 0x62] = 1  # an entry that is neither a state nor 0xFFFF
    dead = _table(2, ((0, 0x61, 1),))  # state 1 can be reached and allows nothing
    return [
        (dict(con=_con(ok, size=8)), f"{what}: constraint of 8 bytes, expected 16"),
        (dict(con=_con(ok, states=0)), f"{what}: constraint states must be in [1, 4096] (got 0)"),
        (dict(con=_con(ok, states=4097)), f"{what}: constraint states must be in [1, 4096] (got 4097)"),
        (dict(con=_con(ok, null=True)), f"{what}: constraint with a null table"),
        (dict(con=_con(high)), f"{what}: constraint entry next[0][98] = 1 is neither a state below 1 nor 0xFFFF"),
        (dict(con=_con(ok), start=np.array([-1], np.int32)), f"{what}: start_state[0] = -1 is outside [0, 1)"),
        (dict(con=_con(ok), start=np.array([1], np.int32)), f"{what}: start_state[0] = 1 is outside [0, 1)"),
        (dict(con=_con(dead)), f"{what}: constraint state 1 can be reached and has no allowed byte"),
    ]


def _generate_cases():
    u1 = np.zeros(1, np.float64)
    return [
        (dict(opt=None), "generate: null sampling options"),
        (dict(size=8), "generate: sampling options of 8 bytes, expected 40"),
        (dict(top_k=-1), "generate: top_k must be in [0, 256] (got -1)"),
        (dict(top_k=257), "generate: top_k must be in [0, 256] (got 257)"),
        (dict(top_p=0.0), "generate: top_p must be in (0, 1] (got 0)"),
        (dict(top_p=1.5), "generate: top_p must be in (0, 1] (got 1.5)"),
        (dict(stop_byte=-2), "generate: stop_byte must be -1 or in [0, 255] (got -2)"),
        (dict(stop_byte=256), "generate: stop_byte must be -1 or in [0, 255] (got 256)"),
        (dict(streams=0), "generate: streams must be in [1, 4096] (got 0)"),
        (dict(streams=4097), "generate: streams must be in [1, 4096] (got 4097)"),
        (dict(count=-1), "generate: count < 0 (-1)"),
        (dict(temperature=-1.0), "generate: temperature must be finite and >= 0 (got -1)"),
        (dict(temperature=float("inf")), "generate: temperature must be finite and >= 0 (got inf)"),
        (dict(count=1, temperature=1.0), "generate: draws u are needed unless temperature is 0"),
        (dict(count=1, out=None), "generate: null out with count > 0"),
        (dict(count=1, temperature=1.0, u=u1, out=None), "generate: null out with count > 0"),
        (dict(prompts=ABC), "generate: prompts without prompt_off"),
        (dict(prompts=ABC, off=(3, 3)), "generate: prompt_off[0] must be 0 (got 3)"),
        (dict(streams=2, prompts=ABC, off=(0, 3, 2)), "generate: prompt_off decreases at stream 1 (2 < 3)"),
        (dict(streams=3, prompts=ABC, off=(0, 1, 3, 0)), "generate: prompt_off decreases at stream 2 (0 < 3)"),
        (dict(off=(0, 3)), "generate: prompt_off without prompts"),
        (dict(start=I1), "generate: start_state / end_state given without a constraint"),
        (dict(end=I1), "generate: start_state / end_state given without a constraint"),
        *_constraint_cases("generate"),
        (dict(con=_con(_table()), prompts=np.frombuffer(b"aab", np.uint8), off=(0, 3)),
         "generate: stream 0: prompt byte 0x62 at offset 2 is forbidden in state 0"),
        (dict(streams=2, con=_con(_table(2, ((0, 0x61, 1), (1, 0x62, 1)))), prompts=np.frombuffer(b"aabba", np.uint8), off=(0, 1, 5)),
         "generate: stream 1: prompt byte 0x61 at offset 3 is forbidden in state 1"),
    ]


def _beam_cases():
    acc0 = np.zeros(1, np.uint8)
    return [
        (dict(opt=None), "beam_search: null options"),
        (dict(size=8), "beam_search: options of 8 bytes, expected 12"),
        (dict(beams=0), "beam_search: beams must be in [1, 32] (got 0)"),
        (dict(beams=33), "beam_search: beams must be in [1, 32] (got 33)"),
        (dict(stop_byte=-2), "beam_search: stop_byte must be -1 or in [0, 255] (got -2)"),
        (dict(stop_byte=256), "beam_search: stop_byte must be -1 or in [0, 255] (got 256)"),
        (dict(streams=0), "beam_search: streams must be >= 1 and streams * beams <= 4096 (got 0 x 2)"),
        (dict(streams=129, beams=32), "beam_search: streams must be >= 1 and streams * beams <= 4096 (got 129 x 32)"),
        (dict(count=-1), "beam_search: count < 0 (-1)"),
        (dict(count=1, out=None), "beam_search: null out, out_len or bits with count > 0"),
        (dict(count=1, out_len=None), "beam_search: null out, out_len or bits with count > 0"),
        (dict(count=1, bits=None), "beam_search: null out, out_len or bits with count > 0"),
        (dict(prompts=ABC), "beam_search: prompts without prompt_off"),
        (dict(prompts=ABC, off=(3, 3)), "beam_search: prompt_off[0] must be 0 (got 3)"),
        (dict(streams=2, prompts=ABC, off=(0, 3, 2)), "beam_search: prompt_off decreases at stream 1 (2 < 3)"),
        (dict(streams=3, prompts=ABC, off=(0, 1, 3, 0)), "beam_search: prompt_off decreases at stream 2 (0 < 3)"),
        (dict(off=(0, 3)), "beam_search: prompt_off without prompts"),
        (dict(start=I1), "beam_search: start_state / end_state given without a constraint"),
        (dict(end=np.zeros(2, np.int32)), "beam_search: start_state / end_state given without a constraint"),
        (dict(con=_con(_table()), bc_size=8), "beam_search: beam constraint of 8 bytes, expected 24"),
        (dict(bc_size=24), "beam_search: beam constraint with a null constraint"),
        *_constraint_cases("beam_search"),
        (dict(con=_con(_table()), prompts=np.frombuffer(b"aab", np.uint8), off=(0, 3)),
         "beam_search: stream 0: prompt byte 0x62 at offset 2 is forbidden in state 0"),
        (dict(streams=2, con=_con(_table(2, ((0, 0x61, 1), (1, 0x62, 1)))), prompts=np.frombuffer(b"aabba", np.uint8), off=(0, 1, 5)),
         "beam_search: stream 1: prompt byte 0x61 at offset 3 is forbidden in state 1"),
        (dict(con=_con(_table()), accept=acc0, count=1 << 28),
         "beam_search: (count + 1) x states = 268435457 above 2^28 with accepting states"),
        # the deadline: no state accepts, so no string of `count` bytes or fewer can end accepted
        (dict(con=_con(_table()), accept=acc0, count=2),
         "beam_search: stream 0: no accepted string of 2 bytes or fewer ending in the stop byte from state 0"),
        (dict(streams=2, con=_con(_table(2, ((0, 0x61, 0), (1, 0x61, 1)))), accept=np.array([1, 0], np.uint8), count=3,
              start=np.array([0, 1], np.int32)),
         "beam_search: stream 1: no accepted string of 3 bytes or fewer ending in the stop byte from state 1"),
    ]


def _score_cases():
    b1, f1 = np.zeros(1, np.uint8), np.zeros(1, np.float32)
    return [
        (dict(opt=None), "score: null options"),
        (dict(size=8), "score: options of 8 bytes, expected 24"),
        (dict(out_size=8), "score: outputs of 8 bytes, expected 64"),
        (dict(first=2), "score: first must be 0 or 1 (got 2)"),
        (dict(top_n=-1), "score: top_n must be in [0, 8] (got -1)"),
        (dict(top_n=9), "score: top_n must be in [0, 8] (got 9)"),
        (dict(top_byte=b1), "score: top_byte / top_bits given with top_n = 0"),
        (dict(top_bits=f1), "score: top_byte / top_bits given with top_n = 0"),
        (dict(start=I1), "score: start_state / end_state given without a constraint"),
        (dict(end=I1), "score: start_state / end_state given without a constraint"),
        (dict(streams=0), "score: streams must be in [1, 4096] (got 0)"),
        (dict(streams=4097), "score: streams must be in [1, 4096] (got 4097)"),
        (dict(off=None), "score: null text_off"),
        (dict(text=ABC, off=(3, 3)), "score: text_off[0] must be 0 (got 3)"),
        (dict(streams=2, text=ABC, off=(0, 3, 2)), "score: text_off decreases at stream 1 (2 < 3)"),
        (dict(streams=3, text=ABC, off=(0, 1, 3, 0)), "score: text_off decreases at stream 2 (0 < 3)"),
        (dict(off=(0, 3)), "score: null text with 3 bytes to score"),
        *_constraint_cases("score"),
        (dict(con=_con(_table()), text=np.frombuffer(b"aab", np.uint8), off=(0, 3)),
         "score: stream 0: byte 0x62 at offset 2 is forbidden in state 0"),
        (dict(streams=2, con=_con(_table(2, ((0, 0x61, 1), (1, 0x62, 1)))), text=np.frombuffer(b"aabba", np.uint8), off=(0, 1, 5)),
         "score: stream 1: byte 0x61 at offset 3 is forbidden in state 1"),
    ]


def _encode_cases():
    return [
        (dict(streams=0), "encode: streams must be in [1, 4096] (got 0)"),
        (dict(streams=4097), "encode: streams must be in [1, 4096] (got 4097)"),
        (dict(off=None), "encode: null text_off"),
        (dict(text=ABC, off=(3, 3)), "encode: text_off[0] must be 0 (got 3)"),
        (dict(streams=2, text=ABC, off=(0, 3, 2)), "encode: text_off decreases at stream 1 (2 < 3)"),
        (dict(streams=3, text=ABC, off=(0, 1, 3, 0)), "encode: text_off decreases at stream 2 (0 < 3)"),
        (dict(text=ABC, off=(0, 3), code_off=None), "encode: null code_off"),
        (dict(off=(0, 3)), "encode: null text with 3 bytes to code"),
        (dict(text=ABC, off=(0, 1 << 63)), "encode: text too long"),
        (dict(text=ABC, off=(0, 3), cap=12), "encode: code_cap 12 is below the bound 13 (sum of lstm_hip_code_bound)"),
        (dict(streams=2, text=ABC, off=(0, 1, 3), cap=16), "encode: code_cap 16 is below the bound 17 (sum of lstm_hip_code_bound)"),
        (dict(text=ABC, off=(0, 3), cap=13, code=None), "encode: null code"),
    ]


def _decode_cases():
    return [
        (dict(streams=0), "decode: streams must be in [1, 4096] (got 0)"),
        (dict(streams=4097), "decode: streams must be in [1, 4096] (got 4097)"),
        (dict(code_off=None), "decode: null code_off"),
        (dict(code=ABC, code_off=(3, 3)), "decode: code_off[0] must be 0 (got 3)"),
        (dict(streams=2, code=ABC, code_off=(0, 3, 2), text_off=(0, 0, 0)), "decode: code_off decreases at stream 1 (2 < 3)"),
        (dict(text_off=None), "decode: null text_off"),
        (dict(text=ABC, text_off=(3, 3)), "decode: text_off[0] must be 0 (got 3)"),
        (dict(streams=2, text=ABC, code_off=(0, 0, 0), text_off=(0, 3, 2)), "decode: text_off decreases at stream 1 (2 < 3)"),
        (dict(streams=3, text=ABC, code_off=(0, 0, 0, 0), text_off=(0, 1, 3, 0)), "decode: text_off decreases at stream 2 (0 < 3)"),
        (dict(code_off=(0, 3)), "decode: null code with 3 code bytes"),
        (dict(code=ABC, code_off=(0, 3), text_off=(0, 3)), "decode: null text with 3 bytes to decode"),
    ]


CALLS = [(generate, _generate_cases), (beam, _beam_cases), (score, _score_cases), (encode, _encode_cases), (decode, _decode_cases)]


@pytest.mark.parametrize("call,cases", CALLS, ids=[c.__name__ for c, _ in CALLS])
def test_refusals(L, call, cases):
    for kwargs, text in cases():
        _refused(L, call(L, **kwargs), text)


def test_struct_sizes():
    """the sizes the texts above spell out"""
    import lstm_hip
    assert [C.sizeof(t) for t in (lstm_hip._Sampling, lstm_hip._Constraint, lstm_hip._Beam, lstm_hip._BeamConstraint,
                                  lstm_hip._Scoring, lstm_hip._Scores)] == [40, 16, 12, 24, 24, 64]
