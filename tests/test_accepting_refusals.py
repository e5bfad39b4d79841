"""-m gpu: the argument refusals of lstm_hip_generate_accepting (include/lstm_hip.h), return code and the whole text of
lstm_hip_last_error(), reached through ctypes on the loaded library as tests/test_inference_refusals.py reaches the other
calls': one handle at hidden 32.  The texts of lstm_hip_generate_constrained that pass through the new function are checked
again through the old entry point.  Nothing here launches a kernel."""
import ctypes as C

import numpy as np
import pytest

import beam_constraint_ref as bcr

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


def _con(table, size=None, states=None, null=False):
    import lstm_hip
    t = np.ascontiguousarray(table, dtype=np.uint16)
    con = lstm_hip._Constraint(C.sizeof(lstm_hip._Constraint) if size is None else size, t.shape[0] if states is None else states,
                               None if null else _p(t, U16))
    con._keep = t
    return con


NO_BC = object()


def accepting(L, streams=1, prompts=None, off=None, count=0, con=None, accept=None, start=None, end=None, bc_size=None, bc=None,
              stop_byte=-1, temperature=0.0, u=None):
    import lstm_hip
    o = lstm_hip._Sampling(C.sizeof(lstm_hip._Sampling), temperature, 0, 1.0, stop_byte)
    acc = None if accept is None else np.ascontiguousarray(accept, np.uint8)
    if bc is not NO_BC:
        bc = lstm_hip._BeamConstraint(C.sizeof(lstm_hip._BeamConstraint) if bc_size is None else bc_size,
                                      C.pointer(con) if con is not None else None, _p(acc, U8))
    cells = max(count, 1) * max(streams, 1)
    return L.lib.lstm_hip_generate_accepting(
        L._h, I32(streams), _p(prompts, U8), _p(None if off is None else np.array(off, np.uint64), U64), None, None, C.byref(o),
        _p(u, F64), I32(count), _p(np.zeros(cells, np.uint8), U8), None, None, None, None, None,
        None if bc is NO_BC else C.byref(bc), _p(start, I32), _p(end, I32))


def _refused(L, rc, text):
    import lstm_hip
    assert rc == lstm_hip.EINVAL, (rc, L.lib.lstm_hip_last_error().decode())
    assert L.lib.lstm_hip_last_error().decode() == text


def test_the_new_refusals(L):
    import lstm_hip
    pat, acc = bcr.pattern_ab_newline()
    ends = np.zeros(2, np.int32)
    size = C.sizeof(lstm_hip._BeamConstraint)
    _refused(L, accepting(L, con=_con(pat), accept=acc, bc_size=size - 8), f"generate: beam constraint of {size - 8} bytes, expected {size}")
    _refused(L, accepting(L, con=_con(pat), accept=acc, bc_size=0), f"generate: beam constraint of 0 bytes, expected {size}")
    _refused(L, accepting(L, con=None, accept=acc), "generate: beam constraint with a null constraint")
    _refused(L, accepting(L, bc=NO_BC, start=np.zeros(1, np.int32)), "generate: start_state / end_state given without a constraint")
    _refused(L, accepting(L, bc=NO_BC, end=ends), "generate: start_state / end_state given without a constraint")
    # the deadline: no accepted string within count from where a stream stands
    _refused(L, accepting(L, count=1, con=_con(pat), accept=acc, stop_byte=10),
             "generate: stream 0: no accepted string of 1 bytes or fewer ending in the stop byte from state 0")
    _refused(L, accepting(L, streams=2, count=1, con=_con(pat), accept=acc, stop_byte=10, start=np.array([1, 0], np.int32)),
             "generate: stream 1: no accepted string of 1 bytes or fewer ending in the stop byte from state 0")
    _refused(L, accepting(L, count=1, con=_con(pat), accept=acc),  # (without a stop byte too: one letter is no match)
             "generate: stream 0: no accepted string of 1 bytes or fewer ending in the stop byte from state 0")
    # count 0: the state after the prompt must accept
    _refused(L, accepting(L, count=0, con=_con(pat), accept=acc, stop_byte=10),
             "generate: stream 0: no accepted string of 0 bytes or fewer ending in the stop byte from state 0")
    # (the state is the one after the prompt)
    _refused(L, accepting(L, streams=2, prompts=np.frombuffer(b"ab", np.uint8), off=[0, 0, 2], count=0, con=_con(pat), accept=acc,
                          stop_byte=10, start=np.array([4, 0], np.int32)),
             "generate: stream 1: no accepted string of 0 bytes or fewer ending in the stop byte from state 2")
    # (count + 1) x states above 2^28
    big = np.zeros((4096, 256), np.uint16)
    _refused(L, accepting(L, count=65536, con=_con(big), accept=np.ones(4096, np.uint8)),
             f"generate: (count + 1) x states = {65537 * 4096} above 2^28 with accepting states")
    # and every refusal of lstm_hip_generate_constrained comes first, with its text
    _refused(L, accepting(L, con=_con(pat, size=4), accept=acc), f"generate: constraint of 4 bytes, expected {C.sizeof(lstm_hip._Constraint)}")
    _refused(L, accepting(L, con=_con(pat, states=0), accept=acc), "generate: constraint states must be in [1, 4096] (got 0)")
    _refused(L, accepting(L, con=_con(pat, null=True), accept=acc), "generate: constraint with a null table")
    _refused(L, accepting(L, con=_con(pat), accept=acc, start=np.array([5], np.int32)), "generate: start_state[0] = 5 is outside [0, 5)")
    _refused(L, accepting(L, prompts=np.frombuffer(b"ac", np.uint8), off=[0, 2], con=_con(pat), accept=acc),
             "generate: stream 0: prompt byte 0x63 at offset 1 is forbidden in state 1")
    _refused(L, accepting(L, count=2, con=_con(pat), accept=acc, stop_byte=10, temperature=1.0), "generate: draws u are needed unless temperature is 0")
    _refused(L, accepting(L, streams=0, con=_con(pat), accept=acc), "generate: streams must be in [1, 4096] (got 0)")


def test_the_old_entry_points_keep_their_texts(L):
    import lstm_hip
    pat, _ = bcr.pattern_ab_newline()
    o = lstm_hip._Sampling(C.sizeof(lstm_hip._Sampling), 0.0, 0, 1.0, -1)
    out = np.zeros(4, np.uint8)

    def old(con=None, start=None, end=None, count=0):
        return L.lib.lstm_hip_generate_constrained(L._h, I32(1), None, None, None, None, C.byref(o), None, I32(count), _p(out, U8), None,
                                                   None, None, None, None, C.byref(con) if con is not None else None, _p(start, I32),
                                                   _p(end, I32))

    _refused(L, old(start=np.zeros(1, np.int32)), "generate: start_state / end_state given without a constraint")
    _refused(L, old(end=np.zeros(1, np.int32)), "generate: start_state / end_state given without a constraint")
    _refused(L, old(con=_con(pat, size=12)), f"generate: constraint of 12 bytes, expected {C.sizeof(lstm_hip._Constraint)}")
    _refused(L, old(con=_con(pat, states=4097)), "generate: constraint states must be in [1, 4096] (got 4097)")
    _refused(L, old(con=_con(pat, null=True)), "generate: constraint with a null table")
    bad = pat.copy()
    bad[2, 7] = 5
    _refused(L, old(con=_con(bad)), "generate: constraint entry next[2][7] = 5 is neither a state below 5 nor 0xFFFF")
    dead = pat.copy()
    dead[4, 10] = NONE
    _refused(L, old(con=_con(dead)), "generate: constraint state 4 can be reached and has no allowed byte")
    # the Python wrapper: accept needs a constraint
    with pytest.raises(lstm_hip.LstmHipError, match="generate: accept given without a constraint"):
        L.generate(count=1, temperature=0.0, accept=np.ones(1, np.uint8))
