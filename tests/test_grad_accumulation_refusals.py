"""-m gpu: the refusals of gradient accumulation (include/lstm_hip.h), return code and the whole text of
lstm_hip_last_error(), reached through ctypes on the loaded library: one handle at hidden 32.  After every refusal the
handle answers lstm_hip_get_grad_accumulation with the setting it had.  Nothing here launches a kernel.

lstm_hip_comm_init's refusal while accumulation is on comes before the communicator library is loaded, so it is reached
here; turning accumulation on with a communicator on the handle needs a communicator and is left to the text check of
tests/test_grad_accumulation_cpu.py."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
I32, U64, F32, F64 = C.c_int32, C.c_uint64, C.c_float, C.c_double
OFF = "gradient accumulation is off on this handle (lstm_hip_set_grad_accumulation)"


@pytest.fixture()
def L():
    import lstm_hip
    handle = lstm_hip.Lstm(32, 4, 2)
    yield handle
    handle.close()


def _err(L):
    return L.lib.lstm_hip_last_error().decode()


def _refused(L, rc, code, text, setting):
    assert rc == code, (rc, _err(L))
    assert _err(L) == text
    assert L.grad_accumulation() == setting  # the handle is usable and as it was


def _block(L):
    return np.zeros(L.np, np.float32)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(F32))


@pytest.mark.parametrize("every", [0, -1, -2147483648])
def test_bad_every(L, every):
    import lstm_hip
    for setting in ((1, False, 0), (3, True, 0)):
        L.set_grad_accumulation(setting[0], setting[1])
        _refused(L, L.lib.lstm_hip_set_grad_accumulation(L._h, I32(every), I32(0)), lstm_hip.EINVAL,
                 f"set_grad_accumulation: every must be >= 1 (1 = off; got {every})", setting)


@pytest.mark.parametrize("mean", [2, -1, 256])
def test_bad_mean(L, mean):
    import lstm_hip
    for every in (1, 4):  # (checked when turning off too)
        _refused(L, L.lib.lstm_hip_set_grad_accumulation(L._h, I32(every), I32(mean)), lstm_hip.EINVAL,
                 f"set_grad_accumulation: mean must be 0 or 1 (got {mean})", (1, False, 0))


@pytest.mark.parametrize("pending", [-1, 3, 4, 2147483647])
def test_pending_outside_the_cycle(L, pending):
    import lstm_hip
    L.set_grad_accumulation(3)
    blk = _block(L)
    _refused(L, L.lib.lstm_hip_set_grad_accumulator(L._h, _fp(blk), I32(pending)), lstm_hip.EINVAL,
             f"set_grad_accumulator: pending must be in [0, 2] (got {pending})", (3, False, 0))


def test_null_pointers(L):
    import lstm_hip
    lib = L.lib
    L.set_grad_accumulation(2, True)
    setting = (2, True, 0)
    e, m, p = I32(), I32(), I32()
    for args in ((None, C.byref(m), C.byref(p)), (C.byref(e), None, C.byref(p)), (C.byref(e), C.byref(m), None)):
        _refused(L, lib.lstm_hip_get_grad_accumulation(L._h, *args), lstm_hip.EINVAL, "get_grad_accumulation: null argument", setting)
    _refused(L, lib.lstm_hip_get_grad_accumulation(None, C.byref(e), C.byref(m), C.byref(p)), lstm_hip.EINVAL,
             "get_grad_accumulation: null argument", setting)
    _refused(L, lib.lstm_hip_get_grad_accumulator(L._h, None), lstm_hip.EINVAL, "get_grad_accumulator: null pointer", setting)
    _refused(L, lib.lstm_hip_set_grad_accumulator(L._h, None, I32(0)), lstm_hip.EINVAL, "set_grad_accumulator: null pointer", setting)
    blk = _block(L)
    _refused(L, lib.lstm_hip_set_grad_accumulation(None, I32(2), I32(0)), lstm_hip.EINVAL, "null handle", setting)
    _refused(L, lib.lstm_hip_get_grad_accumulator(None, _fp(blk)), lstm_hip.EINVAL, "null handle", setting)
    _refused(L, lib.lstm_hip_set_grad_accumulator(None, _fp(blk), I32(0)), lstm_hip.EINVAL, "null handle", setting)


def test_the_accumulator_needs_accumulation_on(L):
    import lstm_hip
    blk = _block(L)
    for _ in range(2):  # on a fresh handle, and after it was on and is off again
        _refused(L, L.lib.lstm_hip_get_grad_accumulator(L._h, _fp(blk)), lstm_hip.ESTATE, "get_grad_accumulator: " + OFF, (1, False, 0))
        _refused(L, L.lib.lstm_hip_set_grad_accumulator(L._h, _fp(blk), I32(0)), lstm_hip.ESTATE, "set_grad_accumulator: " + OFF,
                 (1, False, 0))
        L.set_grad_accumulation(2)
        L.set_grad_accumulation(1)


def test_the_adaptive_coders_while_on(L):
    import lstm_hip
    L.set_grad_accumulation(2)
    off = np.zeros(L.B + 1, np.uint64)
    offp = off.ctypes.data_as(C.POINTER(U64))
    tail = "gradient accumulation is on (lstm_hip_set_grad_accumulation); the adaptive coders update after every block"
    rc = L.lib.lstm_hip_encode_adaptive(L._h, None, offp, F64(0.01), None, U64(0), offp, None, None, None)
    _refused(L, rc, lstm_hip.ESTATE, "encode_adaptive: " + tail, (2, False, 0))
    rc = L.lib.lstm_hip_decode_adaptive(L._h, None, offp, offp, F64(0.01), None)
    _refused(L, rc, lstm_hip.ESTATE, "decode_adaptive: " + tail, (2, False, 0))


def test_comm_init_while_on(L):
    import lstm_hip
    L.set_grad_accumulation(2)
    uid = (C.c_uint8 * lstm_hip.UNIQUE_ID_BYTES)()
    _refused(L, L.lib.lstm_hip_comm_init(L._h, uid, I32(1), I32(0)), lstm_hip.ESTATE,
             "comm_init: gradient accumulation is on (lstm_hip_set_grad_accumulation); it runs on one device", (2, False, 0))
