"""-m gpu: the argument refusals of lstm_hip_generate_processed (include/lstm_hip.h), return code and the whole text of
lstm_hip_last_error(), reached through ctypes on the loaded library as tests/test_accepting_refusals.py reaches
lstm_hip_generate_accepting's: one handle at hidden 32.  The refused calls launch nothing; the handle generates afterwards."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U8, I32, U64, F32, F64 = C.c_uint8, C.c_int32, C.c_uint64, C.c_float, C.c_double


@pytest.fixture(scope="module")
def L():
    import lstm_hip
    handle = lstm_hip.Lstm(32, 4, 1)
    handle.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(5), 32))
    yield handle
    handle.close()


def _p(a, t):
    return None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.POINTER(t))


def processed(L, streams=1, prompts=None, off=None, count=0, size=None, bias=None, min_p=0.0, no_repeat=0, history=None,
              history_off=None):
    import lstm_hip
    o = lstm_hip._Sampling(C.sizeof(lstm_hip._Sampling), 0.0, 0, 1.0, -1)
    b = None if bias is None else np.ascontiguousarray(bias, np.float32)
    hist = None if history is None else np.frombuffer(history, np.uint8)
    hoff = None if history_off is None else np.array(history_off, np.uint64)
    lp = lstm_hip._LogitProcessors(C.sizeof(lstm_hip._LogitProcessors) if size is None else size, _p(b, F32), min_p, no_repeat,
                                   _p(hist, U8), _p(hoff, U64))
    cells = max(count, 1) * max(streams, 1)
    return L.lib.lstm_hip_generate_processed(
        L._h, I32(streams), _p(None if prompts is None else np.frombuffer(prompts, np.uint8), U8),
        _p(None if off is None else np.array(off, np.uint64), U64), None, None, C.byref(o), None, I32(count),
        _p(np.zeros(cells, np.uint8), U8), None, None, None, None, None, None, None, None, C.byref(lp))


def _refused(L, rc, text):
    import lstm_hip
    assert rc == lstm_hip.EINVAL, (rc, L.lib.lstm_hip_last_error().decode())
    assert L.lib.lstm_hip_last_error().decode() == text


def test_the_refusals(L):
    import lstm_hip
    size = C.sizeof(lstm_hip._LogitProcessors)
    _refused(L, processed(L, size=size - 8), f"generate: logit processors of {size - 8} bytes, expected {size}")
    _refused(L, processed(L, size=0), f"generate: logit processors of 0 bytes, expected {size}")
    _refused(L, processed(L, size=size + 8), f"generate: logit processors of {size + 8} bytes, expected {size}")
    ban = "(to ban a byte, restrict a table with lstm_hip_dfa_restrict)"
    for at, value, text in ((0, np.nan, "nan"), (65, np.inf, "inf"), (255, -np.inf, "-inf")):
        bias = np.zeros(256, np.float32)
        bias[at] = value
        _refused(L, processed(L, bias=bias), f"generate: bias[{at}] = {text} is not finite {ban}")
    _refused(L, processed(L, min_p=float("nan")), "generate: min_p must be in [0, 1] (got nan)")
    _refused(L, processed(L, min_p=-0.5), "generate: min_p must be in [0, 1] (got -0.5)")
    _refused(L, processed(L, min_p=1.5), "generate: min_p must be in [0, 1] (got 1.5)")
    _refused(L, processed(L, min_p=float("inf")), "generate: min_p must be in [0, 1] (got inf)")
    _refused(L, processed(L, no_repeat=-1), "generate: no_repeat must be in [0, 64] (got -1)")
    _refused(L, processed(L, no_repeat=65), "generate: no_repeat must be in [0, 64] (got 65)")
    _refused(L, processed(L, no_repeat=2, history=b"abc"), "generate: history without history_off")
    _refused(L, processed(L, no_repeat=2, history_off=[0, 3]), "generate: history_off without history")
    _refused(L, processed(L, no_repeat=2, history=b"abc", history_off=[1, 3]), "generate: history_off[0] must be 0 (got 1)")
    _refused(L, processed(L, streams=2, no_repeat=2, history=b"abc", history_off=[0, 3, 2]),
             "generate: history_off decreases at stream 1 (2 < 3)")
    _refused(L, processed(L, history=b"abc", history_off=[0, 3]), "generate: history given with no_repeat 0: nothing reads it")
    # the scan's limit: the longest history + prompt, + count
    linear = "above 65536: the scan is linear in the text at every draw"
    _refused(L, processed(L, count=65537, no_repeat=1),
             f"generate: no_repeat over a text of 65537 bytes (the longest history + prompt, + count), {linear}")
    _refused(L, processed(L, streams=2, prompts=b"xy" * 10, off=[0, 5, 20], count=100, no_repeat=3, history=bytes(70000),
                          history_off=[0, 4000, 70000]),
             f"generate: no_repeat over a text of {66000 + 15 + 100} bytes (the longest history + prompt, + count), {linear}")
    # and what lstm_hip_generate_accepting refuses comes first, with its text
    _refused(L, processed(L, streams=0, no_repeat=1), "generate: streams must be in [1, 4096] (got 0)")
    _refused(L, processed(L, count=-1, min_p=0.5), "generate: count < 0 (-1)")


def test_the_handle_generates_afterwards(L):
    import lstm_hip
    _refused(L, processed(L, min_p=2.0), "generate: min_p must be in [0, 1] (got 2)")
    u = np.random.RandomState(1).random_sample((12, 3))
    out, _, _, _, info = L.generate([b"ab", b"", b"abc"], count=12, u=u, temperature=0.9, info=True, min_p=0.1, no_repeat_ngram=2,
                                    logit_bias={65: 1.5, 66: -1.5}, history=[b"xyz", b"", b"ab"])
    assert out.shape == (12, 3) and (info["out_len"] == 12).all() and (info["kept"] >= 1).all()
    with pytest.raises(lstm_hip.LstmHipError, match="generate: min_p must be in"):
        L.generate(count=2, temperature=0.0, min_p=3.0)
    at_the_limit = processed(L, count=2, no_repeat=64, min_p=1.0)  # both ends of the ranges are taken
    assert at_the_limit == 0, L.lib.lstm_hip_last_error().decode()
