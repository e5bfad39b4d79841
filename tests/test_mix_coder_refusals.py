"""-m gpu: the argument refusals of lstm_hip_encode_mixed and lstm_hip_decode_mixed (include/lstm_hip.h, DESIGN.md section
3.25), return code and the whole text of lstm_hip_last_error(), reached through ctypes on the loaded library as
tests/test_guided_refusals.py reaches the guided calls': a main handle at hidden 32 and a guide at hidden 16.  The refused calls
launch nothing (the launch counts of a profiling handle stay where they were); then the launch counts of one mixed call.  Not
reached: a guide on another device and a guide whose internal width is above 16384, as in tests/test_guided_refusals.py."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U8, I32, U64, F32, F64 = C.c_uint8, C.c_int32, C.c_uint64, C.c_float, C.c_double
TEXT = np.frombuffer(b"abc", np.uint8)
OFF = np.array([0, 3], np.uint64)


@pytest.fixture(scope="module")
def pair():
    import lstm_hip
    hs = []
    for n, seed in ((32, 5), (16, 6)):
        h = lstm_hip.Lstm(n, 4, 1)
        h.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(seed), n))
        hs.append(h)
    yield hs
    for h in hs:
        h.close()


def _p(a, t):
    return None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.POINTER(t))


def _block(models, weights, main_weight=1.0, size=None, nguides=None, null_guides=False, state=None):
    """state = (k, field): guide k gets a non-null pointer in that field"""
    import lstm_hip
    arr = (lstm_hip._Guide * max(len(models), 1))()
    buf = np.zeros(64, np.float32)
    for k, (m, w) in enumerate(zip(models, weights)):
        ptrs = {f: None for f in ("h0", "c0", "h_out", "c_out")}
        if state is not None and state[0] == k:
            ptrs[state[1]] = _p(buf, F32)
        arr[k] = lstm_hip._Guide(None if m is None else m._h.value, w, ptrs["h0"], ptrs["c0"], ptrs["h_out"], ptrs["c_out"])
    gd = lstm_hip._Guidance(C.sizeof(lstm_hip._Guidance) if size is None else size, main_weight,
                            len(models) if nguides is None else nguides, None if null_guides else arr)
    return gd, (arr, buf)


def _mix(rate=0.0, size=None):
    import lstm_hip
    return lstm_hip._MixCoding(C.sizeof(lstm_hip._MixCoding) if size is None else size, rate)


def encode(L, models=None, weights=None, mx=None, streams=1, code_cap=13, w_out=False, w_trace=False, **kw):
    gd = alive = None
    if models is not None:
        gd, alive = _block(models, weights, **kw)
    code, code_off = np.zeros(64, np.uint8), np.zeros(2, np.uint64)
    wo, wt = np.zeros(16, np.float32), np.zeros(64, np.float32)
    return L.lib.lstm_hip_encode_mixed(L._h, I32(streams), _p(TEXT, U8), _p(OFF, U64), _p(code, U8), U64(code_cap), _p(code_off, U64),
                                       None, None, C.byref(gd) if gd is not None else None, C.byref(mx) if mx is not None else None,
                                       _p(wo, F32) if w_out else None, _p(wt, F32) if w_trace else None)


def decode(L, models=None, weights=None, mx=None, streams=1, w_out=False, w_trace=False, **kw):
    assert not w_trace
    gd = alive = None
    if models is not None:
        gd, alive = _block(models, weights, **kw)
    code, text = np.zeros(8, np.uint8), np.zeros(3, np.uint8)
    wo = np.zeros(16, np.float32)
    return L.lib.lstm_hip_decode_mixed(L._h, I32(streams), _p(code, U8), _p(np.array([0, 8], np.uint64), U64), _p(OFF, U64), _p(text, U8),
                                       C.byref(gd) if gd is not None else None, C.byref(mx) if mx is not None else None,
                                       _p(wo, F32) if w_out else None)


def _refused(L, rc, text):
    import lstm_hip
    assert rc == lstm_hip.EINVAL, (rc, L.lib.lstm_hip_last_error().decode())
    assert L.lib.lstm_hip_last_error().decode() == text


def test_the_refusals(pair):
    import lstm_hip
    L, G = pair
    size, msize = C.sizeof(lstm_hip._Guidance), C.sizeof(lstm_hip._MixCoding)
    assert msize == 16 and lstm_hip._MixCoding.rate.offset == 8  # this ABI
    assert lstm_hip.mix_coder_version() == 1 and lstm_hip.coder_version() == 1
    L.set_profiling(True)
    L.reset_kernel_stats()
    for call, what in ((encode, "encode"), (decode, "decode")):
        # the guidance block's, in the words of the guided calls
        _refused(L, call(L, [G], [0.5], size=size - 8), f"{what}: guidance of {size - 8} bytes, expected {size}")
        _refused(L, call(L, [G], [0.5], nguides=0), f"{what}: nguides must be in [1, 4] (got 0)")
        _refused(L, call(L, [G] * 5, [0.1] * 5), f"{what}: nguides must be in [1, 4] (got 5)")
        _refused(L, call(L, [G], [0.5], null_guides=True), f"{what}: guidance with null guides")
        _refused(L, call(L, [G, None], [0.5, 0.5]), f"{what}: guide 1: null model")
        _refused(L, call(L, [G], [0.5], main_weight=float("nan")), f"{what}: main_weight must be finite (got nan)")
        _refused(L, call(L, [G, G], [0.5, float("inf")]), f"{what}: guide 1: weight must be finite (got inf)")
        # a guide's states: the coders start from zero and keep none
        for field in ("h0", "c0", "h_out", "c_out"):
            _refused(L, call(L, [G, G], [0.5, 0.5], state=(1, field)),
                     f"{what}: guide 1: h0, c0, h_out and c_out must be null (the coders start every model from zero)")
        # the mix coding block
        _refused(L, call(L, [G], [0.5], mx=_mix(size=msize - 8)), f"{what}: mix coding of {msize - 8} bytes, expected {msize}")
        _refused(L, call(L, [G], [0.5], mx=_mix(size=0)), f"{what}: mix coding of 0 bytes, expected {msize}")
        _refused(L, call(L, [G], [0.5], mx=_mix(size=msize + 8)), f"{what}: mix coding of {msize + 8} bytes, expected {msize}")
        for value, text in ((-0.5, "-0.5"), (float("nan"), "nan"), (float("inf"), "inf"), (float("-inf"), "-inf")):
            _refused(L, call(L, [G], [0.5], mx=_mix(rate=value)), f"{what}: rate must be finite and >= 0 (got {text})")
        _refused(L, call(L, mx=_mix(rate=0.0)), f"{what}: mix coding given without guidance")
        _refused(L, call(L, w_out=True), f"{what}: w_out / w_trace given without guidance")
        # the guidance's come before the mix coding's, and what the unmixed calls refuse comes first, with its text
        _refused(L, call(L, [G], [0.5], size=0, mx=_mix(size=0)), f"{what}: guidance of 0 bytes, expected {size}")
        _refused(L, call(L, [G], [0.5], size=0, streams=0), f"{what}: streams must be in [1, 4096] (got 0)")
    _refused(L, encode(L, w_trace=True), "encode: w_out / w_trace given without guidance")
    _refused(L, encode(L, [G], [0.5], size=0, code_cap=12), "encode: code_cap 12 is below the bound 13 (sum of lstm_hip_code_bound)")
    # nothing was launched by any of them
    assert all(v[0] == 0 for v in L.kernel_stats().values()), L.kernel_stats()
    L.set_profiling(False)


def test_the_launches_of_one_mixed_call(pair):
    L, G = pair
    texts = [b"abcde", b"", b"ab"]
    L.set_profiling(True)
    for guides in ([(G, 0.5)], [(G, 0.5), (L, 0.25), (G, -0.1)]):
        g = len(guides)
        L.reset_kernel_stats()
        codes, _ = L.encode_mixed(texts, guides=guides, main_weight=0.5, rate=0.01)
        st = {k: v[0] for k, v in L.kernel_stats().items() if v[0]}
        # five steps; behind the last one nothing is stepped
        assert st == {"pack_U": 1 + g, "fwd_step": 4 * (1 + g), "guide_logits": 5, "code_head_mixed": 5}, st
        L.reset_kernel_stats()
        assert L.decode_mixed(codes, [5, 0, 2], guides=guides, main_weight=0.5, rate=0.01) == texts
        st = {k: v[0] for k, v in L.kernel_stats().items() if v[0]}
        assert st == {"pack_U": 1 + g, "fwd_step": 4 * (1 + g), "guide_logits": 5, "code_head_mixed": 5}, st
    L.reset_kernel_stats()
    L.encode(texts)
    st = {k: v[0] for k, v in L.kernel_stats().items() if v[0]}
    assert st == {"pack_U": 1, "fwd_step": 4, "code_head": 5}, st  # the unmixed call: as before
    L.set_profiling(False)
