"""-m gpu: the argument refusals of lstm_hip_generate_guided and lstm_hip_score_guided (include/lstm_hip.h), return code and
the whole text of lstm_hip_last_error(), reached through ctypes on the loaded library as tests/test_processor_refusals.py
reaches lstm_hip_generate_processed's: a main handle at hidden 32 and a guide at hidden 16.  The refused calls launch nothing
(the launch counts of a profiling handle stay where they were); the handles generate and score afterwards.  Not reached: a
guide on another device (the tests have one) and a guide whose internal width is above 16384 (no handle of that width is built
here, as tests/test_inference_refusals.py leaves the main handle's)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U8, I32, U64, F32, F64 = C.c_uint8, C.c_int32, C.c_uint64, C.c_float, C.c_double


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


def _block(models, weights, main_weight=1.0, size=None, nguides=None, null_guides=False):
    import lstm_hip
    arr = (lstm_hip._Guide * max(len(models), 1))()
    for k, (m, w) in enumerate(zip(models, weights)):
        arr[k] = lstm_hip._Guide(None if m is None else m._h.value, w, None, None, None, None)
    gd = lstm_hip._Guidance(C.sizeof(lstm_hip._Guidance) if size is None else size, main_weight,
                            len(models) if nguides is None else nguides, None if null_guides else arr)
    return gd, arr


def generate(L, models, weights, count=2, **kw):
    import lstm_hip
    gd, _alive = _block(models, weights, **kw)
    o = lstm_hip._Sampling(C.sizeof(lstm_hip._Sampling), 0.0, 0, 1.0, -1)
    return L.lib.lstm_hip_generate_guided(L._h, I32(1), None, None, None, None, C.byref(o), None, I32(count),
                                          _p(np.zeros(max(count, 1), np.uint8), U8), None, None, None, None, None, None, None, None,
                                          None, C.byref(gd))


def score(L, models, weights, **kw):
    import lstm_hip
    gd, _alive = _block(models, weights, **kw)
    o = lstm_hip._Scoring(C.sizeof(lstm_hip._Scoring), 1, 0, None)
    return L.lib.lstm_hip_score_guided(L._h, I32(1), _p(np.frombuffer(b"abc", np.uint8), U8), _p(np.array([0, 3], np.uint64), U64),
                                       None, None, C.byref(o), None, None, None, None, C.byref(gd))


def _refused(L, rc, text):
    import lstm_hip
    assert rc == lstm_hip.EINVAL, (rc, L.lib.lstm_hip_last_error().decode())
    assert L.lib.lstm_hip_last_error().decode() == text


def test_the_refusals(pair):
    import lstm_hip
    L, G = pair
    size = C.sizeof(lstm_hip._Guidance)
    L.set_profiling(True)
    L.reset_kernel_stats()
    for call, what in ((generate, "generate"), (score, "score")):
        _refused(L, call(L, [G], [0.5], size=size - 8), f"{what}: guidance of {size - 8} bytes, expected {size}")
        _refused(L, call(L, [G], [0.5], size=0), f"{what}: guidance of 0 bytes, expected {size}")
        _refused(L, call(L, [G], [0.5], size=size + 8), f"{what}: guidance of {size + 8} bytes, expected {size}")
        _refused(L, call(L, [G], [0.5], nguides=0), f"{what}: nguides must be in [1, 4] (got 0)")
        _refused(L, call(L, [G], [0.5], nguides=-1), f"{what}: nguides must be in [1, 4] (got -1)")
        _refused(L, call(L, [G] * 5, [0.1] * 5), f"{what}: nguides must be in [1, 4] (got 5)")
        _refused(L, call(L, [G], [0.5], null_guides=True), f"{what}: guidance with null guides")
        _refused(L, call(L, [None], [0.5]), f"{what}: guide 0: null model")
        _refused(L, call(L, [G, L, None], [0.5, 0.25, 0.25]), f"{what}: guide 2: null model")
        for value, text in ((np.nan, "nan"), (np.inf, "inf"), (-np.inf, "-inf")):
            _refused(L, call(L, [G], [0.5], main_weight=value), f"{what}: main_weight must be finite (got {text})")
            _refused(L, call(L, [G], [value]), f"{what}: guide 0: weight must be finite (got {text})")
            _refused(L, call(L, [G, G, L, G], [0.5, 0.0, -1.0, value]), f"{what}: guide 3: weight must be finite (got {text})")
    # and what the unguided calls refuse comes first, with its text
    _refused(L, generate(L, [G], [0.5], count=-1), "generate: count < 0 (-1)")
    # nothing was launched by any of them
    assert all(v[0] == 0 for v in L.kernel_stats().values()), L.kernel_stats()
    L.set_profiling(False)


def test_the_handles_work_afterwards(pair):
    import lstm_hip
    L, G = pair
    _refused(L, generate(L, [None], [1.0]), "generate: guide 0: null model")
    u = np.random.RandomState(1).random_sample((12, 3))
    out, _, _, _, info = L.generate([b"ab", b"", b"abc"], count=12, u=u, temperature=0.9, info=True, guides=[(G, -0.5), (L, 0.0)],
                                    main_weight=1.5)
    assert out.shape == (12, 3) and (info["out_len"] == 12).all() and (info["kept"] >= 1).all()
    assert len(info["guide_h"]) == 2 and info["guide_h"][0].shape == (3, 16) and info["guide_h"][1].shape == (3, 32)
    got = L.score_guided([b"hello", b""], first=True, guides=[(G, 0.5)], main_weight=0.5)
    assert got["surprisal"][0].shape == (5,) and np.isfinite(got["bits"]).all()
    with pytest.raises(lstm_hip.LstmHipError, match="generate: guide 0: weight must be finite"):
        L.generate(count=2, temperature=0.0, guides=[(G, float("nan"))])
    with pytest.raises(lstm_hip.LstmHipError, match="score: nguides must be in"):
        L.score_guided([b"ab"], guides=[])
    at_the_limit = generate(L, [G, L, G, L], [0.0, -1.0, 1000.0, 1.0])  # four guides; 0 and negative weights are taken
    assert at_the_limit == 0, L.lib.lstm_hip_last_error().decode()
    # the four rows a guided call adds to, and nothing else
    L.set_profiling(True)
    L.reset_kernel_stats()
    L.generate([b"ab"], count=3, temperature=0.0, guides=[(G, 0.5), (G, 0.25)])
    st = {k: v[0] for k, v in L.kernel_stats().items() if v[0]}
    L.set_profiling(False)
    assert st == {"pack_U": 3, "fwd_step": 3 * 5, "gen_head": 6, "guide_logits": 6}, st
