"""CPU: the reference of the mixed coder (tests/mix_coder_ref.py) against itself -- the control of
tests/test_mix_code_head_emulation_cpu.py and tests/test_mix_coder.py, which hold the kernels to it.  Identities (a mix that
selects one member is that member's own table; rate 0 leaves the weights alone), the float32 gradient against its float64
statement within the derived bound, a learning case in which the learned weights must beat the fixed ones by a stated margin,
and mutants of the rule that the comparisons used elsewhere must catch."""
import numpy as np
import pytest

import code_table_ref as ct
import mix_coder_ref as mr
import range_coder_ref as rc

f32 = np.float32
M = 256


def _logits(rs, scale=3.0):
    return (rs.standard_normal(M) * scale).astype(f32)


def test_a_mix_that_selects_one_member_is_that_members_table():
    rs = np.random.RandomState(1)
    for _ in range(8):
        zs = [_logits(rs), _logits(rs)]
        for v, k in (((1.0, 0.0), 0), ((0.0, 1.0), 1)):
            q, cum, T = ct.table32(mr.mix32(zs, v))
            q1, cum1, T1 = ct.table32(zs[k])
            assert q.tobytes() == q1.tobytes() and cum.tobytes() == cum1.tobytes() and T == T1
            assert mr.update32(v, q, T, zs, 17, 0.0).tobytes() == np.array(v, f32).tobytes()  # rate 0: the identity


def test_rate_zero_keeps_the_calls_weights_at_every_byte():
    rs = np.random.RandomState(2)
    text = rs.randint(0, 256, size=20)
    zs = [[_logits(rs), _logits(rs), _logits(rs)] for _ in text]
    v0 = (0.3, 0.9, -0.7)
    _, trace, w_trace, w_out, _ = mr.encode(text, lambda j: zs[j], v0, 0.0)
    assert (w_trace == np.array(v0, f32)).all() and w_out.tobytes() == np.array(v0, f32).tobytes()
    assert w_trace[0].tobytes() == np.array(v0, f32).tobytes()
    for j, x in enumerate(text):
        q, cum, T = ct.table32(mr.mix32(zs[j], v0))
        assert tuple(trace[j]) == (cum[x], q[x], T)


def test_the_float32_gradient_is_within_the_derived_bound_of_its_float64_statement():
    rs = np.random.RandomState(3)
    worst = 0.0
    for i in range(40):
        zs = [_logits(rs, 1.0 + i % 5), _logits(rs, 4.0), (rs.randint(-64, 65, size=M) / 16).astype(f32)]
        v = (rs.standard_normal(3) * 0.7).astype(f32)
        q, _, T = ct.table32(mr.mix32(zs, v))
        x = int(rs.randint(0, 256)) if i % 2 else int(np.argmax(q))
        g32, g64, bound = mr.grad32(q, T, zs, x), mr.grad64(q, T, zs, x), mr.grad_bound(q, T, zs, x)
        err = np.abs(g32.astype(np.float64) - g64)
        assert (err <= bound).all(), (i, err, bound)
        worst = max(worst, float((err / bound).max()))
        assert (bound < 1e-3 * (1 + np.abs(g64))).all(), (i, bound, g64)  # the bound says something
    assert worst > 1e-3, worst  # ... and is not idle: float32 does round here


def _learning_case(seed=5, n=240, peak=3.0):
    """the main model's logits are noise, the guide's are flat but for `peak` on the true byte"""
    rs = np.random.RandomState(seed)
    text = rs.randint(0, 256, size=n)
    z0 = (rs.standard_normal((n, M)) * 2.0).astype(f32)
    z1 = np.zeros((n, M), f32)
    z1[np.arange(n), text] = peak
    return text, lambda j: [z0[j], z1[j]]


LEARN_RATE = 0.02
LEARN_MARGIN = 0.25  # the learned run needs at most (1 - margin) of the fixed run's bits


def test_learned_weights_beat_the_fixed_mix_when_the_guide_is_the_better_model():
    text, zs_of = _learning_case()
    assert len(text) >= 200
    _, _, _, _, fixed = mr.encode(text, zs_of, (0.5, 0.5), 0.0)
    code, _, w_trace, w_out, learned = mr.encode(text, zs_of, (0.5, 0.5), LEARN_RATE)
    assert w_out[1] > 1.0 > 0.5 and w_trace[-1][1] > w_trace[len(text) // 4][1] > w_trace[0][1] == f32(0.5)  # the guide's weight rises
    assert abs(w_out[0]) < 0.25  # ... and the noise is turned down
    assert learned <= (1.0 - LEARN_MARGIN) * fixed, (learned, fixed)
    back, w_dec = mr.decode(code, len(text), zs_of, (0.5, 0.5), LEARN_RATE)
    assert back == bytes(int(b) for b in text) and w_dec.tobytes() == w_out.tobytes()


def test_round_trips_of_the_reference_with_two_guides_and_odd_weights():
    rs = np.random.RandomState(7)
    for n in (0, 1, 2, 33):
        text = rs.randint(0, 256, size=n)
        zs = [[_logits(rs), _logits(rs, 1.0), _logits(rs, 2.0)] for _ in range(n)]
        for rate in (0.0, 0.01):
            code, _, _, w_out, _ = mr.encode(text, lambda j: zs[j], (0.7, 0.3, -0.2), rate)
            back, w_dec = mr.decode(code, n, lambda j: zs[j], (0.7, 0.3, -0.2), rate)
            assert back == bytes(int(b) for b in text) and w_dec.tobytes() == w_out.tobytes(), (n, rate)
            assert (len(code) == 0) == (n == 0)


# ---- mutants: each changes what a comparison elsewhere relies on, and each must show
def test_mutant_sign_flipped_is_caught():
    text, zs_of = _learning_case()
    _, _, _, w_out, learned = mr.encode(text, zs_of, (0.5, 0.5), LEARN_RATE)
    _, _, _, w_mut, mutant = mr.encode(text, zs_of, (0.5, 0.5), LEARN_RATE, sign=-1)
    _, _, _, _, fixed = mr.encode(text, zs_of, (0.5, 0.5), 0.0)
    assert w_mut[1] < 0.5 < w_out[1] and mutant > fixed > learned  # it unlearns: the learning test fails on it
    assert w_mut.tobytes() != w_out.tobytes()


def test_mutant_update_before_the_byte_is_coded_breaks_the_round_trip():
    text, zs_of = _learning_case(n=60)
    code, trace, _, _, _ = mr.encode(text, zs_of, (0.5, 0.5), LEARN_RATE, early=True)
    good, trace_good, _, _, _ = mr.encode(text, zs_of, (0.5, 0.5), LEARN_RATE)
    assert not np.array_equal(trace, trace_good)
    try:
        back, _ = mr.decode(code, len(text), zs_of, (0.5, 0.5), LEARN_RATE)
    except rc.CoderError:
        back = None
    assert back != bytes(int(b) for b in text)  # the decoder cannot know the byte before it has decoded it
    assert mr.decode(good, len(text), zs_of, (0.5, 0.5), LEARN_RATE)[0] == bytes(int(b) for b in text)


def test_mutant_gradient_summed_in_reverse_is_caught():
    rs = np.random.RandomState(11)
    differs = 0
    for _ in range(10):
        zs = [_logits(rs), _logits(rs)]
        q, _, T = ct.table32(mr.mix32(zs, (0.6, 0.4)))
        x = int(rs.randint(0, 256))
        a = mr.update32((0.6, 0.4), q, T, zs, x, 0.05)
        b = mr.update32((0.6, 0.4), q, T, zs, x, 0.05, reverse=True)
        differs += a.tobytes() != b.tobytes()
    assert differs >= 5, differs  # a bit-for-bit comparison of the weights sees the order


def test_mutant_mix_from_the_left_with_two_guides_is_caught():
    rs = np.random.RandomState(13)
    differs = 0
    for _ in range(10):
        zs = [_logits(rs), _logits(rs), _logits(rs)]
        v = (0.7, 0.3, -0.2)
        a, b = mr.mix32(zs, v), mr.mix32(zs, v, mix_left=True)
        assert np.allclose(a, b, rtol=0, atol=1e-4)
        differs += a.tobytes() != b.tobytes()
    assert differs == 10, differs  # some of 256 logits round differently every time: the trace comparison sees it
    zs = [_logits(rs), _logits(rs)]
    assert mr.mix32(zs, (0.7, 0.3)).tobytes() == mr.mix32(zs, (0.7, 0.3), mix_left=True).tobytes()  # (one guide: the same sum)
