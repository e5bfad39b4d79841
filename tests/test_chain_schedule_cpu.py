"""An equivalence about the scatter backward's readiness test (csrc/persistent.hip, bwds_elementwise), stated in numpy.

The elementwise wave takes a ring slot for complete when none of its 32 words is the sentinel HX_SENT = 0xFFFFFFFF, word by
word.  HX_SENT is the largest uint32, so "the UNSIGNED maximum of the 32 words is not the sentinel" says the same: the
maximum is the sentinel exactly when some word is.  A float maximum would not do: the sentinel is a NaN pattern, which a
float maximum drops, and negative floats order the other way round as integers.  The kernel does not use the maximum form:
as a v_max3_u32 chain it made the kernel 17 us a launch faster, and two handles with one seed then disagreed after some
hundred windows -- the arithmetic below is not where that came from.
"""
import numpy as np

HX_SENT = np.uint32(0xFFFFFFFF)
WORDS = 32  # eight 16-byte pieces per lane at N = 512


def word_by_word(v):
    """hx_ready of every piece: no word equals the sentinel (axis -1: the words of a lane)."""
    return (v != HX_SENT).all(axis=-1)


def by_maximum(v):
    """the form that was tried: the chain mx = max(max(mx, x), y) from 0 in load order, compared once"""
    mx = np.zeros(v.shape[:-1], np.uint32)
    for i in range(v.shape[-1]):
        mx = np.maximum(mx, v[..., i])
    return mx != HX_SENT


def test_every_value_of_one_word():
    """all 2^32 values of one word beside 31 words that are not the sentinel: ready everywhere but at the sentinel itself
    (about 6-10 s on one core: 16 GB of words in cache-sized chunks)"""
    rest = np.array([0, 1, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFFFFFFE, 0x80000000, 0x00000001], np.uint32)
    rest_max = rest.max()
    assert rest_max != HX_SENT
    step = 1 << 18                                       # (chunks that stay in the cache)
    low = np.arange(step, dtype=np.uint32)
    x, mx = np.empty(step, np.uint32), np.empty(step, np.uint32)
    not_ready = 0
    for lo in range(0, 1 << 32, step):
        np.bitwise_or(low, np.uint32(lo), out=x)         # lo is a multiple of step: the values lo .. lo + step - 1
        np.maximum(x, rest_max, out=mx)                  # the maximum with the other words
        a = x != HX_SENT                                 # word by word: the other words are ready
        b = mx != HX_SENT
        assert np.array_equal(a, b), hex(lo)
        not_ready += step - int(np.count_nonzero(b))
    assert not_ready == 1


def test_random_sets_with_the_sentinel_in_each_position():
    rs = np.random.RandomState(7)
    v = rs.randint(0, 1 << 32, size=(4096, WORDS), dtype=np.uint64).astype(np.uint32)
    v[v == HX_SENT] = 0
    # floats of both signs, denormals, infinities and NaNs that are not the sentinel
    v[:, ::5] = (rs.randn(4096, len(range(0, WORDS, 5))) * 1e3).astype(np.float32).view(np.uint32)
    v[::7, 3] = 0x00000001
    v[::11, 9] = 0xFF800000
    v[::13, 17] = 0xFFFFFFFE
    v[::17, 21] = 0x7FC00000
    assert word_by_word(v).all() and by_maximum(v).all()
    for pos in range(WORDS):
        w = v.copy()
        w[:, pos] = HX_SENT
        assert not word_by_word(w).any() and not by_maximum(w).any(), pos
    # several sentinels, as in a slot of which some pieces have not arrived
    w = v.copy()
    mask = rs.rand(*w.shape) < 0.1
    w[mask] = HX_SENT
    assert np.array_equal(word_by_word(w), by_maximum(w))
    assert np.array_equal(word_by_word(w), ~mask.any(axis=1))


def test_a_float_maximum_would_not_do():
    """why the kernel's maximum is an integer one: as floats the sentinel is a NaN, and fmax returns the other operand"""
    w = np.array([[1.0, -2.0]], np.float32).view(np.uint32).copy()
    w[0, 1] = HX_SENT
    assert not by_maximum(w)[0]
    assert np.fmax.reduce(w.view(np.float32), axis=-1).view(np.uint32)[0] != HX_SENT
