"""-m gpu: the whole frequency table k_code_head builds, read from the device and held to the model.

Round trips, batch independence and the trace's own consistency (tests/test_compress.py) cannot see a table that is a valid
partition but not the model's: encoder and decoder build the same one.  The trace gives only the coded byte's row, so a whole
table is read with the 256 streams prefix + bytes([b]), b = 0..255: their last trace rows are (cum_b, q_b, T) of the state
after `prefix`.  That state is taken from the generator (a call that draws nothing), the logits from the float32 master
parameters by the heads' sequential sum (tests/logits_ref.py), and every q_b must lie in the interval tests/code_table_ref.py
derives from the float64 statement of the rule; T and cum must be the sums of the device's own q.  The probes sit at the start
of the batch, across a workgroup boundary and at its end, among fillers of mixed length, at the smallest stream count of every
group size SB.  tests/golden/coder_v1.npz pins one code, so that a change of the arithmetic cannot pass unnoticed."""
import os

import numpy as np
import pytest

import code_table_ref as ct
import gpu_util as gu
import sampling_ref as sr
from logits_ref import logits32
from oracle_lib import split_params
from test_logit_processors import _group_rule

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 256
f32 = np.float32
TEXT = bytes(gu.text_bytes(9, 5))
PREFIXES = (0, 1, 2, 5, 9)
MAX_STREAMS = 4096


def _model(P, N):
    sp = split_params(np.asarray(P, f32), N)
    return np.asarray(sp["Why"], f32), np.asarray(sp["by"], f32).reshape(M)


def _batch(probes, K, sb, seed):
    """K texts.  probes: (prefix, pos) pairs; the 256 probes prefix + bytes([b]) stand at pos .. pos + 255.  Around them
    fillers of 0 .. 12 random bytes, so that some are empty, some end before the probes do and some are still coded at the
    probes' last step.  Where a first probe does not begin a workgroup, the probes' neighbours in their group are a stream
    that outlasts them, in another state, and one that has ended: by turns the group's first stream is a one-byte text and
    the stream just before the probes the long one, or the first stream the long one and the other empty."""
    rs = np.random.RandomState(seed)
    texts = [bytes(rs.randint(0, 256, size=int(rs.randint(0, 13))).astype(np.uint8)) for _ in range(K)]
    for i, (prefix, pos) in enumerate(probes):
        if pos % sb:
            long = bytes(rs.randint(0, 256, size=len(prefix) + 3).astype(np.uint8))
            first, before = ((b"\x20", long), (long, b""))[(seed + i) % 2]
            texts[pos - 1] = before
            texts[pos - pos % sb] = first  # (the same stream where sb = 2)
    for prefix, pos in probes:
        texts[pos:pos + M] = [prefix + bytes([b]) for b in range(M)]
    return texts


def _rows(L, probes, K, sb, seed):
    """per (prefix, pos) of probes: (cum_b, q_b, T) for b = 0..255 of the state after prefix, all from one encode call of K
    streams"""
    texts = _batch(probes, K, sb, seed)
    codes, bits, tr = L.encode(texts, trace=True)
    off = np.concatenate([[0], np.cumsum([len(t) for t in texts])])
    return [tr[off[pos:pos + M] + len(prefix)].astype(np.int64) for prefix, pos in probes]


def _check_table(rows, z, where):
    """(a) one T, the sum of the q; (b) cum is the running sum of the device's own q; (c) every q inside the interval of the
    float64 statement.  Returns (q, how many q differ from the float32 / libm statement, the largest difference)."""
    cum, q, T = rows[:, 0], rows[:, 1], rows[:, 2]
    assert (T == T[0]).all() and T[0] == q.sum(), (where, np.unique(T), int(q.sum()))
    assert np.array_equal(cum, np.concatenate([[0], np.cumsum(q)[:-1]])), where
    bad = ct.outside(q, z)
    lo, hi = ct.interval64(z)
    assert bad.size == 0, (where, [(int(m), int(q[m]) - 1, int(lo[m]), int(hi[m])) for m in bad[:8]])
    diff = np.abs(q - ct.table32(z)[0].astype(np.int64))
    return q, int((diff != 0).sum()), int(diff.max())


def _positions(K, sb):
    """where the 256 probes begin: the start of the batch, across workgroup boundaries (not a multiple of SB, so the first
    and the last probe share their workgroups with fillers), the end"""
    if K == M:
        return [0]
    mid = min(3 * sb + max(sb // 2, 1), K - M - 1) if K - M > 1 else 0
    return sorted({0, mid, K - M})


def _probe_handle(L, state_of, Why, by, K, sb, name, prefixes=PREFIXES):
    """every prefix at every position: asserts (a) (b) (c); returns (tables probed, q = 1 entries, the largest q, float32
    disagreements, their largest)"""
    n_tab = ones = top = n_diff = d_max = 0
    for n in prefixes:
        prefix = TEXT[:n]
        z = logits32(Why, by, state_of(prefix))
        for pos in _positions(K, sb):
            rows = _rows(L, [(prefix, pos)], K, sb, seed=1000 * n + pos)[0]
            q, nd, dm = _check_table(rows, z, (name, n, K, pos))
            n_tab += 1
            ones += int((q == 1).sum())
            top = max(top, int(q.max()))
            n_diff += nd
            d_max = max(d_max, dm)
    print(f"{name}: SB = {sb}, {K} streams: {n_tab} whole tables probed, every q inside its interval; {n_diff} of {n_tab * M} q "
          f"differ from the float32/libm statement, by at most {d_max}; q = 1 entries {ones}, largest q {top}")
    assert ones >= 1 and top > 1 << 15, (name, ones, top)  # (else the interval test is vacuous at one end)
    return n_tab, ones, top, n_diff, d_max


def _generator_state(L, N):
    """h after `prefix` from a call that draws nothing (zero for the empty prefix: byte 0 is coded with softmax(by))"""
    def state_of(prefix):
        if not prefix:
            return np.zeros(N, f32)
        return np.asarray(L.generate([prefix], count=0)[2], f32).reshape(N)
    return state_of


@pytest.mark.parametrize("sb", [1, 2, 4, 8, 16])
def test_whole_tables_at_every_group_size(sb):
    """N = 16, the smallest stream count gen_head_group (read from the source) maps to SB"""
    import lstm_hip
    N = 16
    group = _group_rule()
    K = 300 if sb == 1 else next(k for k in range(1, MAX_STREAMS + 1) if group(N, k) == sb)
    assert group(N, K) == sb and (sb == 1 or group(N, K - 1) == sb // 2)
    P = sr.peaked_params(N, seed=7, gain=16.0)
    Why, by = _model(P, N)
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(P)
    _probe_handle(L, _generator_state(L, N), Why, by, K, sb, f"N = {N}")
    L.close()


@pytest.mark.parametrize("N", [512, 1024])
def test_whole_tables_at_large_widths(N):
    """one batch of 4096 streams each: the largest SB the rule allows at that width, read from the source (16 at both: at
    N = 1024 the group's h fills the 64 KB of dynamic LDS exactly)"""
    import lstm_hip
    K = MAX_STREAMS
    sb = _group_rule()(N, K)
    assert sb >= 8
    P = sr.peaked_params(N, seed=7, gain=12.0)
    Why, by = _model(P, N)
    L = lstm_hip.Lstm(N, 2, 1)
    L.set_params(P)
    state_of = _generator_state(L, N)
    # one batch: the five prefixes' probes in it together, at the start, across workgroup boundaries and at the end
    probes = list(zip([TEXT[:n] for n in PREFIXES], [0, 512 + sb // 2, 1024 + sb // 2 + 1, 2048 - 3, K - M]))
    ones = top = 0
    for (prefix, pos), rows in zip(probes, _rows(L, probes, K, sb, seed=N)):
        q, nd, dm = _check_table(rows, logits32(Why, by, state_of(prefix)), (N, len(prefix), pos))
        print(f"N = {N}: SB = {sb}, prefix {len(prefix)} at {pos}: whole table probed, every q inside its interval; {nd} of 256 q "
              f"differ from the float32/libm statement, by at most {dm}")
        ones += int((q == 1).sum())
        top = max(top, int(q.max()))
    L.close()
    assert ones >= 1 and top > 1 << 15, (ones, top)


def test_whole_tables_of_a_bf16_handle():
    """LSTM_HIP_BF16_RECURRENCE: the coder reads the float32 master parameters only, so the tables are those of the float32
    model on the float32 states (taken from a float32 handle with the same parameters)"""
    import lstm_hip
    N, K = 256, 512
    sb = _group_rule()(N, K)
    P = sr.peaked_params(N, seed=7, gain=12.0)
    Why, by = _model(P, N)
    F = lstm_hip.Lstm(N, 2, 1)
    F.set_params(P)
    L = lstm_hip.Lstm(N, 2, 8, flags=lstm_hip.BF16_RECURRENCE)
    L.set_params(P)
    _probe_handle(L, _generator_state(F, N), Why, by, K, sb, "bf16 N = 256")
    L.close()
    F.close()


def test_whole_tables_of_a_padded_handle():
    """LSTM_HIP_PAD_HIDDEN at N = 500: the tables are those of the logical parameters (the padding adds exact zeros)"""
    import lstm_hip
    N, K = 500, 512
    sb = _group_rule()(512, K)
    P = sr.peaked_params(N, seed=7, gain=12.0)
    Why, by = _model(P, N)
    L = lstm_hip.Lstm(N, 2, 1, flags=lstm_hip.PAD_HIDDEN)
    L.set_params(P)
    _probe_handle(L, _generator_state(L, N), Why, by, K, sb, "padded N = 500")
    L.close()


# ---- the pinned code -------------------------------------------------------------------------------------------------------
def test_the_pinned_code_of_coder_version_1():
    """tests/golden/coder_v1.npz (tests/golden/make_fixtures.py coder): four texts, and the codes and the trace an MI355X build
    made of them on fixture A's model"""
    import lstm_hip
    g = np.load(os.path.join(ROOT, "tests", "golden", "coder_v1.npz"))
    fx = gu.fixture("A")
    texts = [g["texts"][int(a):int(b)].tobytes() for a, b in zip(g["text_off"][:-1], g["text_off"][1:])]
    want = [g["codes"][int(a):int(b)].tobytes() for a, b in zip(g["code_off"][:-1], g["code_off"][1:])]
    assert [len(t) for t in texts] == [512, 0, 1, 64] and texts[0] == fx["text"][:512].tobytes()
    why = ("the coder's arithmetic has changed: either lstm_hip_coder_version() must change (and this fixture be remade with "
           "tests/golden/make_fixtures.py coder), or the cause must be found and fixed")
    assert lstm_hip.coder_version() == int(g["coder_version"]), why
    L = lstm_hip.Lstm(fx["N"], 2, 1)  # (no LSTM_HIP_FAST_MATH)
    L.set_params(fx["params"])
    codes, bits, tr = L.encode(texts, trace=True)
    back = L.decode(want, [len(t) for t in texts])
    L.close()
    first = next((int(i) for i in np.nonzero((tr != g["trace"]).any(axis=1))[0]), None)
    assert first is None, f"trace row {first}: {tr[first]} for the stored {g['trace'][first]}; {why}"
    assert codes == want, why
    assert back == texts, why
