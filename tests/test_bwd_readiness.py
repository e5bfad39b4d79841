"""-m gpu: two handles with one seed give bit-identical losses and parameters where the launch boundary dominates the
backward recurrence -- short windows, many launches.

What this guards: k_bwd_scatter's product waves take the operands of the dWhy sums from a three-deep LDS ring that wave 11
stages; a wave that falls a step behind the others of its workgroup used to find its slot staged over (one running release
count for the whole ring; now one per slot -- csrc/persistent.hip, BWDH_SYNC; tools/probes/wy_ring_sim.py).  How far the
waves drift apart is a matter of timing -- the readiness test of the elementwise waves as an unsigned maximum, 200 cycles
a step faster, turned a failure nobody had seen into one in every run at 512 x 20 x 60 -- so nothing here triggers it
deterministically: these are the shapes with the most launches per second and the least work between them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_TEXT = []


def _text():
    if not _TEXT:
        from bench import synthetic_text
        _TEXT.append(synthetic_text(200_000, seed=0))
    return _TEXT[0]


def _handle(lstm_hip, N, S, B):
    L = lstm_hip.Lstm(N, S, B)
    L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(1), N))
    L.set_text(_text())
    L.set_cursors(lstm_hip.initial_cursors(len(_text()), S, B))
    return L


def _run(lstm_hip, N, S, B, calls):
    L = _handle(lstm_hip, N, S, B)
    try:
        losses = [L.train_windows(c, 0.005) for c in calls]
        return np.concatenate(losses), L.get_params(), L.get_params(lstm_hip.P_MEM)
    finally:
        L.close()


def _same_bits(a, b):
    for x, y in zip(a, b):
        assert x.shape == y.shape
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), \
            f"first differing entry: {int(np.argmax(x.view(np.uint32) != y.view(np.uint32)))} of {x.size}"


@pytest.mark.parametrize("N,S,B,windows", [
    (512, 3, 8, 400),      # one hand-off per launch
    (512, 4, 60, 400),     # ragged: the last group has a padded half
    (512, 5, 64, 400),     # the shortest window that uses a slot of the dy / h ring twice
    (256, 4, 40, 400),
    (512, 11, 96, 300),    # two launches per direction; the pinned second launch
    (512, 20, 60, 400),    # where the faster elementwise wave made the slow product wave's stale slot show in every run
])
def test_two_handles_one_seed_same_bits(N, S, B, windows):
    import lstm_hip
    a = _run(lstm_hip, N, S, B, [windows])
    b = _run(lstm_hip, N, S, B, [windows])
    assert np.all(np.isfinite(a[0]))
    _same_bits(a, b)


def test_alternating_short_calls_equal_one_long_call():
    """512 x 6 x 64, 200 windows: train_windows(1) and train_windows(7) alternately on one handle against a twin that runs
    the same windows in one call."""
    import lstm_hip
    N, S, B, windows = 512, 6, 64, 200
    calls, left = [], windows
    while left:
        c = min(1 if len(calls) % 2 == 0 else 7, left)
        calls.append(c)
        left -= c
    a = _run(lstm_hip, N, S, B, calls)
    b = _run(lstm_hip, N, S, B, [windows])
    assert np.all(np.isfinite(a[0])) and a[0].size == windows
    _same_bits(a, b)
