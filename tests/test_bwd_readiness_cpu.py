"""CPU: the dy / h staging ring of the dWhy sums in k_bwd_scatter with asynchronous waves (tools/probes/wy_ring_sim.py).

One release count per ring slot keeps every fetch on the step it wants, whichever product wave is slow and under random
schedules; the mutant with one running count for the whole ring -- the kernel until the race was found -- lets a fast wave's
releases of later steps stand in for a slow wave's missing one: the slow wave then finds the operands of the step three
behind the one it wanted (the ring is three deep), which is the pair of steps the GPU localisation named
(profiles/bwd_readiness/README.md)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sim():
    spec = importlib.util.spec_from_file_location("wy_ring_sim", os.path.join(ROOT, "tools", "probes", "wy_ring_sim.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_one_count_per_slot_is_safe_whichever_wave_is_slow(sim):
    for S in list(range(2, 40)) + [60, 100, 101, 102]:
        for lag in range(8):
            assert sim.run(S, "slot", laggard=lag) is None, (S, lag)
        for seed in range(8):
            assert sim.run(S, "slot", seed=seed) is None, (S, seed)


def test_one_running_count_lets_a_slow_wave_read_a_slot_staged_over(sim):
    # S - 4 >= 1: the first window length with a fourth staging, i.e. a slot that is used twice
    for S in (5, 6, 11, 20, 100):
        for lag in (0, 4, 7):
            bad = sim.run(S, "ring", laggard=lag)
            assert bad is not None, (S, lag)
            wave, wanted, found = bad
            assert wave == lag and found == wanted - 3, bad
    # and random schedules find it too, given a few tries
    assert any(sim.run(20, "ring", seed=seed) is not None for seed in range(200))
    # windows too short to use a slot twice have no such hole
    for S in (2, 3, 4):
        for lag in range(8):
            assert sim.run(S, "ring", laggard=lag) is None
