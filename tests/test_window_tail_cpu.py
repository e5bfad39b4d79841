"""The split window slide of the update launch against the one-workgroup k_slide_window, simulated on the
CPU (tools/probes/slide_split_sim.py): same cursors, ring rows, head and flat indices whatever the order of the workgroups."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "probes"))


@pytest.mark.parametrize("S,B,stride,text_len,n_index", [
    (100, 64, 1, 5000, 25),   # the headline window
    (32, 63, 1, 900, 8),
    (20, 12, 3, 400, 3),      # stride above 1: the newest entries are recomputed from the text
    (50, 32, 7, 3000, 7),
    (16, 20, 1, 16 + 5, 2),   # a text short enough to wrap every cursor every few windows
    (16, 20, 3, 16 + 4, 5),
    (5, 3, 4, 9, 1),          # stride S - 1: one step of the old window survives
    (2, 4, 1, 40, 3),         # the smallest window
])
def test_split_slide_equals_the_one_workgroup_slide(S, B, stride, text_len, n_index):
    import slide_split_sim as sim
    assert sim.run(S, B, stride, text_len, windows=3 * S + 7, n_index=n_index, seed=S + B) == 3 * S + 7
