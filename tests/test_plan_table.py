"""-m gpu: the engine plan of every shape class is the one tests/golden/plan_table.json pins.

plan_engine (csrc/persistent.hip) decides at create which form of each recurrence a handle runs, from the shape, the flags,
two environment switches and what the occupancy API says about the instantiations the handle would launch.  The golden table
was written on an MI355X by tools/plan_table.py with the library of the commit before the launchers and the occupancy
questions came to share one resolver per kernel; it holds lstm_hip_plan_identity()'s string, or the text of the create's
refusal, for hidden 64 to 1088 x 1 to 520 streams x seven flag sets at S = 3, and for hidden 256 / 512 / 1024 with 16
streams under the four settings of LSTM_HIP_FWD_HALVES / LSTM_HIP_BWD_HALVES.  Every case must give the same string, and the
cases between them must show every FwdForm and BwdForm value (csrc/kernels.h), so that no form's rule goes unpinned.
"""
import json
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import plan_table  # noqa: E402

pytestmark = pytest.mark.gpu

FORMS = 7  # FwdForm and BwdForm have seven values each (csrc/kernels.h)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "plan_table.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def table():
    return plan_table.table()


def test_every_plan_is_the_pinned_one(golden, table):
    assert sorted(table) == sorted(golden)
    wrong = {k: (table[k], golden[k]) for k in golden if table[k] != golden[k]}
    assert not wrong, f"{len(wrong)} of {len(golden)} plans differ (case: got, pinned): {dict(list(wrong.items())[:8])}"


def test_the_cases_show_every_form(golden, table):
    for t in (golden, table):
        forms = [re.search(r" fwd(\d+) bwd(\d+) ", v) for v in t.values() if not v.startswith("refused")]
        assert {int(m.group(1)) for m in forms} == set(range(FORMS))
        assert {int(m.group(2)) for m in forms} == set(range(FORMS))
