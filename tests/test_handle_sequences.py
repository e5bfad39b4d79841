"""-m gpu: long-lived handles.  Mixed call sequences against a fresh-handle replay, bit for bit.

A handle that lives through a real run carries state the caller cannot see: the images of U and Why (packed when a flag says
stale, or rewritten by the update launch itself), the hand-off rings and launch counters, the window loop's carried slide and
loss tail, the scratch memory of the inference calls, the evaluator's own handle.  The contract: none of it may
show.  For every op k of a script (tests/handle_sequence_cases.py) the long-lived handle A is snapshot through the public
wrapper (tests/handle_replay.py), op k runs on A and on a fresh handle restored from the snapshot, and the op's outputs and
the snapshots after it must be the same bytes.  No tolerance anywhere.

The first seven scripts hold the state of the window loop, the optimizers and the inference calls.  The seven after them hold
what the features added since carry across calls: the image flags under weight drop, the accumulator and its pending count
across loops, the running average and the inference source, the text windows' softmax form, weights and ring, eval_texts'
cached handle on the shared scratch, and a borrowed teacher that trains itself between its student's calls.  The snapshot
holds their observable state (a student's includes its teacher's), and a twin restored with texts has run a text window of
its own to reach `next`, so a stream window of such a handle is also replayed on a twin that never heard of the texts.
Two handles, one device: every op ends synchronised and work of two handles is never in flight together (handle_replay).

The module takes 78 s on an MI355X: 197 cases, 1.3 s the longest (profiles/handle_sequences/run.jsonl; seeded faults that
the new scripts catch: profiles/handle_sequences/seeded_faults.txt).

The hand-off counters' reset (every 2^26 launches) is made reachable by LSTM_HIP_EPOCH_LIMIT: a script under limit 1 and 3
must give the bits of the default limit, with the "counter_resets" row of the kernel statistics proving the path ran.

Report: HANDLE_SEQUENCES_REPORT=profiles/handle_sequences/run.jsonl pytest -m gpu tests/test_handle_sequences.py
"""
import json
import os
import time

import numpy as np
import pytest

import handle_replay as hr
import handle_sequence_cases as hsc
from input_stats_cases import assert_plan

pytestmark = pytest.mark.gpu


def _report(row):
    path = os.environ.get("HANDLE_SEQUENCES_REPORT")
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a") as f:
            f.write(json.dumps(row) + "\n")


def _text(n):
    from bench import synthetic_text
    return synthetic_text(n, seed=3)


@pytest.mark.parametrize("case", hsc.CASES, ids=hsc.case_id)
def test_every_op_replays_on_a_fresh_handle(case):
    script, shape = case
    t0 = time.time()
    text = _text(script.text_len)
    A = hr.start(shape, text)
    twin, twins, ctx = None, 0, {}
    try:
        plan = assert_plan(A, shape.plan)
        # the premise: for identical state the twin's first forward is A's
        twin = hr.restore(shape, hr.snapshot(A, text))
        assert twin.plan_identity() == plan
        A.forward()
        A.synchronize()   # (two handles, one device: never work of both in flight)
        twin.forward()
        twin.synchronize()
        before = hr.snapshot(A, text)
        hr.assert_same(dict(before, loss=np.array([A.loss()])), dict(hr.snapshot(twin, text), loss=np.array([twin.loss()])),
                       f"{script.name} on {hsc.shape_id(shape)}: the first forward")
        hr.close(twin)
        twin = None
        twins += 1
        for k, op in enumerate(script.ops):
            where = f"{script.name} on {hsc.shape_id(shape)}, op {k} {hr.op_name(op)} after {[hr.op_name(o) for o in script.ops[:k]]}"
            out_a = hr.run_op(A, op, ctx)
            twin = hr.restore(shape, before)
            twins += 1
            out_t = hr.run_op(twin, op, ctx, twin=True)
            hr.assert_same(out_a, out_t, where + ", outputs")
            after, after_t = hr.snapshot(A, text), hr.snapshot(twin, text)
            assert set(after) == set(after_t), (where, sorted(set(after) ^ set(after_t)))
            hr.assert_same(after, after_t, where + ", the state it leaves")
            if op[0] in hr.INFERENCE or op[0] == "BAD":
                hr.assert_same(before, after, where + ", which must leave the handle as it was")
            hr.close(twin)
            twin = None
            if op[0] in ("T", "W", "FB") and "tt_text" in before:
                # only train_text_windows reads what set_train_texts gave the handle: a twin that never heard of the texts
                # (and so never ran a text window, as the first twin's positioning run did) gives the same window
                twin = hr.restore(shape, hr.without_texts(before))
                twins += 1
                out_t = hr.run_op(twin, op, ctx, twin=True)
                hr.assert_same(out_a, out_t, where + ", outputs, against a twin without the texts")
                hr.assert_same(after, hr.snapshot(twin, text), where + ", the state it leaves, against a twin without the texts")
                hr.close(twin)
                twin = None
            before = after
    finally:
        hr.close(A)
        if twin is not None:
            hr.close(twin)
    _report(dict(test="replay", script=script.name, shape=hsc.shape_id(shape), forms=shape.forms, ops=[hr.op_name(o) for o in script.ops],
                 twins=twins, seconds=round(time.time() - t0, 2), plan=plan))


def _run_script(shape, script, text, limit=None):
    """The script on one handle (created under the limit): every op's outputs, the final snapshot, resets counted, plan."""
    env = dict(shape.env, **({"LSTM_HIP_EPOCH_LIMIT": str(limit)} if limit is not None else {}))
    L = hr.start(shape._replace(env=env), text)
    try:
        plan = assert_plan(L, shape.plan)
        outs = [hr.run_op(L, op, {}) for op in script.ops]
        resets = L.kernel_stats()["counter_resets"]
        assert resets[1] == 0.0
        return outs, hr.snapshot(L, text), resets[0], plan
    finally:
        L.close()


@pytest.fixture(scope="module")
def default_limit_runs():
    cache = {}

    def get(shape):
        key = hsc.shape_id(shape)
        if key not in cache:
            cache[key] = _run_script(shape, hsc.EPOCH_SCRIPT, _text(hsc.EPOCH_SCRIPT.text_len))
        return cache[key]
    return get


@pytest.mark.parametrize("shape,limit", hsc.EPOCH_CASES, ids=lambda v: hsc.shape_id(v) if isinstance(v, tuple) else f"limit{v}")
def test_counter_reset_changes_no_bit(shape, limit, default_limit_runs):
    """Limit 1: every launch after a direction's first clears its counters first; limit 3: every third (on the several-launch
    rows the epoch also advances inside a window, behind the check, so they reset more often).  A hand-off that timed out
    would raise (LSTM_HIP_ESTATE)."""
    t0 = time.time()
    script = hsc.EPOCH_SCRIPT
    ref_outs, ref_snap, ref_resets, plan = default_limit_runs(shape)
    assert ref_resets == 0
    outs, snap, resets, plan_l = _run_script(shape, script, _text(script.text_len), limit)
    assert plan_l == plan
    for k, (a, b) in enumerate(zip(ref_outs, outs)):
        hr.assert_same(a, b, f"{script.name} on {hsc.shape_id(shape)}, limit {limit} against the default, op {k} {hr.op_name(script.ops[k])}")
    hr.assert_same(ref_snap, snap, f"{script.name} on {hsc.shape_id(shape)}, limit {limit} against the default, the final state")
    # per direction: launch k + 1 of a handle finds epoch >= limit at the latest when k is a multiple of the limit
    implied = 2 * ((hsc.windows(script.ops) - 1) // limit)
    assert implied > 0 and resets >= implied, (resets, implied)
    _report(dict(test="epoch_limit", script=script.name, shape=hsc.shape_id(shape), forms=shape.forms, limit=limit,
                 ops=[hr.op_name(o) for o in script.ops], twins=0, resets=int(resets), resets_implied=implied,
                 seconds=round(time.time() - t0, 2), plan=plan))


@pytest.mark.parametrize("value", ["0", "-1", "67108865", "abc", "3x", ""])
def test_epoch_limit_outside_its_range_is_refused_at_create(value, monkeypatch):
    import lstm_hip
    monkeypatch.setenv("LSTM_HIP_EPOCH_LIMIT", value)
    with pytest.raises(lstm_hip.LstmHipError, match=rf"error {lstm_hip.EINVAL}: LSTM_HIP_EPOCH_LIMIT"):
        lstm_hip.Lstm(128, 5, 16)


def test_epoch_limit_accepts_its_default(monkeypatch):
    import lstm_hip
    monkeypatch.setenv("LSTM_HIP_EPOCH_LIMIT", str(1 << 26))
    L = lstm_hip.Lstm(128, 5, 16)
    assert L.kernel_stats()["counter_resets"] == (0, 0.0)
    L.close()
