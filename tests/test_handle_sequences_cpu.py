"""No device: what tests/test_handle_sequences.py (-m gpu) runs is what it is meant to run, its helpers work, and the arithmetic
behind the hand-off counters' reset holds.

* the script table (tests/handle_sequence_cases.py) holds, as adjacent ops, every pair and condition the GPU file exists for;
  the first seven scripts are as they were, each later one holds its runs on its rows, and every op of the newer features
  meets the state it needs (a TX in loss mode 0 without soft targets, a refusal refused for the reason meant, ...);
* the stand-in zeroes and refuses as the library does, and the newer state (average, weight drop, accumulator, soft targets
  with a teacher, texts) round-trips through snapshot / restore in the order restore promises;
* every shape row names forms that exist, on rows of param_stats_cases.SHAPES, at an odd window of 5 to 9 steps;
* snapshot / restore (tests/handle_replay.py) round-trip on the tests/fake_gpu stand-in, taught to remember what it is given;
* the largest number of arrivals one hand-off counter receives in a launch, times the default epoch limit, stays inside 32 bits.
"""
import importlib.util
import os
import re
import types

import numpy as np
import pytest

import handle_replay as hr
import handle_sequence_cases as hsc
import input_stats_cases as isc
import param_stats_cases as psc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "eigen-lstm_amd", "csrc")


# ---- the script table ---------------------------------------------------------------------------------------------------
def _matches(op, pat):
    pat = (pat,) if isinstance(pat, str) else tuple(pat)
    return tuple(op[:len(pat)]) == pat


def _scripts_with(run, scripts=None):
    """Names of the scripts that hold `run` (op names, or tuples matched as a prefix of the op) as adjacent ops."""
    found = []
    for sc in scripts or hsc.SCRIPTS:
        ops = sc.ops
        if any(all(_matches(ops[i + j], p) for j, p in enumerate(run)) for i in range(len(ops) - len(run) + 1)):
            found.append(sc.name)
    return found


IMAGE_RUNS = [("T", "FB"), ("T", "W"), ("W", "T"), ("SP", "T"), ("T", "SP", "FB")]
ADAPTIVE_RUNS = [("AD", "T"), ("T", "AD")]
SWITCH_RUNS = [
    ("T", ("CLIP", 1), "T", ("CLIP", 0), "T"), ("T", ("PROF", 1), "T", ("PROF", 0), "T"),
    (("OPT", "adam"), "T", ("OPT", "adagrad"), "T"), (("LM", 1), "T"), (("LM", 2), "T"), (("GB", 2), "T"), (("ST", 3, 2), "T"),
    ("CUR", "T"), ("RW", "T"), (("T", 1), ("T", 2), ("T", 3)),
]
SCRATCH_RUNS = [(("G", 64), ("G", 3)), ("BS", "G"), ("EN", "SC"), ("SC", "BSC"), ("GC", "EN", "DE"), ("AD", "G")]
SCRATCH_RUNS_WITH_T = [(("G", 64), "T", ("G", 3)), ("BS", "T", "G"), ("EN", "T", "SC"), ("SC", "T", "BSC"), ("GC", "T", "EN", "DE"),
                       ("AD", "T", "G")]   # (between GC and EN; behind an EN the model must stay as it is until the DE)
EVALUATOR_RUNS = [("EV", "T", "EV"), ("SA", "T", "SA")]
REFUSAL_RUNS = [("T", "BAD", "T"), ("G", "BAD", "SC")]


@pytest.mark.parametrize("run", IMAGE_RUNS + SWITCH_RUNS, ids=str)
def test_every_shape_runs_the_image_and_loop_switch_pairs(run):
    names = _scripts_with(run)
    assert names, f"no script holds {run} as adjacent ops"
    for sh in hsc.SHAPES:
        assert any(hsc.runs(hsc.SCRIPT[n], sh) for n in names), (run, sh.forms)


@pytest.mark.parametrize("run", ADAPTIVE_RUNS, ids=str)
def test_adaptive_pairs_run_on_every_shape_of_at_most_64_streams(run):
    names = _scripts_with(run)
    assert names
    for sh in hsc.SHAPES:
        ran = any(hsc.runs(hsc.SCRIPT[n], sh) for n in names)
        assert ran == (sh.B <= hsc.ADAPTIVE_MAX_B), (run, sh.forms)
    for sc, sh in hsc.CASES:  # AD codes B streams: never on a wider row
        assert sh.B <= 64 or not any(op[0] == "AD" for op in sc.ops), (sc.name, sh.forms)


@pytest.mark.parametrize("run", SCRATCH_RUNS + SCRATCH_RUNS_WITH_T + EVALUATOR_RUNS + REFUSAL_RUNS, ids=str)
def test_scratch_evaluator_and_refusal_pairs_run_on_the_inference_rows(run):
    names = _scripts_with(run)
    assert names, f"no script holds {run} as adjacent ops"
    rows = [sh for sh in hsc.SHAPES if sh.forms in hsc.INFERENCE_ROWS]
    assert len(rows) == len(hsc.INFERENCE_ROWS) == 4
    for sh in rows:
        assert any(hsc.runs(hsc.SCRIPT[n], sh) for n in names), (run, sh.forms)


def test_inference_rows_are_one_two_half_one_bf16_one_padded_row_and_the_step_control():
    rows = {sh.forms: sh for sh in hsc.SHAPES if sh.forms in hsc.INFERENCE_ROWS}
    kinds = sorted(("bf16" if "BF16_RECURRENCE" in sh.flags else "padded" if "PAD_HIDDEN" in sh.flags else
                    "step" if "STEP_KERNELS" in sh.flags else "fp32 two-half" if sh.plan["fwd"] == psc.FWD_TWO_HALF else "?")
                   for sh in rows.values())
    assert kinds == ["bf16", "fp32 two-half", "padded", "step"]


def test_scripts_are_fixed_short_and_made_of_known_ops():
    assert len({sc.name for sc in hsc.SCRIPTS}) == len(hsc.SCRIPTS)
    for sc in hsc.SCRIPTS:
        assert 10 <= len(sc.ops) <= 16, (sc.name, len(sc.ops))
        assert sc.needs in ("all", "adaptive", "inference", "distill")
        for k, op in enumerate(sc.ops):
            assert op[0] in hr.OPS, op
            if op[0] == "T":
                assert 1 <= op[1] <= 3
            if op[0] == "G":
                assert 3 <= op[1] <= 64
            if op[0] == "BAD":
                assert op[1] in hr.BAD_CALLS
            if op[0] == "DE":  # decodes the code of the last EN before it, which has its text
                ens = [i for i, o in enumerate(sc.ops[:k]) if o[0] == "EN"]
                assert ens and sc.ops[ens[-1]][1:] == op[1:], (sc.name, k)
                between = [o[0] for o in sc.ops[ens[-1] + 1:k]]     # ... and nothing between them changes the model
                assert all(o in hr.INFERENCE or o == "BAD" for o in between), (sc.name, k, between)
    # a text short enough that every cursor wraps inside the script: at most 18 slides to the end, and more windows than that
    short = [sc for sc in hsc.SCRIPTS if sc.text_len - 9 <= 18 and sc.text_len > 9 + 1]
    assert short and all(sc.needs == "all" and hsc.windows(sc.ops) > sc.text_len - 5 for sc in short)
    assert [op[0] for op in hsc.EPOCH_SCRIPT.ops] == ["T", "FB", "FB", "W", "T"]
    assert hsc.EPOCH_SCRIPT.ops[0] == ("T", 3) and hsc.EPOCH_SCRIPT.ops[-1] == ("T", 2) and hsc.EPOCH_LIMITS == (1, 3)
    assert hsc.windows(hsc.EPOCH_SCRIPT.ops) == 10


# ---- the scripts of the features added since ------------------------------------------------------------------------------
WD5, WD0 = ("WD", .5), ("WD", 0)
NEW_RUNS = {   # script -> the adjacent runs it exists for
    "drop_images": [("T", WD5, "T", "FB", "T", "SP", "T", WD0, "T"), (WD5, "W", "W"), ("SP", WD5, "W", "W", "FB", WD0, "T")],
    "accumulate": [(("ACC", 3, 0), ("T", 1), "FB", ("T", 1), "W", ("T", 2), ("ACC", 2, 1), ("T", 3), ("ACC", 1, 0), ("T", 2)),
                   (("ACC", 3, 0), ("T", 1), "SP", ("T", 2)), (("BAD", "acc_adaptive"),), (("BAD", "acc_pending"),)],
    "drop_accumulate_average": [(WD5, ("ACC", 2, 0), ("AVG", "ema", 2), ("T", 3), "FB", ("T", 1), WD0, ("T", 2), ("AVG", "uniform", 1),
                                 ("T", 2), ("AVG", "off"), ("T", 1)), (("CLIP", 1), ("OPT", "adam"), "T")],
    "texts_and_stream": [("TX", "RW", "T"), ("TXC", "RW", "T"), (("ACC", 2, 0), "TX", ("T", 1), "TXC"),
                         (("TX", 1, 2), ("T", 1), ("TXC", 1), "RW", ("T", 2)), (("TX", 2, 1), "W", ("TXC", 2), "FB", "CUR", ("T", 1))],
    "averaged_inference": [(("AVG", "ema", 1), ("T", 2), ("SRC", 1), ("G", 5), ("SC", 1), ("T", 1), ("G", 5), ("EVT", 0), ("EVT", 5),
                            ("T", 1), ("EVT", 0), ("BS", 1), ("EN", 1), ("DE", 1), ("SRC", 0), ("G", 5))],
    "eval_texts_scratch": [(("G", 64), ("EVT", 0), ("G", 3), ("EVT", 5), ("SC", 1), ("T", 1), ("EVT", 5), ("EV", 1), ("EVT", 0), WD5,
                            ("T", 1), ("EVT", 0)), (("BAD", "src_average_n0"),)],
    "distill": [(("SOFT", "smooth"), ("T", 2), ("SOFT", "distill"), ("T", 2), "FB", "W", ("T", 1), ("TTR", 2), ("T", 2), ("TTR", 1), "FB"),
                ("FB", ("BAD", "text_windows_soft"), ("SOFT", "off"), ("T", 1))],
}
NEW_NEEDS = {"drop_images": "all", "accumulate": "all", "drop_accumulate_average": "all", "texts_and_stream": "all",
             "averaged_inference": "inference", "eval_texts_scratch": "inference", "distill": "distill"}


@pytest.mark.parametrize("name", sorted(NEW_RUNS))
def test_the_new_scripts_hold_their_runs_on_their_rows(name):
    sc = hsc.SCRIPT[name]
    assert sc.needs == NEW_NEEDS[name] and sc.text_len == hsc.LONG
    for run in NEW_RUNS[name]:
        assert _scripts_with(run, [sc]) == [name], f"{name} does not hold {run} as adjacent ops"
    rows = [sh.forms for sh in hsc.SHAPES if hsc.runs(sc, sh)]
    want = {"all": [sh.forms for sh in hsc.SHAPES], "inference": list(hsc.INFERENCE_ROWS), "distill": list(hsc.DISTILL_ROWS)}[sc.needs]
    assert sorted(rows) == sorted(want)
    # a text window with a weighted set before a stream window: the weights are scratch and must not show
    if name == "texts_and_stream":
        assert any(a[0] == "TX" and a[1] % 2 == 1 and b[0] == "T" for a, b in zip(sc.ops, sc.ops[1:]))


def test_the_old_scripts_are_the_first_seven_unchanged():
    assert [sc.name for sc in hsc.SCRIPTS[:7]] == ["images", "images_adaptive", "clip_profile", "optimizer_modes", "scratch_generate",
                                                   "scratch_coders", "evaluator_refusals"]
    assert [sc.name for sc in hsc.SCRIPTS[7:]] == ["drop_images", "accumulate", "drop_accumulate_average", "texts_and_stream",
                                                   "averaged_inference", "eval_texts_scratch", "distill"]
    new_ops = {"AVG", "SRC", "WD", "ACC", "SOFT", "TX", "TXC", "TTR", "EVT"}
    assert not any(op[0] in new_ops for sc in hsc.SCRIPTS[:7] for op in sc.ops)
    assert len(hsc.SHAPES) == 17 and len(hsc.CASES) == sum(hsc.runs(sc, sh) for sc in hsc.SCRIPTS[:7] for sh in hsc.SHAPES) + 17 * 4 + 4 * 2 + 5


def test_distill_rows_are_a_fused_a_bf16_a_padded_an_unfused_row_and_the_step_control():
    rows = {sh.forms: sh for sh in hsc.SHAPES if sh.forms in hsc.DISTILL_ROWS}
    assert sorted(hsc.shape_id(sh) for sh in rows.values()) == sorted(
        ["512x7x24", "512x7x64-bf16_recurrence", "100x9x16-pad_hidden", "1024x5x16", "64x7x8-step_kernels"])
    assert rows["Cols8 / Cols8, unfused"].plan["fused"] == 0 and rows["TwoHalf / Scatter, fused, 4-column pinned groups"].plan["fused"] == 1
    L = types.SimpleNamespace(S=7, B=8, _replay_cfg=hr.Config(64, 7, 8, ("STEP_KERNELS",), ()))
    assert hr.teacher_config(L) == hr.Config(64, 7, 8, ("STEP_KERNELS",), ())
    L = types.SimpleNamespace(S=9, B=16, _replay_cfg=hr.Config(100, 9, 16, ("PAD_HIDDEN",), ()))
    assert hr.teacher_config(L) == hr.Config(128, 9, 16, (), ())


def _walk(sc):
    """The settings a script has applied before each op, and the accumulator's pending count: (op index, op, state)."""
    st = dict(loss_mode=0, soft="off", acc=(1, 0), pending=0, wd=0, avg="off", avg_n=0, src=0, texts=None, tt_next=0, adam=False)
    for k, op in enumerate(sc.ops):
        yield k, op, dict(st)
        name = op[0]
        windows = op[1] if name == "T" else op[-1] if name in ("TX", "TXC") else 1 if name == "W" else 0
        if name == "TX":
            st.update(texts=op[1], tt_next=0)
        if name in ("TX", "TXC"):
            st["tt_next"] += windows
        updates = (st["pending"] + windows) // st["acc"][0]
        st["pending"] = (st["pending"] + windows) % st["acc"][0]
        if st["avg"] != "off":
            st["avg_n"] += updates   # (every script averages every update or every second one; n > 0 is what matters)
        if name == "LM":
            st["loss_mode"] = op[1]
        elif name == "SOFT":
            st["soft"] = op[1]
        elif name == "ACC" and tuple(op[1:]) != st["acc"]:
            st.update(acc=tuple(op[1:]), pending=0)
        elif name == "WD":
            st["wd"] = op[1]
        elif name == "AVG" and op[1] != st["avg"]:
            st.update(avg=op[1], avg_n=0, src=0)
        elif name == "SRC":
            st["src"] = op[1]
        elif name == "OPT":
            st["adam"] = op[1] == "adam"


def test_every_new_op_meets_the_state_it_needs():
    seen = set()
    for sc in hsc.SCRIPTS:
        for k, op, st in _walk(sc):
            name, where = op[0], (sc.name, k, op)
            seen.add(op[:2] if name == "BAD" else name)
            if name in ("TX", "TXC"):   # the text windows answer ESTATE otherwise
                assert st["loss_mode"] == 0 and st["soft"] == "off", where
                assert all(o[0] != "LM" and o[0] != "SOFT" for o in sc.ops[:k]), where
            if name == "TX":
                assert 1 <= op[2] <= 3 and op[1] >= 1, where
            if name == "TXC":   # more windows of the last TX's plan, which has three at least (train_texts)
                assert st["texts"] is not None and st["tt_next"] + op[1] <= 3, where
            if name == "TTR":
                assert st["soft"] == "distill" and 1 <= op[1] <= 3, where
            if name == "SRC" and op[1] == 1:
                assert st["avg"] != "off" and st["avg_n"] > 0, where
            if name == "AD":    # the adaptive coders answer ESTATE under any of these
                assert st["acc"][0] == 1 and st["wd"] == 0 and st["soft"] == "off" and st["src"] == 0, where
            if op[:2] == ("BAD", "acc_adaptive"):   # ... so that accumulation is the reason
                assert st["acc"][0] > 1 and st["wd"] == 0 and st["soft"] == "off" and st["src"] == 0, where
            if op[:2] == ("BAD", "acc_pending"):
                assert st["acc"][0] > 1, where
            if op[:2] == ("BAD", "src_average_n0"):
                assert st["avg_n"] == 0, where
            if op[:2] == ("BAD", "text_windows_soft"):
                assert st["soft"] != "off" and st["texts"] is None and st["loss_mode"] == 0, where
            if name == "WD":
                assert op[1] in (0, .5), where
            if name == "SOFT" and op[1] == "distill":
                assert st["wd"] == 0, where
    assert seen >= {"AVG", "SRC", "WD", "ACC", "SOFT", "TX", "TXC", "TTR", "EVT"} | {("BAD", b) for b in hr.BAD_CALLS if b not in ("loss_mode",)}
    # clip and the optimizer are switched while the accumulator holds a window, and a T follows
    hits = [(op, st["pending"]) for _, op, st in _walk(hsc.SCRIPT["drop_accumulate_average"]) if op in (("CLIP", 1), ("OPT", "adam"))]
    assert [h[0] for h in hits] == [("CLIP", 1), ("OPT", "adam")] and all(h[1] > 0 for h in hits)
    # accumulate: a cycle is cut by a W and by call boundaries, and both new pairs discard a pending window
    acc = list(_walk(hsc.SCRIPT["accumulate"]))
    assert any(op == ("W",) and st["pending"] == st["acc"][0] - 1 for _, op, st in acc)
    assert [st["pending"] for _, op, st in acc if op in (("ACC", 2, 1), ("ACC", 1, 0))] == [2, 1]
    # texts_and_stream: under ACC(2,0) the cycle that T(1) opens is closed by a text window
    tx = list(_walk(hsc.SCRIPT["texts_and_stream"]))
    assert any(op == ("TXC", 1) and st["acc"] == (2, 0) and st["pending"] == 1 for _, op, st in tx)
    # the weight-drop scripts switch it with a forward pass's masked images in place (FB, WD(0), T) and with the update
    # launch's unmasked ones (T, WD(.5), T)
    assert _scripts_with(("FB", WD0, "T")) and _scripts_with(("T", WD5, "T"))
    # ... and the first switch of a case finds no flag set (an upload right before it), so the first WD(0) is the first place
    # where only set_weight_drop's own clearing of the flags decides which images the next window reads
    assert [o[0] for o in hsc.SCRIPT["drop_images"].ops[:6]] == ["SP", "WD", "W", "W", "FB", "WD"]
    # eval_texts: the same lanes on both sides of a T (its cached handle lives on), other lanes in between (it is remade)
    for name in ("averaged_inference", "eval_texts_scratch"):
        ops = [o for o in hsc.SCRIPT[name].ops if o[0] in ("EVT", "T")]
        same_lanes = any(a[0] == "EVT" and b[0] == "T" and c == a for a, b, c in zip(ops, ops[1:], ops[2:]))
        assert same_lanes == (name == "eval_texts_scratch")   # (averaged_inference changes lanes across its T: a fresh copy)
        assert any(a[0] == b[0] == "EVT" and a != b for a, b in zip(ops, ops[1:])), name


def test_refused_calls_name_their_status():
    import lstm_hip
    assert list(hr.BAD_CALLS)[:5] == ["stride", "clip", "loss_mode", "score_top_n", "cursor"]
    assert all(hr.BAD_CALLS[b] == "EINVAL" for b in list(hr.BAD_CALLS)[:5])
    assert {b: hr.BAD_CALLS[b] for b in ("acc_adaptive", "src_average_n0", "text_windows_soft", "acc_pending")} == \
        dict(acc_adaptive="ESTATE", src_average_n0="ESTATE", text_windows_soft="ESTATE", acc_pending="EINVAL")
    assert lstm_hip.EINVAL != lstm_hip.ESTATE and set(hr.BAD_WORDS) <= set(hr.BAD_CALLS)
    assert "EVT" in hr.INFERENCE and not set(hr.INFERENCE) & set(hr.TRAINING + hr.STATE_EDITS)


@pytest.mark.parametrize("S,B", [(5, 16), (9, 272), (7, 1)])
def test_train_texts_start_continue_and_idle_within_the_plan(S, B):
    import lstm_hip
    for ident in (1, 2, 3):
        texts, weights = hr.train_texts(S, B, ident)
        again, _ = hr.train_texts(S, B, ident)
        assert texts == again and len(texts) == B + 3
        lengths = [len(t) for t in texts]
        assert max(lengths) == lengths[0] == 3 * (S - 1) + 1 and lengths[1:3] == [0, 1] and min(lengths) == 0
        assert (weights is not None) == (ident % 2 == 1)
        if weights is not None:
            assert all(w.dtype == np.float32 and w.size == n and (w >= 0).all() for w, n in zip(weights, lengths))
            assert (weights[0][2:4] == 0).all() and (weights[0][4:] > 0).any()   # zeros inside a text: context, not an end
        windows, lane_of, first = lstm_hip.text_plan(S - 1, B, lengths)
        assert windows >= 3 and lane_of[1] == lane_of[2] == -1
        if B > 1:   # in window 1 a lane continues its text, another starts one; B + 3 texts of which two have no step
            starts = {int(f) for f in first if f >= 0}
            assert 0 in starts and len(starts) > 1
    assert hr.train_texts(S, B, 1)[0] != hr.train_texts(S, B, 3)[0]


def test_op_seeds_depend_on_the_op_only():
    a, b = hr._rs(("G", 3)).random_sample(4), hr._rs(("G", 3)).random_sample(4)
    assert a.tobytes() == b.tobytes() and a.tobytes() != hr._rs(("G", 4)).random_sample(4).tobytes()
    p = hr._prompts(hr._rs(("GC", 1)), 64, 0, 20, ascii_only=True)
    assert len(p) == 64 and all(len(q) <= 20 and all(32 <= c < 128 for c in q) for q in p) and min(map(len, p)) == 0


# ---- the shapes ---------------------------------------------------------------------------------------------------------
FWD_FORMS = {isc.FWD_STEP, isc.FWD_SMALL, psc.FWD_PERSISTENT, psc.FWD_COLS8, psc.FWD_TWO_HALF, psc.FWD_BF16, psc.FWD_BF16_HALVES}
BWD_FORMS = {isc.BWD_STEP, isc.BWD_SMALL, isc.BWD_PERSISTENT, isc.BWD_COLS8, isc.BWD_SCATTER, isc.BWD_BF16, isc.BWD_BF16_SCATTER}
# the table of the issue: (fwd, bwd, N, B, flags, halves off)
TABLE = [
    (psc.FWD_TWO_HALF, isc.BWD_SCATTER, 512, 24, (), False), (psc.FWD_TWO_HALF, isc.BWD_SCATTER, 256, 272, (), False),
    (psc.FWD_PERSISTENT, isc.BWD_COLS8, 128, 16, (), False), (psc.FWD_COLS8, isc.BWD_COLS8, 512, 64, (), True),
    (psc.FWD_COLS8, isc.BWD_COLS8, 1024, 16, (), False), (psc.FWD_TWO_HALF, isc.BWD_SCATTER, 256, 64, ("NO_FUSED_GRADS",), False),
    (psc.FWD_PERSISTENT, isc.BWD_PERSISTENT, 128, 264, (), False),
    (psc.FWD_BF16_HALVES, isc.BWD_BF16_SCATTER, 512, 64, ("BF16_RECURRENCE",), False),
    (psc.FWD_BF16_HALVES, isc.BWD_BF16_SCATTER, 1024, 16, ("BF16_RECURRENCE",), False),
    (psc.FWD_BF16_HALVES, isc.BWD_BF16_SCATTER, 256, 272, ("BF16_RECURRENCE",), False),
    (psc.FWD_BF16, isc.BWD_BF16, 256, 64, ("BF16_RECURRENCE",), True),
    (psc.FWD_TWO_HALF, isc.BWD_SCATTER, 500, 64, ("PAD_HIDDEN",), False), (psc.FWD_PERSISTENT, isc.BWD_COLS8, 100, 16, ("PAD_HIDDEN",), False),
    (psc.FWD_PERSISTENT, isc.BWD_COLS8, 128, 16, ("STABLE_SOFTMAX",), False), (psc.FWD_PERSISTENT, isc.BWD_COLS8, 128, 16, ("FAST_MATH",), False),
    (isc.FWD_SMALL, isc.BWD_SMALL, 128, 1, (), False), (isc.FWD_STEP, isc.BWD_STEP, 64, 8, ("STEP_KERNELS",), False),
]


def test_shape_rows_name_forms_that_exist():
    import lstm_hip
    assert len({hsc.shape_id(sh) for sh in hsc.SHAPES}) == len(hsc.SHAPES)
    got = []
    for sh in hsc.SHAPES:
        assert sh.plan["fwd"] in FWD_FORMS and sh.plan["bwd"] in BWD_FORMS, sh
        assert sh.S % 2 == 1 and 5 <= sh.S <= 9, sh
        assert all(isinstance(getattr(lstm_hip, f), int) for f in sh.flags), sh
        assert sh.env in ({}, psc.HALVES_OFF), sh
        got.append((sh.plan["fwd"], sh.plan["bwd"], sh.N, sh.B, sh.flags, sh.env == psc.HALVES_OFF))
        if "STEP_KERNELS" not in sh.flags:  # N, B, flags, environment and plan of a row of param_stats_cases.SHAPES
            assert any((r.N, r.B, tuple(r.flags), dict(r.env), r.plan) == (sh.N, sh.B, sh.flags, sh.env, sh.plan) for r in psc.SHAPES), sh
    assert sorted(got) == sorted(TABLE)
    several = [sh for sh in hsc.SHAPES if sh.B == 272]
    assert len(several) == 2 and all(sh.S * sh.B > 2048 for sh in several)   # the slide keeps its own launch there
    assert sum(hsc.persistent(sh) for sh in hsc.SHAPES) == len(hsc.SHAPES) - 1
    assert len(hsc.EPOCH_CASES) == 2 * (len(hsc.SHAPES) - 1)
    # the direct dg image and the plain bf16 scatter row differ in what the plan says, as do the fused and unfused rows
    assert {sh.plan.get("dgt") for sh in hsc.SHAPES if sh.plan["bwd"] == isc.BWD_BF16_SCATTER} >= {0, 1}


# ---- snapshot / restore on the stand-in -----------------------------------------------------------------------------------
def _fake_module():
    """tests/fake_gpu/lstm_hip.py, its Lstm taught to remember what the real one keeps (the stand-in computes nothing and
    returns constants), under the real wrapper's constants."""
    import lstm_hip as real
    spec = importlib.util.spec_from_file_location("fake_gpu_lstm_hip", os.path.join(ROOT, "tests", "fake_gpu", "lstm_hip.py"))
    fake = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fake)

    class Remembering(fake.Lstm):
        def __init__(self, N, S, B, device=0, flags=0):
            super().__init__(N, S, B, device, flags)
            self.flags, self.calls = flags, []
            self.size = 4 * N * 256 + 4 * N * N + 4 * N + 256 * N + 256
            self.blocks = {w: np.zeros(self.size, np.float32) for w in (0, 1, 2)}
            self.kind, self.steps, self.numbers = real.OPT_ADAGRAD, 0, None
            self.h, self.c = np.zeros((S, B, N), np.float32), np.zeros((S, B, N), np.float32)
            self.xi, self.ti = np.full((S, B), -1, np.int32), np.full((S, B), -1, np.int32)
            self.pos, self.text, self.set = np.zeros(B, np.uint64), None, {}

        def set_params(self, p, which=0):
            assert which in self.blocks, which     # block 3 exists on Adam only
            self.calls.append(("set_params", which))
            self.blocks[which] = np.array(p, np.float32)

        def get_params(self, which=0): return self.blocks[which].copy()
        def set_state(self, t, h, c): self.h[t], self.c[t] = h, c
        def get_state(self, t): return self.h[t].copy(), self.c[t].copy()
        def set_text(self, t): self.text = np.array(t, np.uint8)
        def set_cursors(self, pos): super().set_cursors(pos); self.pos = np.array(pos, np.uint64)
        def get_cursors(self): return self.pos.copy()
        def set_window(self, xi, ti): super().set_window(np.asarray(xi), np.asarray(ti)); self.xi, self.ti = np.array(xi, np.int32), np.array(ti, np.int32)
        def get_window(self): return self.xi.copy(), self.ti.copy()
        def optimizer_steps(self): return self.steps
        def set_optimizer_steps(self, t): self.calls.append(("set_optimizer_steps",)); self.steps = t
        def set_stride(self, s, c=1): self.set["stride"], self.set["carry"] = s, c
        def set_loss_mode(self, m): self.set["loss_mode"] = m
        def set_global_batch(self, gb): self.set["global_batch"] = gb
        def set_grad_clip(self, x): self.set["clip"] = x
        def set_profiling(self, on): self.set["profiling"] = on

        def set_optimizer(self, kind, **numbers):
            self.calls.append(("set_optimizer", kind))
            if kind != self.kind:   # a new kind zeroes the optimizer state and the step count
                self.blocks[2] = np.zeros(self.size, np.float32)
                self.blocks.pop(3, None)
                if kind == real.OPT_ADAM:
                    self.blocks[3] = np.zeros(self.size, np.float32)
                self.kind, self.steps = kind, 0
            self.numbers = numbers

        # ---- the features added since: what the real handle keeps, with its zeroing rules and its refusals ----
        def _more(self):
            if not hasattr(self, "avg"):
                self.avg = dict(kind=real.AVG_OFF, decay=0.0, every=1, block=np.zeros(self.size, np.float32), seen=0, n=0, src=0)
                self.wd, self.accn, self.accb = (0.0, 0, 0), [1, False, 0], np.zeros(self.size, np.float32)
                self.soft, self.teacher, self.tt = (1.0, 1.0, 0.0), None, None
            return self

        def _refuse(self, status, what):
            raise real.LstmHipError(f"lstm_hip error {status}: {what}")

        def set_averaging(self, kind, decay=0.0, every=1):
            a = self._more().avg
            self.calls.append(("set_averaging", kind))
            if kind != a["kind"]:   # a new kind zeroes the block, the counts and the source
                a.update(kind=kind, block=np.zeros(self.size, np.float32), seen=0, n=0, src=real.SRC_PARAMS)
            a.update(decay=decay, every=every)

        def _averaging(self, what):
            if self._more().avg["kind"] == real.AVG_OFF:
                self._refuse(real.ESTATE, f"{what}: averaging is off")
            return self.avg

        def get_average(self): return self._averaging("get_average")["block"].copy()
        def set_average(self, block): self.calls.append(("set_average",)); self._averaging("set_average")["block"] = np.array(block, np.float32)
        def averaging_counts(self): a = self._averaging("averaging_counts"); return a["seen"], a["n"]

        def set_averaging_counts(self, seen, n):
            self.calls.append(("set_averaging_counts",))
            self._averaging("set_averaging_counts").update(seen=seen, n=n)

        def set_inference_source(self, source):
            a = self._more().avg
            self.calls.append(("set_inference_source", source))
            if source == real.SRC_AVERAGE and (a["kind"] == real.AVG_OFF or a["n"] == 0):
                self._refuse(real.ESTATE, "set_inference_source: LSTM_HIP_SRC_AVERAGE needs n >= 1")
            a["src"] = source

        def set_weight_drop(self, rate, seed=0, t=0): self._more().wd = (rate, seed, t); self.calls.append(("set_weight_drop",))
        def weight_drop(self): return self._more().wd

        def set_grad_accumulation(self, every, mean=False):
            self.calls.append(("set_grad_accumulation", every))
            if [every, bool(mean)] != self._more().accn[:2]:   # a new pair zeroes pending
                self.accn = [every, bool(mean), 0]

        def grad_accumulation(self): return tuple(self._more().accn)

        def grad_accumulator(self):
            if self._more().accn[0] == 1:
                self._refuse(real.ESTATE, "get_grad_accumulator: gradient accumulation is off")
            return self.accb.copy() if self.accn[2] else np.zeros(self.size, np.float32)

        def set_grad_accumulator(self, block, pending):
            self.calls.append(("set_grad_accumulator",))
            if self._more().accn[0] == 1:
                self._refuse(real.ESTATE, "set_grad_accumulator: gradient accumulation is off")
            if not 0 <= pending < self.accn[0]:
                self._refuse(real.EINVAL, "set_grad_accumulator: pending must be in range")
            self.accb, self.accn[2] = np.array(block, np.float32), pending

        def set_soft_targets(self, teacher=None, alpha=1.0, temperature=1.0, smoothing=0.0):
            self.calls.append(("set_soft_targets", teacher is not None))
            self._more().soft, self.teacher = (alpha, temperature, smoothing), teacher

        def soft_targets(self): return (self._more().teacher,) + self.soft

        def set_train_texts(self, texts, weights=None):
            self.calls.append(("set_train_texts", weights is not None))
            self._more().tt = None if not texts else dict(texts=list(texts), weights=weights, windows=7, next=0)

        def train_texts_progress(self): return self._more().tt["windows"], self.tt["next"]

        def train_text_windows(self, count, lr, want_losses=True, want_time=False):
            self.calls.append(("train_text_windows", count, lr))
            self._more().tt["next"] += count   # and it trains: the blocks and the step count move
            self.steps += count
            self.blocks[2] = self.blocks[2] + 1.0

        def synchronize(self): self.calls.append(("synchronize",))
        def close(self): self.closed = True

    names = ("P_PARAMS", "P_GRADS", "P_MEM", "P_ADAM_V", "OPT_ADAGRAD", "OPT_ADAM", "STEP_KERNELS", "PAD_HIDDEN", "EINVAL", "ESTATE",
             "AVG_OFF", "AVG_EMA", "AVG_UNIFORM", "SRC_PARAMS", "SRC_AVERAGE", "LstmHipError")
    return types.SimpleNamespace(Lstm=Remembering, **{n: getattr(real, n) for n in names})


@pytest.mark.parametrize("adam", [False, True])
def test_snapshot_and_restore_round_trip_on_the_stand_in(adam, monkeypatch):
    fake = _fake_module()
    cfg = hsc.Shape("stand-in", 16, 5, 3, ("STEP_KERNELS",), {"LSTM_HIP_FWD_HALVES": "0"}, {})
    monkeypatch.delenv("LSTM_HIP_FWD_HALVES", raising=False)
    rs = np.random.RandomState(1)
    L = hr.create(cfg, fake)
    assert L.flags == fake.STEP_KERNELS and "LSTM_HIP_FWD_HALVES" not in os.environ   # set for the create only
    text = rs.randint(0, 256, size=40).astype(np.uint8)
    hr.apply_setting(L, "optimizer", fake.OPT_ADAM if adam else fake.OPT_ADAGRAD, fake)
    for which in (0, 2) + ((3,) if adam else ()):
        L.set_params(rs.randn(L.size).astype(np.float32), which)
    L.set_optimizer_steps(17)
    L.set_text(text)
    L.set_cursors(rs.randint(5, 40, size=3).astype(np.uint64))
    L.set_window(rs.randint(-1, 256, size=(5, 3)), rs.randint(-1, 256, size=(5, 3)))
    for t in range(5):
        L.set_state(t, rs.randn(3, 16).astype(np.float32), rs.randn(3, 16).astype(np.float32))
    for key, value in (("stride", 3), ("carry", 2), ("loss_mode", 2), ("global_batch", 6), ("clip", 0.05), ("profiling", True)):
        hr.apply_setting(L, key, value, fake)
    snap = hr.snapshot(L, text)
    assert ("adam_v" in snap) == adam and snap["h"].shape == (5, 3, 16) and int(snap["steps"][0]) == 17
    twin = hr.restore(cfg, snap, fake)
    hr.assert_same(snap, hr.snapshot(twin, text), "the stand-in's round trip")
    assert set(snap) == set(hr.snapshot(twin, text))
    assert {k: twin.set[k] for k in ("stride", "carry", "loss_mode", "global_batch", "clip")} == \
        dict(stride=3, carry=2, loss_mode=2, global_batch=6, clip=0.05)
    assert "profiling" not in twin.set and twin.kind == L.kind and twin.numbers == L.numbers   # a twin never profiles
    # the order: the optimizer (a new kind zeroes state), then the blocks, then the step count
    order = [c[0] for c in twin.calls if c[0] in ("set_optimizer", "set_params", "set_optimizer_steps")]
    assert order[0] == "set_optimizer" and order[-1] == "set_optimizer_steps" and order.count("set_params") == (3 if adam else 2)
    # and a difference is found and named
    other = dict(snap, c=snap["c"].copy())
    other["c"][2, 1, 5] = np.nextafter(other["c"][2, 1, 5], np.float32(9))
    assert hr.first_difference(snap, other)[0] == "c"
    with pytest.raises(AssertionError, match=r"script x, op 3 T\(2\): 'c' differs \(1 of 240 elements differ, the first at flat index 117"):
        hr.assert_same(snap, other, "script x, op 3 T(2)")
    assert hr.first_difference(dict(a=np.float32([0.0])), dict(a=np.float32([-0.0])))[0] == "a"   # bytes, not values


def _stand_in_handle(fake, cfg, rs, text):
    L = hr.create(cfg, fake)
    L.set_params(rs.randn(L.size).astype(np.float32), 0)
    L.set_text(text)
    L._replay_text = text
    L.set_cursors(rs.randint(5, 40, size=cfg.B).astype(np.uint64))
    L.set_window(rs.randint(-1, 256, size=(cfg.S, cfg.B)), rs.randint(-1, 256, size=(cfg.S, cfg.B)))
    for t in range(cfg.S):
        L.set_state(t, rs.randn(cfg.B, cfg.N).astype(np.float32), rs.randn(cfg.B, cfg.N).astype(np.float32))
    return L


@pytest.mark.parametrize("teacher", [False, True])
def test_round_trip_of_the_newer_state_and_the_order_of_restore(teacher):
    fake = _fake_module()
    cfg = hsc.Shape("stand-in", 16, 5, 3, ("STEP_KERNELS",), {}, {})
    rs = np.random.RandomState(2)
    text = rs.randint(0, 256, size=40).astype(np.uint8)
    L = _stand_in_handle(fake, cfg, rs, text)
    texts, weights = hr.train_texts(5, 3, 1)
    if not teacher:   # (the text windows refuse soft targets: one or the other)
        hr.apply_setting(L, "texts", (texts, weights), fake)
        L.train_text_windows(2, 0.01)
    hr.apply_setting(L, "averaging", (fake.AVG_EMA, 0.9, 2), fake)
    L.set_average(rs.randn(L.size).astype(np.float32))
    L.set_averaging_counts(9, 4)
    hr.apply_setting(L, "infer_src", fake.SRC_AVERAGE, fake)
    L.set_weight_drop(0.5, 11, 6)
    L.set_grad_accumulation(3, True)
    L.set_grad_accumulator(rs.randn(L.size).astype(np.float32), 2)
    if teacher:
        T = _stand_in_handle(fake, hr.Config(8, 5, 3, (), ()), rs, rs.randint(0, 256, size=50).astype(np.uint8))
        hr.apply_setting(T, "clip", 0.05, fake)
        hr._set_teacher(L, T, alpha=0.5, temperature=2.0)
    else:
        hr._set_teacher(L, None, smoothing=0.1)
    snap = hr.snapshot(L)
    want = {"avg_kind", "avg_numbers", "average", "avg_counts", "infer_src", "weight_drop", "acc", "accumulator", "soft"}
    want |= {"teacher.cfg", "teacher.params", "teacher.h", "teacher.xi", "teacher.cursors", "teacher.text", "teacher.set_clip",
             "teacher.soft"} if teacher else {"tt_text", "tt_off", "tt_weights", "tt_progress"}
    assert want <= set(snap) and ("teacher.cfg" in snap) == teacher and ("tt_text" in snap) != teacher
    assert snap["acc"].tolist() == [3, 1, 2] and snap["weight_drop"].tolist() == [np.float64(0.5).view(np.uint64), 11, 6] and snap["avg_counts"].tolist() == [9, 4]
    assert snap["soft"].tolist() == ([0.5, 2.0, 0.0] if teacher else [1.0, 1.0, 0.1])
    if teacher:
        assert snap["teacher.h"].shape == (5, 3, 8) and snap["teacher.set_clip"][0] == 0.05
    else:
        assert snap["tt_progress"].tolist() == [7, 2] and snap["tt_off"].size == 3 + 3 + 1
    twin = hr.restore(cfg, snap, fake)
    again = hr.snapshot(twin)
    assert set(again) == set(snap)
    hr.assert_same(snap, again, "the stand-in's round trip of the newer state")
    assert twin.avg["src"] == fake.SRC_AVERAGE and twin.accn == [3, True, 2] and twin.wd == (0.5, 11, 6)
    order = [c[0] for c in twin.calls]
    if teacher:
        assert twin.teacher is not L.teacher and twin.teacher is twin._replay_teacher and twin.soft == (0.5, 2.0, 0.0)
        assert twin.teacher.set["clip"] == 0.05 and twin.teacher.N == 8
    else:
        # the order that matters: the texts and their positioning run come before everything they would overwrite
        assert order[:3] == ["set_train_texts", "train_text_windows", "synchronize"]
        assert twin.calls[1] == ("train_text_windows", 2, 0.0) and twin.calls[0] == ("set_train_texts", True)
        assert int(twin.steps) == int(snap["steps"][0]) == 2   # (the positioning run's own steps were overwritten)
        less = hr.restore(cfg, hr.without_texts(snap), fake)
        assert "train_text_windows" not in [c[0] for c in less.calls] and less.tt is None
        hr.assert_same(hr.without_texts(snap), hr.snapshot(less), "a twin without the texts")
    # ... the calls that zero state before the blocks and counts they zero; the source last
    for zeroing, block in (("set_averaging", "set_average"), ("set_averaging", "set_averaging_counts"),
                           ("set_grad_accumulation", "set_grad_accumulator"), ("set_optimizer", "set_params")):
        assert order.index(zeroing) < order.index(block), (zeroing, block)
    assert order[-1] == "set_inference_source" and order.index("set_averaging_counts") < len(order) - 1
    # averaging off: the kind only; accumulation off: the triple only
    hr.apply_setting(L, "averaging", (fake.AVG_OFF, 0.0, 1), fake)
    L.set_grad_accumulation(1, False)
    off = hr.snapshot(L)
    assert not {"average", "avg_counts", "avg_numbers", "infer_src", "accumulator"} & set(off) and off["acc"].tolist() == [1, 0, 0]
    assert hr.settings(L)["infer_src"] == fake.SRC_PARAMS
    twin2 = hr.restore(cfg, off, fake)
    hr.assert_same(off, hr.snapshot(twin2), "the round trip with averaging and accumulation off")
    for h in (twin, twin2, L):
        t = h._replay_teacher
        hr.close(h)
        assert h.closed and (t is None or t.closed)


def test_the_stand_in_zeroes_and_refuses_as_the_library_does():
    fake = _fake_module()
    L = hr.create(hsc.Shape("stand-in", 16, 5, 3, (), {}, {}), fake)
    with pytest.raises(fake.LstmHipError, match=f"error {fake.ESTATE}:"):
        L.get_average()
    with pytest.raises(fake.LstmHipError, match=f"error {fake.ESTATE}:"):
        L.grad_accumulator()
    L.set_averaging(fake.AVG_EMA, 0.9, 1)
    with pytest.raises(fake.LstmHipError, match=f"error {fake.ESTATE}:"):
        L.set_inference_source(fake.SRC_AVERAGE)   # n = 0
    L.set_average(np.ones(L.size, np.float32))
    L.set_averaging_counts(3, 3)
    L.set_inference_source(fake.SRC_AVERAGE)
    L.set_averaging(fake.AVG_EMA, 0.5, 2)   # the same kind keeps everything
    assert L.averaging_counts() == (3, 3) and L.avg["src"] == fake.SRC_AVERAGE and L.get_average()[0] == 1.0
    L.set_averaging(fake.AVG_UNIFORM, 0.0, 1)   # a new kind zeroes the block, the counts and the source
    assert L.averaging_counts() == (0, 0) and L.avg["src"] == fake.SRC_PARAMS and not L.get_average().any()
    L.set_grad_accumulation(3, False)
    L.set_grad_accumulator(np.ones(L.size, np.float32), 2)
    with pytest.raises(fake.LstmHipError, match=f"error {fake.EINVAL}:"):
        L.set_grad_accumulator(np.ones(L.size, np.float32), 3)
    L.set_grad_accumulation(3, False)    # the same pair keeps pending
    assert L.grad_accumulation() == (3, False, 2) and L.grad_accumulator()[0] == 1.0
    L.set_grad_accumulation(3, True)     # a new pair zeroes it
    assert L.grad_accumulation() == (3, True, 0) and not L.grad_accumulator().any()


def test_window_count_of_a_script():
    assert hsc.windows([("T", 3), ("FB",), ("W",), ("SP", 1), ("G", 3)]) == 3 + 2 + 1


# ---- the hand-off counters under the epoch limit ------------------------------------------------------------------------------
# Mirrors csrc/persistent.hip (checked against the source below): wait_arrivals expects `epoch * ceil((n_prod - lane) / SH)` on
# shard `lane` of a counter, SH = FWD_SH (64) forward and BWD_SH (8) backward; the producers of one counter are the
# workgroups of one column group: gridDim.x = N / 4 (k_fwd_persistent), 2 * (N / 8) (k_fwd_persistent2 and the bf16 forms
# of both), N / 16 (k_bwd_persistent, every storing wave for itself: `epoch * EW`, EW = 16 * COLS / 64 waves with COLS = 4, 8
# or 16 columns per group); persistent_supported and persistent_supported_bf16 refuse N > 1024.  The ring forms (TwoHalf,
# Scatter, Bf16Halves, Bf16Scatter) hand off through data and use the counters' memory for the (epoch << 4) | XCC id table only.
FWD_SH, BWD_SH, MAX_N, EPOCH_LIMIT, GROUP_COLS = 64, 8, 1024, 1 << 26, (4, 8, 16)


def _max_arrivals_per_counter():
    worst = 0
    for N in range(64, MAX_N + 1, 64):
        for n_prod in (N // 4, 2 * (N // 8)):
            worst = max(worst, -(-n_prod // FWD_SH))
        for cols in GROUP_COLS:
            worst = max(worst, -(-(N // 16) // BWD_SH) * (16 * cols // 64))
    return worst


def test_epoch_limit_keeps_the_counters_inside_32_bits():
    worst = _max_arrivals_per_counter()
    assert worst == 32   # hidden 1024, 16-column backward groups: 8 workgroups to a shard, 4 storing waves each
    assert EPOCH_LIMIT * worst < 2 ** 32
    assert EPOCH_LIMIT << 4 < 2 ** 32   # the XCC table's (epoch << 4) | id
    # on the several-launch rows the epoch advances inside a window, behind the check: by less than one per 4 columns
    assert (EPOCH_LIMIT + 4096 // 4) << 4 < 2 ** 32


def test_the_mirrored_constants_are_the_sources():
    src = open(os.path.join(CSRC, "persistent.hip")).read()
    assert re.search(r"#define FWD_SH (\d+)", src).group(1) == str(FWD_SH)
    assert re.search(r"#define BWD_SH (\d+)", src).group(1) == str(BWD_SH)
    assert "constexpr int ETH = 16 * COLS;" in src and "constexpr int EW = ETH / 64;" in src
    assert "expect = lane < CNT_SH ? epoch * (unsigned)((n_prod - lane + CNT_SH - 1) / CNT_SH) : 0u;" in src
    assert "wait_arrivals<BWD_SH>(cpn, NBK, epoch * EW, abortp, l)" in src
    assert len(re.findall(r"wait_arrivals<FWD_SH>\(cp, (?:NB|2 \* NB2), epoch, abortp, l\)", src)) == \
        len(re.findall(r"wait_arrivals<FWD_SH>", src)) == 4
    assert len(re.findall(r"wait_arrivals<", src)) == 5   # no other call
    for fn in ("persistent_supported", "persistent_supported_bf16"):
        body = src[src.index(f"static bool {fn}(int N"):]
        assert re.match(r"[^\n]*\n\s*if \(N % \d+ != 0 \|\| N > 1024\) return false;", body), fn
    assert "launch(r, dim3(N / 16, (B + cols - 1) / cols), st, Ubwd, DG, DHy," in src   # bwd_persistent's grid: NBK = N / 16
    rungs = re.findall(r"rung\(k_bwd_persistent<(?:NR4W|16), (\d+), [^>]*>, (\d+)", src)   # its resolver: columns, block size
    assert len(rungs) == 9 and {int(c) for c, _ in rungs} == set(GROUP_COLS) and {t for _, t in rungs} == {"512"}
    assert src.count("epoch << 4) | (__builtin_amdgcn_s_getreg") == src.count("<< 4) | (__builtin_amdgcn_s_getreg") == 6   # the XCC table
    # the limit: default 2^26 in the plan, read at create, and nothing else decides when the counters are cleared
    assert "unsigned epoch_limit = 1u << 26;" in open(os.path.join(CSRC, "kernels.h")).read()
    assert 'getenv("LSTM_HIP_EPOCH_LIMIT")' in src and "v < 1 || v > (1ll << 26)" in src
    api = open(os.path.join(CSRC, "lstm_hip_api.cpp")).read()
    assert api.count("_epoch >= p.epoch_limit") == 2 and "1u << 26" not in api
    assert api.count("h->counter_resets++;") == 2
