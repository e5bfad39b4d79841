"""The scripts and shapes of tests/test_handle_sequences.py (-m gpu), as data; tests/test_handle_sequences_cpu.py checks that
the table holds what it is meant to hold.

A script is a fixed list of ops (tests/handle_replay.py: run_op) with the length of the text it runs on; nothing is drawn at
run time, so a failure reproduces.  A shape is one row per pair of recurrence forms: N, B, flags and environment of the row
of param_stats_cases.SHAPES with those forms (the plan depends on N, B, flags and the CU count only), the window cut to an odd
S between 5 and 9 so that the hand-off rings' slots walk through every residue from launch to launch.

The first seven scripts are those of the first version of the test and stay as they are.  The seven behind them mix the
features added since (weight drop, accumulation, averaging and the inference source, text windows, eval_texts, soft targets
with a borrowed teacher) into stream windows on one handle; each is listed with the adjacent runs it exists for in
tests/test_handle_sequences_cpu.py (NEW_RUNS).
"""
import collections

import param_stats_cases as psc
from param_stats_cases import FWD_PERSISTENT, FWD_COLS8, FWD_TWO_HALF, FWD_BF16, FWD_BF16_HALVES, FWD_STEP, FWD_SMALL, \
    BWD_STEP, BWD_SMALL, BWD_PERSISTENT, BWD_COLS8, BWD_SCATTER, BWD_BF16, BWD_BF16_SCATTER, HALVES_OFF  # noqa: F401

Script = collections.namedtuple("Script", "name text_len ops needs")
# needs: "all" (every shape), "adaptive" (shapes of at most 64 streams: AD codes B streams), "inference" (INFERENCE_ROWS),
# "distill" (DISTILL_ROWS)
T1, T2, T3 = ("T", 1), ("T", 2), ("T", 3)
FB, W, RW = ("FB",), ("W",), ("RW",)
LONG, SHORT = 4000, 23   # SHORT: text_len - S is 14 to 18, every cursor wraps within a dozen windows

SCRIPTS = [
    # images written by the update launch against the twin's packed ones, in both orders, and invalidated images
    Script("images", LONG, [T2, FB, T1, W, W, T2, ("SP", 1), T2, T1, ("SP", 2), FB, ("SM", 1), T1, W, FB], "all"),
    Script("images_adaptive", LONG, [("AD", 1), T2, FB, T1, ("AD", 2), W, T1, ("SP", 3), ("AD", 3), T2, ("AD", 4), ("G", 5),
                                     ("AD", 5), T1, ("G", 4)], "adaptive"),
    # one handle through all four combinations of loss tail and carried slide, and every other setting of the loop
    Script("clip_profile", LONG, [T2, ("CLIP", 1), T3, ("CLIP", 0), T2, ("PROF", 1), T3, ("PROF", 0), T2, T1, T2, T3, FB,
                                  ("CLIP", 1), ("PROF", 1), T2], "all"),
    Script("optimizer_modes", SHORT, [("OPT", "adam"), T3, ("OPT", "adagrad"), T2, ("LM", 1), T2, ("LM", 2), T3, ("GB", 2), T2,
                                      ("ST", 3, 2), T3, ("CUR", 1), T2, RW, T3], "all"),
    # one scratch allocation under every inference call: the largest call first, then a smaller one of another kind
    # (no T between an EN and its DE: a code decodes with the parameters it was made with)
    Script("scratch_generate", LONG, [("G", 64), ("G", 3), ("BS", 1), ("G", 4), ("EN", 1), ("SC", 1), T2, ("G", 64), T1,
                                      ("G", 3), ("BS", 2), T1, ("G", 5), ("EN", 2), T2, ("SC", 2)], "inference"),
    Script("scratch_coders", LONG, [("SC", 3), ("BSC", 1), ("GC", 1), ("EN", 3), ("DE", 3), T2, ("SC", 4), T1, ("BSC", 2),
                                    ("GC", 2), T1, ("EN", 4), ("DE", 4), T1, ("GX", 1)], "inference"),
    # the evaluator's own handle and its copy of P; refused calls between calls that work
    Script("evaluator_refusals", LONG, [("EV", 1), T2, ("EV", 2), ("SA", 1), T1, ("SA", 2), T1, ("BAD", "stride"), T2,
                                        ("G", 6), ("BAD", "score_top_n"), ("SC", 5), ("BAD", "cursor"), T1, ("BAD", "clip"),
                                        FB], "inference"),
    # ---- the features added since the first seven scripts, each with state of its own ----
    # weight drop: the images alternate between the masked copy and the update launch's unmasked ones, and a host upload lands
    # mid-mask.  The head comes to the first WD(0) with every image flag set by a forward pass alone, on MASKED images (the
    # upload clears what the case's first forward left, the updates under the mask clear theirs): only set_weight_drop itself
    # can mark them stale there.  Further on the flags are the update launch's when the rate changes
    Script("drop_images", LONG, [("SP", 6), ("WD", .5), W, W, FB, ("WD", 0), T1, ("WD", .5), T2, FB, T1, ("SP", 4), T2, ("WD", 0),
                                 T1], "all"),
    # accumulation: accumulate-only windows between a carried slide and a fold, a cycle cut across T, W and call boundaries,
    # pending gradient discarded by a new pair; two refusals while it is on
    Script("accumulate", LONG, [("ACC", 3, 0), T1, ("SP", 5), T2, ("BAD", "acc_adaptive"), ("BAD", "acc_pending"), ("ACC", 3, 0), T1,
                                FB, T1, W, T2, ("ACC", 2, 1), T3, ("ACC", 1, 0), T2], "all"),
    # one mask per cycle, and the average takes the unmasked p; then clip and optimizer switched while a window is pending
    Script("drop_accumulate_average", LONG, [("WD", .5), ("ACC", 2, 0), ("AVG", "ema", 2), T3, FB, T1, ("WD", 0), T2,
                                             ("AVG", "uniform", 1), T2, ("AVG", "off"), T1, ("CLIP", 1), ("OPT", "adam"), T2], "all"),
    # text windows between stream windows (loss mode 0 throughout).  After RW the window has empty targets, the only columns
    # on which the text form of the softmax differs from the plain one; odd ids carry weights, which must not show in a T;
    # under ACC(2,0) one cycle spans train_windows and train_text_windows
    Script("texts_and_stream", LONG, [("TX", 3, 1), RW, T2, ("ACC", 2, 0), ("TX", 1, 2), T1, ("TXC", 1), RW, T2, ("ACC", 1, 0),
                                      ("TX", 2, 1), W, ("TXC", 2), FB, ("CUR", 2), T1], "all"),
    # every inference image is packed from a block that moved since the last call: the average, then the parameters again
    Script("averaged_inference", LONG, [("AVG", "ema", 1), T2, ("SRC", 1), ("G", 5), ("SC", 1), T1, ("G", 5), ("EVT", 0), ("EVT", 5),
                                        T1, ("EVT", 0), ("BS", 1), ("EN", 1), ("DE", 1), ("SRC", 0), ("G", 5)], "inference"),
    # eval_texts: its cached handle (remade when lanes changes, given the source block at every call), its pieces in the
    # scratch every inference call shares, never weight drop; and the average refused as a source before its first update
    Script("eval_texts_scratch", LONG, [("AVG", "ema", 1), ("BAD", "src_average_n0"), ("G", 64), ("EVT", 0), ("G", 3), ("EVT", 5),
                                        ("SC", 1), T1, ("EVT", 5), ("EV", 1), ("EVT", 0), ("WD", .5), T1, ("EVT", 0)], "inference"),
    # a borrowed teacher: smoothing alone, then distillation; the teacher trains itself between its student's calls (TTR)
    Script("distill", LONG, [("SOFT", "smooth"), T2, ("SOFT", "distill"), T2, FB, W, T1, ("TTR", 2), T2, ("TTR", 1), FB,
                             ("BAD", "text_windows_soft"), ("SOFT", "off"), T1], "distill"),
]
SCRIPT = {s.name: s for s in SCRIPTS}
# the counter reset (LSTM_HIP_EPOCH_LIMIT): every kind of window, single launches and loops, 10 windows per direction
EPOCH_SCRIPT = Script("epoch_reset", LONG, [T3, FB, FB, W, T2], "persistent")
EPOCH_LIMITS = (1, 3)


def windows(ops):
    """Forward (= backward) passes of a script: FB runs its window twice."""
    return sum(op[1] if op[0] == "T" else 2 if op[0] == "FB" else 1 if op[0] == "W" else 0 for op in ops)


Shape = collections.namedtuple("Shape", "forms N S B flags env plan")


def _row(forms, N, B, S, flags=(), env=None, plan=None):
    """The row of param_stats_cases.SHAPES with this N, B, flags and environment, at window S; plan: for the rows that table
    does not have."""
    env = dict(env or {})
    if plan is None:
        rows = [sh for sh in psc.SHAPES if (sh.N, sh.B, tuple(sh.flags), dict(sh.env)) == (N, B, tuple(flags), env)]
        assert rows, (forms, N, B, flags, env)
        plan = rows[0].plan
    return Shape(forms, N, S, B, tuple(flags), env, dict(plan))


BF = ("BF16_RECURRENCE",)
SHAPES = [
    _row("TwoHalf / Scatter, fused, 4-column pinned groups", 512, 24, 7),
    _row("TwoHalf / Scatter, several launches", 256, 272, 9),          # S * B = 2448 > 2048: the slide keeps its launch
    _row("Persistent / Cols8, fused", 128, 16, 5),
    _row("Cols8 / Cols8, fused, halves off", 512, 64, 7, env=HALVES_OFF),
    _row("Cols8 / Cols8, unfused", 1024, 16, 5),
    _row("TwoHalf / unfused Scatter, side stream", 256, 64, 9, ("NO_FUSED_GRADS",)),
    _row("Persistent / Persistent, 16-column groups", 128, 264, 7),
    _row("Bf16Halves / Bf16Scatter", 512, 64, 7, BF),
    _row("Bf16Halves / Bf16Scatter, direct dg image", 1024, 16, 5, BF),
    _row("Bf16Halves / Bf16Scatter, several launches", 256, 272, 9, BF),
    _row("Bf16 / Bf16, halves off", 256, 64, 5, BF, HALVES_OFF),
    _row("padded TwoHalf / Scatter", 500, 64, 7, ("PAD_HIDDEN",)),
    _row("padded Persistent / Cols8", 100, 16, 9, ("PAD_HIDDEN",)),
    _row("stable softmax, Persistent / Cols8", 128, 16, 7, ("STABLE_SOFTMAX",)),
    _row("fast math, Persistent / Cols8", 128, 16, 5, ("FAST_MATH",)),
    _row("control: Small / Small", 128, 1, 9),
    # (param_stats_cases has the per-step engine at 130 streams; the control needs no more than one column group)
    _row("control: Step / Step", 64, 8, 7, ("STEP_KERNELS",), plan=dict(fwd=FWD_STEP, bwd=BWD_STEP, fused=0)),
]
# inference reads the fp32 parameters only: one fp32 two-half row, one bf16 row, one padded row and the Step control
INFERENCE_ROWS = ("TwoHalf / Scatter, fused, 4-column pinned groups", "Bf16Halves / Bf16Scatter", "padded Persistent / Cols8",
                  "control: Step / Step")
# distillation: the fused fp32 two-half row, a bf16 row, a padded row, an unfused row and the Step control (the teacher is
# hidden 128 with default flags at the row's S and B, hidden 64 on the per-step engine for the control: handle_replay)
DISTILL_ROWS = ("TwoHalf / Scatter, fused, 4-column pinned groups", "Bf16Halves / Bf16Scatter", "padded Persistent / Cols8",
                "Cols8 / Cols8, unfused", "control: Step / Step")
ADAPTIVE_MAX_B = 64


def persistent(shape):
    """The rows whose recurrences count launches (EnginePlan::persistent(): every form but the per-step engine)."""
    return shape.plan.get("fwd") != FWD_STEP


def runs(script, shape):
    if script.needs == "adaptive":
        return shape.B <= ADAPTIVE_MAX_B
    if script.needs == "inference":
        return shape.forms in INFERENCE_ROWS
    if script.needs == "distill":
        return shape.forms in DISTILL_ROWS
    if script.needs == "persistent":
        return persistent(shape)
    return True


def shape_id(sh):
    tag = "".join("-" + f.lower() for f in sh.flags) + "".join(f"-{k[9:].lower()}{v}" for k, v in sorted(sh.env.items()))
    return f"{sh.N}x{sh.S}x{sh.B}{tag}"


CASES = [(sc, sh) for sc in SCRIPTS for sh in SHAPES if runs(sc, sh)]
EPOCH_CASES = [(sh, lim) for sh in SHAPES if persistent(sh) for lim in EPOCH_LIMITS]


def case_id(case):
    return f"{case[0].name}-{shape_id(case[1])}"
