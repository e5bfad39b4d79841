"""No device: what tests/test_handle_sequences.py (-m gpu) runs is what it is meant to run, its helpers work, and the arithmetic
behind the hand-off counters' reset holds.

* the script table (tests/handle_sequence_cases.py) holds, as adjacent ops, every pair and condition the GPU file exists for;
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
        assert sc.needs in ("all", "adaptive", "inference")
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

    names = ("P_PARAMS", "P_GRADS", "P_MEM", "P_ADAM_V", "OPT_ADAGRAD", "OPT_ADAM", "STEP_KERNELS", "PAD_HIDDEN", "EINVAL")
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
    order = [c[0] for c in twin.calls]
    assert order[0] == "set_optimizer" and order[-1] == "set_optimizer_steps" and order.count("set_params") == (3 if adam else 2)
    # and a difference is found and named
    other = dict(snap, c=snap["c"].copy())
    other["c"][2, 1, 5] = np.nextafter(other["c"][2, 1, 5], np.float32(9))
    assert hr.first_difference(snap, other)[0] == "c"
    with pytest.raises(AssertionError, match=r"script x, op 3 T\(2\): 'c' differs \(1 of 240 elements differ, the first at flat index 117"):
        hr.assert_same(snap, other, "script x, op 3 T(2)")
    assert hr.first_difference(dict(a=np.float32([0.0])), dict(a=np.float32([-0.0])))[0] == "a"   # bytes, not values


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
