"""Helpers of tests/test_handle_sequences.py (-m gpu) and of its device-free control, tests/test_handle_sequences_cpu.py.

The contract under test: a fresh handle with the same config
and flags, loaded with a long-lived handle's observable state, behaves bit for bit like that handle -- whatever the long-lived
handle did before -- for every call and for the state the call leaves.  Observable state is what snapshot() reads through the
public wrapper: parameters, optimizer blocks, step count, optimizer kind and numbers; all S columns of h and c; the window's
indices, the text and the cursors; stride and carry column, loss mode, global batch and the clip setting.  Profiling is not
part of it: a twin never profiles, so a profiled window of the long-lived handle (separate loss, fold and slide launches) is
also compared with the carried forms of the same window.

The features added since are observable state too, each through its own getters where it has them and through the settings
this file tracks (settings()) where it has none:
  averaging        kind, decay and every (tracked), get_average(), averaging_counts(), the inference source (tracked); while
                   averaging is off the kind only, because the block calls answer ESTATE
  weight drop      weight_drop() = (rate, seed, t)
  accumulation     grad_accumulation() = (every, mean, pending) and grad_accumulator(); while off (every = 1) the triple only
  soft targets     soft_targets() = (alpha, temperature, smoothing) and, with a teacher, the TEACHER'S OWN SNAPSHOT (its config,
                   blocks, all S state columns, window, text, cursors, settings) under "teacher.": a borrowed teacher is part of
                   its student's observable state, and a twin gets a freshly restored teacher twin
  text windows     the texts and weights given to set_train_texts (tracked) and train_texts_progress()
The streams' prequential bits (train_texts_bits) have no setter and cannot be restored: they are an output of TX only, the op
that starts from a fresh set_train_texts, and never part of a snapshot.

restore() builds the twin in this order: create; the texts and a positioning run train_text_windows(next, 0.0) (`next` has no
setter; whatever that run leaves -- window, states, optimizer memory, step count -- is overwritten by what follows); the calls
that zero state (optimizer kind, averaging kind, weight drop, accumulation); the blocks and counts; text, cursors, window, all
S columns of h and c; stride, carry, loss mode, global batch, clip; soft targets with the teacher twin; the inference source
last, because the average must have n > 0 by then.

Two handles on one device: nothing orders the persistent grids of two handles, so run_op ends
with synchronize(), restore's positioning run is synchronised before anything else is created, and no caller of this file
queues work on a second handle (the twin; a teacher outside its student's own call) without a synchronise in between.

An op is a tuple (name, args...), see run_op.  Everything is seeded from the op itself, so a script (a list of ops,
tests/handle_sequence_cases.py) reproduces.  Nothing here needs a device to import; `lstm_hip` is passed in or imported late.
"""
import ast
import collections
import contextlib
import os
import zlib

import numpy as np

LR = 0.01
ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)
CLIP_ON = 0.05     # below the gradient norm of these windows (about 0.1 to 3), so the coefficient is applied
EMA_DECAY = 0.9
WD_SEED = 11       # the fixed seed of every WD op
SMOOTHING = 0.1
DISTILL = dict(alpha=0.5, temperature=2.0)
DEFAULT_SETTINGS = dict(stride=1, carry=1, loss_mode=0, global_batch=None, clip=0.0, optimizer=0, profiling=False,
                        averaging=(0, 0.0, 1), infer_src=0, texts=None, text_weights=None)
# settings a twin receives (profiling is the long-lived handle's own business, see above)
OBSERVABLE_SETTINGS = ("stride", "carry", "loss_mode", "global_batch", "clip", "optimizer")

TRAINING = ("T", "W", "FB", "TX", "TXC", "TTR")
STATE_EDITS = ("SP", "SM", "CUR", "RW", "ST", "LM", "GB", "CLIP", "PROF", "OPT", "AVG", "SRC", "WD", "ACC", "SOFT")
INFERENCE = ("G", "GX", "GC", "SC", "BS", "BSC", "EN", "DE", "EV", "SA", "EVT")
OPS = TRAINING + STATE_EDITS + INFERENCE + ("AD", "BAD")
# the refused calls and the status each must answer: the names of lstm_hip's constants
BAD_CALLS = collections.OrderedDict([
    ("stride", "EINVAL"), ("clip", "EINVAL"), ("loss_mode", "EINVAL"), ("score_top_n", "EINVAL"), ("cursor", "EINVAL"),
    ("acc_adaptive", "ESTATE"),        # encode_adaptive while accumulation is on
    ("src_average_n0", "ESTATE"),      # the average as inference source before it has taken an update
    ("text_windows_soft", "ESTATE"),   # train_text_windows while soft targets are on
    ("acc_pending", "EINVAL"),         # set_grad_accumulator with pending >= every
])
# a word of the library's message, where the status alone would not tell the refusal meant from another one
BAD_WORDS = {"acc_adaptive": "gradient accumulation", "text_windows_soft": "soft targets", "src_average_n0": "LSTM_HIP_SRC_AVERAGE",
             "acc_pending": "pending"}
AVG_KINDS = {"off": "AVG_OFF", "ema": "AVG_EMA", "uniform": "AVG_UNIFORM"}
Config = collections.namedtuple("Config", "N S B flags env")   # what create() reads of a shape row: a teacher's config


def _lib():
    import lstm_hip
    return lstm_hip


def op_name(op):
    return op[0] + ("(" + ",".join(str(a) for a in op[1:]) + ")" if len(op) > 1 else "")


def _rs(op, salt=0):
    return np.random.RandomState(zlib.crc32(repr((op, salt)).encode()) & 0x7FFFFFFF)


def settings(L):
    """The settings the script has applied to this handle (the wrapper has no getters for them)."""
    if not hasattr(L, "_replay_settings"):
        L._replay_settings = dict(DEFAULT_SETTINGS, global_batch=L.B)
    return L._replay_settings


@contextlib.contextmanager
def environment(env):
    """The plan's switches are read at create: set for the creation of one handle, then put back."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def create(cfg, lstm_hip=None):
    """A handle of cfg (.N .S .B .flags: names, .env), with default settings."""
    lh = lstm_hip or _lib()
    flags = 0
    for f in cfg.flags:
        flags |= getattr(lh, f)
    with environment(dict(cfg.env)):
        L = lh.Lstm(cfg.N, cfg.S, cfg.B, flags=flags)
    L._replay_cfg = Config(cfg.N, cfg.S, cfg.B, tuple(cfg.flags), tuple(sorted(dict(cfg.env).items())))
    L._replay_teacher = None
    return L


def close(L):
    """Closes a handle of create() and the teacher run_op or restore made for it (a teacher cannot go before its student)."""
    teacher = getattr(L, "_replay_teacher", None)
    L.close()
    L._replay_teacher = None
    if teacher is not None:
        teacher.close()


def _set_teacher(L, teacher, **numbers):
    """set_soft_targets, and the end of the teacher this handle held before."""
    old = L._replay_teacher
    L.set_soft_targets(teacher, **numbers)
    L._replay_teacher = teacher
    if old is not None and old is not teacher:
        old.close()


def apply_setting(L, key, value, lstm_hip=None):
    lh = lstm_hip or _lib()
    st = settings(L)
    if key == "averaging":     # (kind, decay, every); a new kind puts the inference source back to the parameters
        if value[0] != st["averaging"][0]:
            st["infer_src"] = lh.SRC_PARAMS
        L.set_averaging(int(value[0]), float(value[1]), int(value[2]))
        value = (int(value[0]), float(value[1]), int(value[2]))
    elif key == "infer_src":
        L.set_inference_source(int(value))
    elif key == "texts":       # (texts, weights or None), or None: no texts
        texts, weights = value if value is not None else (None, None)
        L.set_train_texts(texts, weights)
        st["text_weights"] = None if weights is None else [np.array(w, np.float32) for w in weights]
        value = None if texts is None else [bytes(t) for t in texts]
    elif key in ("stride", "carry"):
        st[key] = value
        L.set_stride(st["stride"], st["carry"])
    elif key == "loss_mode":
        L.set_loss_mode(value)
    elif key == "global_batch":
        L.set_global_batch(value)
    elif key == "clip":
        L.set_grad_clip(value)
    elif key == "profiling":
        L.set_profiling(value)
    elif key == "optimizer":
        if value == lh.OPT_ADAM:
            L.set_optimizer(lh.OPT_ADAM, **ADAM)
        else:
            L.set_optimizer(lh.OPT_ADAGRAD)
    else:
        raise KeyError(key)
    st[key] = value


def host_slide(xi, ti, pos, text, S, stride):
    """OV/lstm_eigen_opt/lstm.cc:190-213 on indices, `stride` times; in place (as tests/test_window_tail.py)."""
    for _ in range(stride):
        ev = text[pos.astype(np.int64)].astype(np.int32)
        pos += 1
        pos[pos >= len(text)] = S
        xi[:-1] = xi[1:].copy()
        ti[:-1] = ti[1:].copy()
        ti[S - 1] = ev
        xi[S - 1] = ti[S - 2]


def start(cfg, text, seed=5, lstm_hip=None):
    """The long-lived handle of a case: seeded parameters (by off zero), the text, spread cursors, a full first window and a
    random carry column."""
    lh = lstm_hip or _lib()
    N, S, B = cfg.N, cfg.S, cfg.B
    L = create(cfg, lh)
    rs = np.random.RandomState(seed)
    P = lh.init_params(lh.MT19937Normal(seed), N)
    P[-256:] = (rs.randn(256) * 0.01).astype(np.float32)
    L.set_params(P)
    text = np.ascontiguousarray(text, np.uint8)
    L.set_text(text)
    L._replay_text = text
    pos = np.array([S + (7 * b) % (len(text) - S) for b in range(B)], np.uint64)
    xi, ti = np.full((S, B), -1, np.int32), np.full((S, B), -1, np.int32)
    host_slide(xi, ti, pos, text, S, S)
    L.set_cursors(pos)
    L.set_window(xi, ti)
    L.set_state(1, (rs.randn(B, N) * 0.1).astype(np.float32), (rs.randn(B, N) * 0.1).astype(np.float32))
    return L


def snapshot(L, text=None):
    """Everything of the contract's observable state, read through the public wrapper (text: the handle's own, by default)."""
    lh = _lib()
    st = dict(settings(L))
    text = L._replay_text if text is None else text
    snap = dict(params=L.get_params(lh.P_PARAMS), mem=L.get_params(lh.P_MEM), steps=np.array([L.optimizer_steps()], np.int64))
    if st["optimizer"] == lh.OPT_ADAM:
        snap["adam_v"] = L.get_params(lh.P_ADAM_V)
    hs, cs = zip(*(L.get_state(t) for t in range(L.S)))
    snap["h"], snap["c"] = np.stack(hs), np.stack(cs)
    snap["xi"], snap["ti"] = L.get_window()
    snap["cursors"] = L.get_cursors()
    snap["text"] = np.array(text, np.uint8)
    for k in OBSERVABLE_SETTINGS:
        snap["set_" + k] = np.array([st[k]], np.float64)
    # averaging: off, the kind only (the block calls answer ESTATE)
    kind, decay, every = st["averaging"]
    snap["avg_kind"] = np.array([kind], np.int64)
    if kind != lh.AVG_OFF:
        snap["avg_numbers"] = np.array([decay, every], np.float64)
        snap["average"] = L.get_average()
        snap["avg_counts"] = np.array(L.averaging_counts(), np.int64)
        snap["infer_src"] = np.array([st["infer_src"]], np.int64)
    rate, seed, t = L.weight_drop()
    snap["weight_drop"] = np.array([np.float64(rate).view(np.uint64), seed, t], np.uint64)   # (the rate as its bits)
    every, mean, pending = L.grad_accumulation()
    snap["acc"] = np.array([every, int(mean), pending], np.int64)
    if every > 1:
        snap["accumulator"] = L.grad_accumulator()
    teacher, alpha, tau, eps = L.soft_targets()
    snap["soft"] = np.array([alpha, tau, eps], np.float64)
    if teacher is not None:   # a borrowed teacher is part of its student's observable state
        assert teacher is L._replay_teacher
        snap["teacher.cfg"] = np.frombuffer(repr(tuple(teacher._replay_cfg)).encode(), np.uint8)
        for k, v in snapshot(teacher).items():
            snap["teacher." + k] = v
    if st["texts"] is not None:
        parts = [np.frombuffer(t, np.uint8) for t in st["texts"]]
        snap["tt_text"] = np.concatenate(parts + [np.zeros(0, np.uint8)])
        snap["tt_off"] = np.cumsum([0] + [p.size for p in parts]).astype(np.int64)
        if st["text_weights"] is not None:
            snap["tt_weights"] = np.concatenate(list(st["text_weights"]) + [np.zeros(0, np.float32)]).astype(np.float32)
        snap["tt_progress"] = np.array(L.train_texts_progress(), np.int64)
    return snap


def without_texts(snap):
    """The snapshot less what set_train_texts gave the handle: only train_text_windows may read it."""
    return {k: v for k, v in snap.items() if not k.startswith("tt_")}


def restore(cfg, snap, lstm_hip=None):
    """A fresh handle loaded with a snapshot, in the order of the file's docstring.  Texts first: their positioning run trains,
    and everything it writes is overwritten below.  Then the calls that zero state, the blocks and counts they would zero, the
    window and states, the settings, the teacher, the inference source."""
    lh = lstm_hip or _lib()
    L = create(cfg, lh)
    if "tt_text" in snap:
        off = snap["tt_off"]
        texts = [snap["tt_text"][int(off[s]):int(off[s + 1])].tobytes() for s in range(off.size - 1)]
        weights = [snap["tt_weights"][int(off[s]):int(off[s + 1])] for s in range(off.size - 1)] if "tt_weights" in snap else None
        apply_setting(L, "texts", (texts, weights), lh)
        L.train_text_windows(int(snap["tt_progress"][1]), 0.0, want_losses=False)   # `next` has no setter
        L.synchronize()                                                              # ... before anything else is created
    apply_setting(L, "optimizer", int(snap["set_optimizer"][0]), lh)
    kind = int(snap["avg_kind"][0])
    if kind != lh.AVG_OFF:
        apply_setting(L, "averaging", (kind, float(snap["avg_numbers"][0]), int(snap["avg_numbers"][1])), lh)
    if "weight_drop" in snap:   # (a caller may take the numbers out of a snapshot and set its own)
        L.set_weight_drop(float(snap["weight_drop"][:1].view(np.float64)[0]), int(snap["weight_drop"][1]), int(snap["weight_drop"][2]))
    every, mean, pending = (int(v) for v in snap["acc"])
    L.set_grad_accumulation(every, bool(mean))
    L.set_params(snap["params"], lh.P_PARAMS)
    L.set_params(snap["mem"], lh.P_MEM)
    if "adam_v" in snap:
        L.set_params(snap["adam_v"], lh.P_ADAM_V)
    L.set_optimizer_steps(int(snap["steps"][0]))
    if kind != lh.AVG_OFF:
        L.set_average(snap["average"])
        L.set_averaging_counts(int(snap["avg_counts"][0]), int(snap["avg_counts"][1]))
    if every > 1:
        L.set_grad_accumulator(snap["accumulator"], pending)
    L.set_text(snap["text"])
    L._replay_text = np.array(snap["text"], np.uint8)
    L.set_cursors(snap["cursors"])
    L.set_window(snap["xi"], snap["ti"])
    for t in range(cfg.S):
        L.set_state(t, snap["h"][t], snap["c"][t])
    apply_setting(L, "stride", int(snap["set_stride"][0]), lh)
    apply_setting(L, "carry", int(snap["set_carry"][0]), lh)
    apply_setting(L, "loss_mode", int(snap["set_loss_mode"][0]), lh)
    apply_setting(L, "global_batch", int(snap["set_global_batch"][0]), lh)
    apply_setting(L, "clip", float(snap["set_clip"][0]), lh)
    alpha, tau, eps = (float(v) for v in snap["soft"])
    if "teacher.cfg" in snap:
        tcfg = Config(*ast.literal_eval(bytes(snap["teacher.cfg"]).decode()))
        teacher = restore(tcfg, {k[len("teacher."):]: v for k, v in snap.items() if k.startswith("teacher.")}, lh)
        _set_teacher(L, teacher, alpha=alpha, temperature=tau, smoothing=eps)
    elif (alpha, tau, eps) != (1.0, 1.0, 0.0):
        _set_teacher(L, None, alpha=alpha, temperature=tau, smoothing=eps)
    if kind != lh.AVG_OFF and int(snap["infer_src"][0]) != lh.SRC_PARAMS:
        apply_setting(L, "infer_src", int(snap["infer_src"][0]), lh)   # last: it needs n > 0
    return L


# ---- the ops ------------------------------------------------------------------------------------------------------------
def _window_outputs(L, out, norms=True):
    """What both handles may report after a window: the gradient block, and gates and probabilities of the first, a middle
    and the last step (after train_windows these are the last window's)."""
    out["grads"] = L.get_grads()
    for t in sorted({1, L.S // 2, L.S - 1}):
        out[f"gates{t}"], out[f"probs{t}"] = L.get_activations(t)
    if norms and settings(L)["clip"] > 0.0:
        out["norms"] = L.grad_norms()
    if getattr(L, "_replay_teacher", None) is not None:   # the figures of the last forward (1) or train_windows (count)
        out["teacher_kl"] = L.teacher_kl()
    return out


def train_texts(S, B, ident):
    """The texts of TX(ident): B + 3 of them, 0 to 3 (S - 1) + 1 bytes long, so that within the plan (S - 1 steps per window,
    B lanes) some lanes start a text, some continue one and some idle; the first is the longest (3 windows: every script's
    TX and TXC fit), the next two have no step at all and get no lane, and the other B have a step at least: B + 1 texts
    for B lanes, so the last one starts where the shortest has ended.  An odd ident carries weights, with exact zeros inside
    the texts."""
    rs = _rs(("TX", ident))
    top = 3 * (S - 1) + 1
    lengths = [top, 0, 1] + [int(v) for v in rs.randint(2, top + 1, size=B)]
    texts = [rs.randint(0, 256, size=n).astype(np.uint8).tobytes() for n in lengths]
    if ident % 2 == 0:
        return texts, None
    weights = []
    for n in lengths:
        w = (rs.random_sample(n) * 2.0).astype(np.float32)
        w[rs.random_sample(n) < 0.3] = 0.0
        w[2:4] = 0.0   # context in the middle of a text, not its end
        weights.append(w)
    return texts, weights


def teacher_config(L):
    """The teacher of SOFT(distill): hidden 128 with default flags at the student's S and B; hidden 64 on the per-step engine
    for a student that runs it."""
    step = "STEP_KERNELS" in L._replay_cfg.flags
    return Config(64 if step else 128, L.S, L.B, ("STEP_KERNELS",) if step else (), ())


def start_teacher(L, op):
    """A teacher with a life of its own: seeded parameters, its own text and cursors, a full window, a carry column."""
    rs = _rs(op)
    return start(teacher_config(L), rs.randint(0, 256, size=600).astype(np.uint8), seed=int(rs.randint(1, 1000)))


def _prompts(rs, streams, lo, hi, ascii_only=False):
    top = 128 if ascii_only else 256
    return [rs.randint(0 if not ascii_only else 32, top, size=rs.randint(lo, hi + 1)).astype(np.uint8).tobytes()
            for _ in range(streams)]


def _flatten(prefix, value, out):
    if isinstance(value, dict):
        for k, v in value.items():
            _flatten(f"{prefix}.{k}", v, out)
    elif isinstance(value, (list, tuple)):
        for i, v in enumerate(value):
            _flatten(f"{prefix}[{i}]", v, out)
    elif isinstance(value, (bytes, bytearray)):
        out[prefix] = np.frombuffer(bytes(value), np.uint8)
    elif value is not None:
        out[prefix] = np.asarray(value)


def run_op(L, op, ctx=None, twin=False):
    """Run one op on L; returns {name: array} of its outputs.  ctx: a dict the ops of one script share on the host (the code
    EN made, for DE).  twin: L is the fresh twin (only AD differs: the long-lived handle encodes, the twin decodes)."""
    lh = _lib()
    ctx = {} if ctx is None else ctx
    name, args = op[0], op[1:]
    N, S, B = L.N, L.S, L.B
    text = L._replay_text
    out = {}
    if name == "T":
        out["losses"] = L.train_windows(int(args[0]), LR)
        _window_outputs(L, out)
    elif name == "W":  # path C of tests/test_window_tail.py, the cursors kept too
        st = settings(L)
        (xi, ti), pos = L.get_window(), L.get_cursors()
        host_slide(xi, ti, pos, text, S, st["stride"])
        L.set_window(xi, ti)
        L.set_cursors(pos)
        L.set_state(0, *L.get_state(st["carry"]))
        L.forward()
        out["loss"] = np.array([L.loss()])
        L.backward()
        L.adagrad(LR)
        _window_outputs(L, out)
    elif name == "FB":
        runs = []
        for _ in range(2):
            L.forward()
            r = {"loss": np.array([L.loss()])}
            L.backward()
            _window_outputs(L, r, norms=False)   # (no update, so no norms to read)
            runs.append(r)
        assert_same(runs[0], runs[1], f"{op_name(op)}: the second run against the first")
        out = runs[0]
    elif name == "SP":
        P = L.get_params()
        L.set_params(P + (_rs(op).randn(P.size) * 1e-3).astype(np.float32))
    elif name == "SM":
        m = L.get_params(lh.P_MEM)
        L.set_params(np.abs(m) + (np.abs(_rs(op).randn(m.size)) * 1e-4).astype(np.float32), lh.P_MEM)
    elif name == "CUR":
        L.set_cursors((S + _rs(op).randint(0, len(text) - S, size=B)).astype(np.uint64))
    elif name == "RW":
        L.reset_window()
    elif name == "ST":
        apply_setting(L, "stride", int(args[0]))
        apply_setting(L, "carry", int(args[1]))
    elif name == "LM":
        apply_setting(L, "loss_mode", int(args[0]))
    elif name == "GB":
        apply_setting(L, "global_batch", int(args[0]) * B)
    elif name == "CLIP":
        apply_setting(L, "clip", CLIP_ON if args[0] else 0.0)
    elif name == "PROF":
        apply_setting(L, "profiling", bool(args[0]))
    elif name == "OPT":
        apply_setting(L, "optimizer", lh.OPT_ADAM if args[0] == "adam" else lh.OPT_ADAGRAD)
    elif name == "AVG":
        kind = getattr(lh, AVG_KINDS[args[0]])
        apply_setting(L, "averaging", (kind, EMA_DECAY if args[0] == "ema" else 0.0, int(args[1]) if len(args) > 1 else 1))
    elif name == "SRC":
        apply_setting(L, "infer_src", lh.SRC_AVERAGE if args[0] else lh.SRC_PARAMS)
    elif name == "WD":     # a fixed seed and the handle's current mask index
        L.set_weight_drop(float(args[0]), WD_SEED, L.weight_drop()[2])
    elif name == "ACC":
        L.set_grad_accumulation(int(args[0]), bool(args[1]))
    elif name == "SOFT":
        if args[0] == "off":
            _set_teacher(L, None)
        elif args[0] == "smooth":
            _set_teacher(L, None, smoothing=SMOOTHING)
        else:
            assert args[0] == "distill", op
            _set_teacher(L, start_teacher(L, op), **DISTILL)
    elif name in ("TX", "TXC"):
        if name == "TX":   # new texts: the plan starts again and the streams' bits are zero
            apply_setting(L, "texts", train_texts(S, B, int(args[0])))
        out["losses"] = L.train_text_windows(int(args[-1]), LR)
        _window_outputs(L, out)
        if name == "TX":   # (the bits cannot be restored: compared where both handles start from a fresh set only)
            out["bits"] = L.train_texts_bits()
        out["progress"] = np.array(L.train_texts_progress(), np.int64)
    elif name == "TTR":    # the borrowed teacher trains on its own text, between two calls of its student
        teacher = L._replay_teacher
        assert teacher is not None, "TTR without a teacher"
        L.synchronize()
        out["losses"] = teacher.train_windows(int(args[0]), LR)
        _window_outputs(teacher, out)
        teacher.synchronize()
    elif name == "EVT":    # lanes 0: the handle's B; another number remakes the cached handle
        rs = _rs(op)
        texts = [rs.randint(0, 256, size=n).astype(np.uint8).tobytes() for n in (140, 0, 1, 2, 37)]
        res = L.eval_texts(texts, h0=(rs.randn(5, N) * 0.1).astype(np.float32), c0=(rs.randn(5, N) * 0.1).astype(np.float32),
                           lanes=int(args[0]), surprisal=True)
        _flatten("evt", {k: res[k] for k in ("bits", "h", "c", "surprisal")}, out)
    elif name == "G":
        streams, rs = int(args[0]), _rs(op)
        res = L.generate(_prompts(rs, streams, 0, 20), count=8, u=rs.random_sample((8, streams)), score=True)
        _flatten("g", res, out)
    elif name == "GX":
        rs = _rs(op)
        res = L.generate(_prompts(rs, 5, 0, 20), count=12, u=rs.random_sample((12, 5)), score=True, top_k=40, top_p=0.9,
                         stop_byte=32, info=True)
        _flatten("gx", res, out)
    elif name == "GC":
        rs = _rs(op)
        res = L.generate(_prompts(rs, 7, 0, 20, ascii_only=True), count=10, u=rs.random_sample((10, 7)), score=True,
                         info=True, constraint=lh.dfa_utf8())
        _flatten("gc", res, out)
    elif name == "SC":
        res = L.score(_prompts(_rs(op), 6, 1, 20), first=True, top_n=3)
        _flatten("sc", res, out)
    elif name == "BS":
        res = L.beam_search(_prompts(_rs(op), 3, 0, 20), count=6, beams=4, stop_byte=32, trace=True)
        _flatten("bs", res[1], out)
    elif name == "BSC":
        table = lh.dfa_utf8()
        accept = np.zeros(table.shape[0], np.uint8)
        accept[0] = 1   # a hypothesis ends on a character boundary
        res = L.beam_search(_prompts(_rs(op), 4, 0, 20, ascii_only=True), count=6, beams=3, trace=True, constraint=table,
                            accept=accept)
        _flatten("bsc", res[1], out)
    elif name in ("EN", "DE"):
        texts = _prompts(_rs(("EN",) + tuple(args)), 5, 0, 20)
        if name == "EN":
            codes, bits, trace = L.encode(texts, trace=True)
            ctx["code"] = (tuple(args), codes)
            _flatten("en", dict(codes=codes, bits=bits, trace=trace), out)
        else:
            assert ctx.get("code", (None,))[0] == tuple(args), "DE without the EN whose code it decodes"
            back = L.decode(ctx["code"][1], [len(t) for t in texts])
            assert back == texts, f"{op_name(op)}: the decoded texts are not the encoded ones"
            _flatten("de", back, out)
    elif name == "EV":
        out["bits"] = np.array([L.eval_bits(_rs(op).randint(0, 256, size=300).astype(np.uint8))])
    elif name == "SA":
        rs = _rs(op)
        res = L.sample((rs.randn(N) * 0.1).astype(np.float32), (rs.randn(N) * 0.1).astype(np.float32), rs.random_sample(10))
        _flatten("sa", res, out)
    elif name == "AD":  # 2 trained blocks and a tail; the long-lived handle encodes, its twin decodes that code
        rs = _rs(op)
        texts = [rs.randint(0, 256, size=2 * (S - 1) + rs.randint(0, 4)).astype(np.uint8).tobytes() for _ in range(B)]
        if not twin:
            codes, bits, block_bits = L.encode_adaptive(texts, LR)
            ctx["adaptive"] = (op, codes)
            _flatten("ad", dict(codes=codes, bits=bits, block_bits=block_bits), out)
            _flatten("ad.text", texts, out)
        else:
            assert ctx.get("adaptive", (None,))[0] == op, "the twin decodes what the long-lived handle has just encoded"
            _flatten("ad.text", L.decode_adaptive(ctx["adaptive"][1], [len(t) for t in texts], LR), out)
    elif name == "BAD":
        calls = {"stride": lambda: L.set_stride(0, 0), "clip": lambda: L.set_grad_clip(-1.0),
                 "loss_mode": lambda: L.set_loss_mode(7), "score_top_n": lambda: L.score([b"ab"], top_n=9),
                 "cursor": lambda: L.set_cursors(np.full(B, len(text), np.uint64)),
                 "acc_adaptive": lambda: L.encode_adaptive([b"abcdefgh"] * B, LR),
                 "src_average_n0": lambda: L.set_inference_source(lh.SRC_AVERAGE),
                 "text_windows_soft": lambda: _text_windows_under_soft_targets(L),
                 "acc_pending": lambda: L.set_grad_accumulator(np.zeros(L.np, np.float32), L.grad_accumulation()[0])}
        status = getattr(lh, BAD_CALLS[args[0]])
        try:
            calls[args[0]]()
        except lh.LstmHipError as e:
            assert f"error {status}:" in str(e), f"{op_name(op)}: refused, but not with LSTM_HIP_{BAD_CALLS[args[0]]}: {e}"
            assert BAD_WORDS.get(args[0], "") in str(e), f"{op_name(op)}: refused, but for another reason: {e}"
            out["refused"] = np.array([status])
        else:
            raise AssertionError(f"{op_name(op)}: the call was not refused")
    else:
        raise KeyError(name)
    L.synchronize()   # nothing of this handle is in flight when the caller turns to another one
    return out


def _text_windows_under_soft_targets(L):
    """The refusal is behind the one for a handle without texts: give it one, and take it away again on every path."""
    assert L.soft_targets()[1:] != (1.0, 1.0, 0.0), "BAD(text_windows_soft) with soft targets off"
    L.set_train_texts([b"a text of its own"])
    try:
        L.train_text_windows(1, LR)
    finally:
        L.set_train_texts(None)


def first_difference(a, b):
    """None, or (key, text) for the first array of a and b (keys both have) that is not the same bytes."""
    common = [k for k in a if k in b]
    assert common or not (a or b), (sorted(a), sorted(b))   # (a state edit has no outputs)
    for k in common:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype:
            return k, f"shape / type {x.shape} {x.dtype} against {y.shape} {y.dtype}"
        if x.tobytes() != y.tobytes():
            xf, yf = x.ravel(), y.ravel()
            differ = np.flatnonzero((np.frombuffer(x.tobytes(), np.uint8).reshape(xf.size, x.itemsize) !=
                                     np.frombuffer(y.tobytes(), np.uint8).reshape(yf.size, y.itemsize)).any(axis=1))
            i = int(differ[0])
            return k, f"{differ.size} of {xf.size} elements differ, the first at flat index {i}: {xf[i]!r} against {yf[i]!r}"
    return None


def assert_same(a, b, where):
    """Bitwise equality of every array both dicts hold; `where` names the script, the op index and the op."""
    d = first_difference(a, b)
    assert d is None, f"{where}: '{d[0]}' differs ({d[1]})"
