"""Helpers of tests/test_handle_sequences.py (-m gpu) and of its device-free control, tests/test_handle_sequences_cpu.py.

The contract under test: a fresh handle with the same config
and flags, loaded with a long-lived handle's observable state, behaves bit for bit like that handle -- whatever the long-lived
handle did before -- for every call and for the state the call leaves.  Observable state is what snapshot() reads through the
public wrapper: parameters, optimizer blocks, step count, optimizer kind and numbers; all S columns of h and c; the window's
indices, the text and the cursors; stride and carry column, loss mode, global batch and the clip setting.  Profiling is not
part of it: a twin never profiles, so a profiled window of the long-lived handle (separate loss, fold and slide launches) is
also compared with the carried forms of the same window.

An op is a tuple (name, args...), see run_op.  Everything is seeded from the op itself, so a script (a list of ops,
tests/handle_sequence_cases.py) reproduces.  Nothing here needs a device to import; `lstm_hip` is passed in or imported late.
"""
import contextlib
import os
import zlib

import numpy as np

LR = 0.01
ADAM = dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)
CLIP_ON = 0.05     # below the gradient norm of these windows (about 0.1 to 3), so the coefficient is applied
DEFAULT_SETTINGS = dict(stride=1, carry=1, loss_mode=0, global_batch=None, clip=0.0, optimizer=0, profiling=False)
# settings a twin receives (profiling is the long-lived handle's own business, see above)
OBSERVABLE_SETTINGS = ("stride", "carry", "loss_mode", "global_batch", "clip", "optimizer")

TRAINING = ("T", "W", "FB")
STATE_EDITS = ("SP", "SM", "CUR", "RW", "ST", "LM", "GB", "CLIP", "PROF", "OPT")
INFERENCE = ("G", "GX", "GC", "SC", "BS", "BSC", "EN", "DE", "EV", "SA")
OPS = TRAINING + STATE_EDITS + INFERENCE + ("AD", "BAD")
BAD_CALLS = ("stride", "clip", "loss_mode", "score_top_n", "cursor")


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
        return lh.Lstm(cfg.N, cfg.S, cfg.B, flags=flags)


def apply_setting(L, key, value, lstm_hip=None):
    lh = lstm_hip or _lib()
    st = settings(L)
    if key in ("stride", "carry"):
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


def snapshot(L, text):
    """Everything of the contract's observable state, read through the public wrapper."""
    lh = _lib()
    st = dict(settings(L))
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
    return snap


def restore(cfg, snap, lstm_hip=None):
    """A fresh handle loaded with a snapshot: the optimizer first (a new kind zeroes its state), then the blocks, then the
    step count; text, cursors, window, states; the settings."""
    lh = lstm_hip or _lib()
    L = create(cfg, lh)
    apply_setting(L, "optimizer", int(snap["set_optimizer"][0]), lh)
    L.set_params(snap["params"], lh.P_PARAMS)
    L.set_params(snap["mem"], lh.P_MEM)
    if "adam_v" in snap:
        L.set_params(snap["adam_v"], lh.P_ADAM_V)
    L.set_optimizer_steps(int(snap["steps"][0]))
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
    return out


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
                 "cursor": lambda: L.set_cursors(np.full(B, len(text), np.uint64))}
        try:
            calls[args[0]]()
        except lh.LstmHipError as e:
            assert f"error {lh.EINVAL}:" in str(e), f"{op_name(op)}: refused, but not with LSTM_HIP_EINVAL: {e}"
            out["refused"] = np.array([lh.EINVAL])
        else:
            raise AssertionError(f"{op_name(op)}: the call was not refused")
    else:
        raise KeyError(name)
    return out


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
