"""Host-side mirror of the reference's device seam over the C ABI (include/lstm_hip.h).

The reference's driver (OV/lstm_eigen_class_CUDA/lstm.cc:99-114,156-163,273-377) owns
`cuParameters p, d, m` and a `cuLSTM<S>` and calls forward / calculate_loss / backward / cuda_adagrad
plus the copy helpers.  `Lstm` below is that set of objects behind one handle, same names and
argument meaning; arrays are numpy, column-major as Eigen's (an `N x B` matrix is passed as a
`[B, N]` C-order array, i.e. the same bytes).

There is no CPU fallback: if eigen-lstm_amd/liblstm_hip.so is missing or no gfx950 device is
visible, construction raises.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LSTM_HIP_LIB", os.path.join(HERE, "liblstm_hip.so"))  # env override: A/B builds only

FAST_MATH = 1
STEP_KERNELS = 4
DEBUG_STAMPS = 16
NO_FUSED_GRADS = 64
BF16_RECURRENCE = 128
PAD_HIDDEN = 256  # any hidden size >= 1, run at an internal padded width (include/lstm_hip.h); shapes stay logical
STABLE_SOFTMAX = 512  # max-shifted output layer with log-sum-exp surprisal, for logits past expf's range (include/lstm_hip.h)
LOSS_ALL_STEPS_BITS, LOSS_LAST_STEP_NATS, LOSS_LAST_STEP_BITS = 0, 1, 2
OK, EINVAL, EHIP, ENODEV, ERCCL, ESTATE = 0, -1, -2, -3, -4, -5  # LSTM_HIP_OK, LSTM_HIP_E* return codes
UNIQUE_ID_BYTES = 128
VOCAB = 256

P_PARAMS, P_GRADS, P_MEM = 0, 1, 2
P_ADAM_V = 3  # Adam's second moment (P_MEM is its first moment on an Adam handle)
OPT_ADAGRAD, OPT_ADAM = 0, 1  # update rules of lstm_hip_set_optimizer (include/lstm_hip.h)
AVG_OFF, AVG_EMA, AVG_UNIFORM = 0, 1, 2  # kinds of lstm_hip_set_averaging
SRC_PARAMS, SRC_AVERAGE = 0, 1  # what the inference calls read (lstm_hip_set_inference_source)


class LstmHipError(RuntimeError):
    pass


class _Sampling(C.Structure):  # lstm_hip_sampling
    _fields_ = [("size", C.c_uint32), ("temperature", C.c_double), ("top_k", C.c_int32), ("top_p", C.c_double),
                ("stop_byte", C.c_int32)]


class _Constraint(C.Structure):  # lstm_hip_constraint
    _fields_ = [("size", C.c_uint32), ("states", C.c_int32), ("next", C.POINTER(C.c_uint16))]


class _Beam(C.Structure):  # lstm_hip_beam
    _fields_ = [("size", C.c_uint32), ("beams", C.c_int32), ("stop_byte", C.c_int32)]


class _BeamConstraint(C.Structure):  # lstm_hip_beam_constraint
    _fields_ = [("size", C.c_uint32), ("con", C.POINTER(_Constraint)), ("accept", C.POINTER(C.c_uint8))]


class _LogitProcessors(C.Structure):  # lstm_hip_logit_processors
    _fields_ = [("size", C.c_uint32), ("bias", C.POINTER(C.c_float)), ("min_p", C.c_double), ("no_repeat", C.c_int32),
                ("history", C.POINTER(C.c_uint8)), ("history_off", C.POINTER(C.c_uint64))]


class _Guide(C.Structure):  # lstm_hip_guide
    _fields_ = [("model", C.c_void_p), ("weight", C.c_double), ("h0", C.POINTER(C.c_float)), ("c0", C.POINTER(C.c_float)),
                ("h_out", C.POINTER(C.c_float)), ("c_out", C.POINTER(C.c_float))]


class _Guidance(C.Structure):  # lstm_hip_guidance
    _fields_ = [("size", C.c_uint32), ("main_weight", C.c_double), ("nguides", C.c_int32), ("guides", C.POINTER(_Guide))]


class _MixCoding(C.Structure):  # lstm_hip_mix_coding
    _fields_ = [("size", C.c_uint32), ("rate", C.c_double)]


class _Scoring(C.Structure):  # lstm_hip_scoring
    _fields_ = [("size", C.c_uint32), ("first", C.c_int32), ("top_n", C.c_int32), ("con", C.POINTER(_Constraint))]


class _Scores(C.Structure):  # lstm_hip_scores
    _fields_ = [("size", C.c_uint32), ("surprisal", C.POINTER(C.c_float)), ("entropy", C.POINTER(C.c_float)),
                ("rank", C.POINTER(C.c_uint8)), ("top_byte", C.POINTER(C.c_uint8)), ("top_bits", C.POINTER(C.c_float)),
                ("bits", C.POINTER(C.c_double)), ("end_state", C.POINTER(C.c_int32))]


class _EvalOpt(C.Structure):  # lstm_hip_eval_opt
    _fields_ = [("size", C.c_uint32), ("lanes", C.c_int32)]


class _Embedding(C.Structure):  # lstm_hip_embedding
    _fields_ = [("size", C.c_uint32), ("mean_h", C.POINTER(C.c_float)), ("max_h", C.POINTER(C.c_float)),
                ("last_h", C.POINTER(C.c_float)), ("mean_c", C.POINTER(C.c_float)), ("max_c", C.POINTER(C.c_float)),
                ("last_c", C.POINTER(C.c_float)), ("count", C.POINTER(C.c_int64)), ("bits", C.POINTER(C.c_double)),
                ("picked_h", C.POINTER(C.c_float)), ("picked_c", C.POINTER(C.c_float))]


class _SoftTargets(C.Structure):  # lstm_hip_soft_targets
    _fields_ = [("size", C.c_uint32), ("alpha", C.c_double), ("temperature", C.c_double), ("smoothing", C.c_double)]


class _Config(C.Structure):
    _fields_ = [("N", C.c_int32), ("M", C.c_int32), ("S", C.c_int32), ("B", C.c_int32), ("device", C.c_int32),
                ("flags", C.c_uint32)]


_lib = None

# every symbol include/lstm_hip.h declares (tests check the library exports all of them)
SYMBOLS = [
    "lstm_hip_create", "lstm_hip_destroy", "lstm_hip_last_error", "lstm_hip_param_count", "lstm_hip_set_params",
    "lstm_hip_get_params", "lstm_hip_set_state", "lstm_hip_get_state", "lstm_hip_get_activations",
    "lstm_hip_set_window", "lstm_hip_set_inputs_dense", "lstm_hip_slide_state", "lstm_hip_forward", "lstm_hip_loss", "lstm_hip_backward",
    "lstm_hip_adagrad", "lstm_hip_comm_unique_id", "lstm_hip_comm_init", "lstm_hip_allreduce_grads",
    "lstm_hip_set_text", "lstm_hip_set_cursors", "lstm_hip_get_cursors", "lstm_hip_reset_window",
    "lstm_hip_get_window", "lstm_hip_train_windows", "lstm_hip_set_global_batch", "lstm_hip_set_loss_mode", "lstm_hip_set_stride", "lstm_hip_eval_bits",
    "lstm_hip_sample", "lstm_hip_generate", "lstm_hip_generate_ex", "lstm_hip_synchronize", "lstm_hip_set_profiling", "lstm_hip_kernel_stat_count",
    "lstm_hip_kernel_stat", "lstm_hip_reset_kernel_stats", "lstm_hip_device_info", "lstm_hip_debug_stamps",
    "lstm_hip_set_grad_clip", "lstm_hip_get_grad_norms", "lstm_hip_set_optimizer", "lstm_hip_get_optimizer_steps",
    "lstm_hip_set_optimizer_steps", "lstm_hip_coder_version", "lstm_hip_code_bound", "lstm_hip_encode", "lstm_hip_decode",
    "lstm_hip_adaptive_version", "lstm_hip_adaptive_blocks", "lstm_hip_encode_adaptive", "lstm_hip_decode_adaptive",
    "lstm_hip_plan_identity", "lstm_hip_beam_search", "lstm_hip_generate_constrained", "lstm_hip_dfa_utf8",
    "lstm_hip_dfa_restrict", "lstm_hip_score", "lstm_hip_beam_search_constrained",
    "lstm_hip_set_averaging", "lstm_hip_get_average", "lstm_hip_set_average", "lstm_hip_get_averaging_counts",
    "lstm_hip_set_averaging_counts", "lstm_hip_set_inference_source",
    "lstm_hip_set_weight_drop", "lstm_hip_get_weight_drop", "lstm_hip_weight_drop_mask",
    "lstm_hip_dfa_regex", "lstm_hip_dfa_intersect", "lstm_hip_generate_accepting",
    "lstm_hip_eval_plan", "lstm_hip_eval_texts",
    "lstm_hip_text_plan", "lstm_hip_set_train_texts", "lstm_hip_get_train_texts", "lstm_hip_train_text_windows",
    "lstm_hip_get_train_texts_bits", "lstm_hip_set_train_texts_weighted",
    "lstm_hip_set_soft_targets", "lstm_hip_get_soft_targets", "lstm_hip_get_teacher_kl",
    "lstm_hip_set_grad_accumulation", "lstm_hip_get_grad_accumulation", "lstm_hip_get_grad_accumulator",
    "lstm_hip_set_grad_accumulator",
    "lstm_hip_generate_processed",
    "lstm_hip_embed_texts",
    "lstm_hip_generate_guided", "lstm_hip_score_guided",
    "lstm_hip_mix_coder_version", "lstm_hip_encode_mixed", "lstm_hip_decode_mixed",
]


def load_library():
    """dlopen the in-tree C-ABI library; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LstmHipError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback for the HIP path)")
    lib = C.CDLL(LIB_PATH)
    lib.lstm_hip_last_error.restype = C.c_char_p
    lib.lstm_hip_param_count.restype = C.c_size_t
    lib.lstm_hip_param_count.argtypes = [C.c_int32, C.c_int32]
    lib.lstm_hip_coder_version.restype = C.c_uint32
    lib.lstm_hip_coder_version.argtypes = []
    lib.lstm_hip_code_bound.restype = C.c_size_t
    lib.lstm_hip_code_bound.argtypes = [C.c_uint64]
    lib.lstm_hip_adaptive_version.restype = C.c_uint32
    lib.lstm_hip_adaptive_version.argtypes = []
    lib.lstm_hip_adaptive_blocks.restype = C.c_int64
    lib.lstm_hip_adaptive_blocks.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_uint64)]
    if hasattr(lib, "lstm_hip_eval_plan"):  # (an older library named by LSTM_HIP_LIB lacks it)
        lib.lstm_hip_eval_plan.restype = C.c_int64
        lib.lstm_hip_eval_plan.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_int32),
                                           C.POINTER(C.c_int64)]
    if hasattr(lib, "lstm_hip_text_plan"):
        lib.lstm_hip_text_plan.restype = C.c_int64
        lib.lstm_hip_text_plan.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_int32),
                                           C.POINTER(C.c_int64)]
    if hasattr(lib, "lstm_hip_mix_coder_version"):
        lib.lstm_hip_mix_coder_version.restype = C.c_uint32
        lib.lstm_hip_mix_coder_version.argtypes = []
    _lib = lib
    return lib


def param_count(N, M=VOCAB):
    return load_library().lstm_hip_param_count(N, M)


def coder_version():
    """lstm_hip_coder_version: changes whenever the arithmetic that feeds the range coder changes (a code decodes only with
    the same version, parameters and LSTM_HIP_FAST_MATH setting)."""
    return int(load_library().lstm_hip_coder_version())


def code_bound(n):
    """lstm_hip_code_bound: the largest code a stream of n bytes can have (0 for n = 0, else 3n + 4)."""
    return int(load_library().lstm_hip_code_bound(int(n)))


def adaptive_version():
    """lstm_hip_adaptive_version: changes whenever the adaptive schedule or anything it calls changes a code."""
    return int(load_library().lstm_hip_adaptive_version())


def adaptive_blocks(S, B, text_off):
    """lstm_hip_adaptive_blocks: floor(shortest stream / (S - 1)), the number of trained blocks; needs no device."""
    off = np.ascontiguousarray(text_off, dtype=np.uint64)
    assert off.size == B + 1, (off.size, B)
    n = int(load_library().lstm_hip_adaptive_blocks(S, B, _ptr(off, C.c_uint64)))
    if n < 0:
        _chk(n)
    return n


EVAL_STEPS = 128  # LSTM_HIP_EVAL_STEPS


def eval_plan(lanes, lengths):
    """lstm_hip_eval_plan: the schedule lstm_hip_eval_texts runs for streams of these byte lengths on `lanes` lanes; needs
    no device.  Returns (windows, lane_of int32 [streams], first_window int64 [streams]); a stream of fewer than 2 bytes has
    no step and gets -1, -1."""
    lengths = [int(v) for v in lengths]
    off = np.zeros(len(lengths) + 1, np.uint64)
    off[1:] = np.cumsum(lengths, dtype=np.uint64)
    lane_of, first = np.zeros(max(len(lengths), 1), np.int32), np.zeros(max(len(lengths), 1), np.int64)
    n = int(load_library().lstm_hip_eval_plan(int(lanes), len(lengths), _ptr(off, C.c_uint64), _ptr(lane_of, C.c_int32),
                                              _ptr(first, C.c_int64)))
    if n < 0:
        _chk(n)
    return n, lane_of[:len(lengths)], first[:len(lengths)]


def text_plan(steps, lanes, lengths):
    """lstm_hip_text_plan: eval_plan's rule with `steps` rows per window, the schedule Lstm.train_text_windows runs with
    steps = S - 1 and lanes = B; needs no device.  Returns (windows, lane_of int32 [streams], first_window int64 [streams])."""
    lengths = [int(v) for v in lengths]
    off = np.zeros(len(lengths) + 1, np.uint64)
    off[1:] = np.cumsum(lengths, dtype=np.uint64)
    lane_of, first = np.zeros(max(len(lengths), 1), np.int32), np.zeros(max(len(lengths), 1), np.int64)
    n = int(load_library().lstm_hip_text_plan(int(steps), int(lanes), len(lengths), _ptr(off, C.c_uint64),
                                              _ptr(lane_of, C.c_int32), _ptr(first, C.c_int64)))
    if n < 0:
        _chk(n)
    return n, lane_of[:len(lengths)], first[:len(lengths)]


def eval_split_pieces(length, pieces, warm=0):
    """The cut Lstm.eval_split makes of a text of `length` bytes: a list of (start, stop, skip).  Piece i scores the bytes
    a_i .. a_{i+1} - 1 with a_i = 1 + floor(i (length - 1) / pieces); its stream is text[max(0, a_i - 1 - warm) : a_{i+1}]
    and skip = a_i - start, so the bytes before a_i are fed as warm-up and every byte 1 .. length - 1 is scored once."""
    length, pieces, warm = int(length), int(pieces), int(warm)
    if length < 2 or pieces < 1 or warm < 0:
        raise LstmHipError(f"eval_split: need >= 2 bytes, >= 1 piece, warm >= 0 (got {length}, {pieces}, {warm})")
    a = [1 + i * (length - 1) // pieces for i in range(pieces + 1)]
    return [(max(0, a[i] - 1 - warm), a[i + 1], a[i] - max(0, a[i] - 1 - warm)) for i in range(pieces)]


def completion_weights(texts, sep):
    """The weights of completion-only training for Lstm.set_train_texts(texts, weights=...): per text a float32 array of its
    length, 1.0 for every byte after the first `sep` byte (a byte value 0..255), 0.0 for the rest -- the prompt and the
    separator itself are context, the completion is learned.  A text without `sep` is all zeros.  Needs no device."""
    sep = int(sep)
    if not 0 <= sep <= 255:
        raise LstmHipError(f"completion_weights: sep must be a byte value 0..255 (got {sep})")
    out = []
    for t in _bytes_list(texts):
        w = np.zeros(t.size, np.float32)
        at = np.flatnonzero(t == sep)
        if at.size:
            w[at[0] + 1:] = 1.0
        out.append(w)
    return out


def weight_drop_mask(N, rate, seed=0, t=0):
    """lstm_hip_weight_drop_mask: the keep mask of lstm_hip_set_weight_drop for a logical hidden size N, as a bool array
    [4N, N] (True where element (r, k) of U is kept).  The shipped rule running on the CPU: needs no device."""
    keep = np.empty(4 * N * N, np.uint8)
    _chk(load_library().lstm_hip_weight_drop_mask(C.c_int32(N), C.c_double(rate), C.c_uint64(seed), C.c_uint64(t),
                                                  _ptr(keep, C.c_uint8)))
    return keep.reshape(N, 4 * N).T != 0  # (keep[r + 4N * k]: column-major)


def dfa_utf8():
    """lstm_hip_dfa_utf8: the automaton of well-formed UTF-8 as an (8, 256) uint16 table for Lstm.generate(constraint=...).
    Entry [q, b] is the state after byte b in state q, 0xFFFF where b is forbidden; state 0 is the start state and the
    only character boundary.  Needs no device."""
    lib = load_library()
    lib.lstm_hip_dfa_utf8.restype = C.c_int32
    table = np.zeros((int(lib.lstm_hip_dfa_utf8(None)), 256), np.uint16)
    lib.lstm_hip_dfa_utf8(_ptr(table, C.c_uint16))
    return table


def dfa_restrict(table, allow):
    """lstm_hip_dfa_restrict: a copy of `table` ((states, 256) uint16) that forbids every byte b with allow[b] == 0 (allow:
    256 flags) and, repeatedly, every transition into a state left with no allowed byte.  State numbers do not change.
    Raises LstmHipError when state 0 ends up empty.  Needs no device."""
    table = np.array(table, dtype=np.uint16, order="C")
    assert table.ndim == 2 and table.shape[1] == 256, table.shape
    flags = np.ascontiguousarray(np.asarray(allow).reshape(256) != 0, dtype=np.uint8)
    _chk(load_library().lstm_hip_dfa_restrict(_ptr(table, C.c_uint16), C.c_int32(table.shape[0]), _ptr(flags, C.c_uint8)))
    return table


def dfa_regex(pattern, stop_byte=-1):
    """lstm_hip_dfa_regex: a byte regular expression (bytes, or str taken as UTF-8) compiled to (table, accept): the minimal
    automaton of the language as a (states, 256) uint16 table and its accepting states as uint8 flags [states].  A match is
    a whole-string match, with the meaning re.fullmatch gives a bytes pattern, for the subset include/lstm_hip.h lists; a
    quantifier binds the last BYTE, so group a multi-byte character before repeating it.  stop_byte 0..255 gives the table of the language followed by that
    byte, whose one accepting state loops on it: the form Lstm.generate(constraint=, accept=, stop_byte=) and
    Lstm.beam_search take as it is.  Raises LstmHipError with the library's message (it names the pattern byte); the
    exception's error_pos holds that offset, -1 where there is none.  Needs no device."""
    lib = load_library()
    pat = np.frombuffer(pattern.encode("utf-8") if isinstance(pattern, str) else bytes(pattern), np.uint8)
    lib.lstm_hip_dfa_regex.restype = C.c_int32
    lib.lstm_hip_dfa_regex.argtypes = [C.POINTER(C.c_uint8), C.c_size_t, C.c_int32, C.POINTER(C.c_uint16), C.POINTER(C.c_uint8),
                                       C.c_int32, C.POINTER(C.c_int32)]
    data = np.ascontiguousarray(pat if pat.size else np.zeros(1, np.uint8))
    pos = C.c_int32(-1)
    table = accept = None
    for _ in range(2):  # the size, then the table
        q = int(lib.lstm_hip_dfa_regex(_ptr(data, C.c_uint8), pat.size, int(stop_byte),
                                       _ptr(table, C.c_uint16) if table is not None else None,
                                       _ptr(accept, C.c_uint8) if accept is not None else None,
                                       0 if table is None else table.shape[0], C.byref(pos)))
        if q < 0:
            err = LstmHipError(f"lstm_hip error {q}: {lib.lstm_hip_last_error().decode()}")
            err.error_pos = int(pos.value)
            raise err
        if table is None:
            table, accept = np.zeros((q, 256), np.uint16), np.zeros(q, np.uint8)
    return table, accept


def dfa_intersect(a, acc_a, b, acc_b):
    """lstm_hip_dfa_intersect: (table, accept) of the strings both automata accept: tables a, b as (states, 256) uint16,
    acc_a, acc_b their accepting flags [states] or None (every state accepts).  The product is trimmed, minimised and
    numbered as dfa_regex's results are.  Raises LstmHipError when nothing is accepted by both or the result has more than
    4096 states.  Needs no device."""
    lib = load_library()
    lib.lstm_hip_dfa_intersect.restype = C.c_int32
    tabs, accs = [], []
    for t, acc in ((a, acc_a), (b, acc_b)):
        t = np.ascontiguousarray(t, dtype=np.uint16)
        assert t.ndim == 2 and t.shape[1] == 256, t.shape
        tabs.append(t)
        accs.append(None if acc is None else np.ascontiguousarray(np.asarray(acc).reshape(t.shape[0]) != 0, dtype=np.uint8))
    table = accept = None
    for _ in range(2):  # the size, then the table
        q = int(lib.lstm_hip_dfa_intersect(
            _ptr(tabs[0], C.c_uint16), C.c_int32(tabs[0].shape[0]), _ptr(accs[0], C.c_uint8) if accs[0] is not None else None,
            _ptr(tabs[1], C.c_uint16), C.c_int32(tabs[1].shape[0]), _ptr(accs[1], C.c_uint8) if accs[1] is not None else None,
            _ptr(table, C.c_uint16) if table is not None else None, _ptr(accept, C.c_uint8) if accept is not None else None,
            C.c_int32(0 if table is None else table.shape[0])))
        if q < 0:
            _chk(q)
        if table is None:
            table, accept = np.zeros((q, 256), np.uint16), np.zeros(q, np.uint8)
    return table, accept


def _bytes_list(texts):
    return [np.frombuffer(bytes(p), np.uint8) if isinstance(p, (bytes, bytearray)) else np.asarray(p, np.uint8).ravel()
            for p in texts]


def _offsets(parts):
    off = np.zeros(len(parts) + 1, np.uint64)
    off[1:] = np.cumsum([q.size for q in parts])
    data = np.ascontiguousarray(np.concatenate(parts) if off[-1] > 0 else np.zeros(1, np.uint8))
    return data, off


def _chk(rc):
    if rc != 0:
        raise LstmHipError(f"lstm_hip error {rc}: {load_library().lstm_hip_last_error().decode()}")


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a, t=C.c_float):
    return a.ctypes.data_as(C.POINTER(t))


def _guidance(guides, main_weight, streams):
    """the lstm_hip_guidance block of guides = [(model, weight[, h0[, c0]]), ...]: (block, the guides' h_out arrays, their
    c_out arrays, what has to stay alive until the call returns)"""
    items = [tuple(g) + (None,) * (4 - len(tuple(g))) for g in guides]
    arr = (_Guide * max(len(items), 1))()
    gh, gc, alive = [], [], [arr]
    for k, (model, weight, h0, c0) in enumerate(items):
        n = model.N
        hh = None if h0 is None else _f32(h0).reshape(streams, n)
        cc = None if c0 is None else _f32(c0).reshape(streams, n)
        gh.append(np.empty((streams, n), np.float32))
        gc.append(np.empty((streams, n), np.float32))
        alive += [hh, cc]
        arr[k] = _Guide(model._h.value, float(weight), _ptr(hh) if hh is not None else None, _ptr(cc) if cc is not None else None,
                        _ptr(gh[k]), _ptr(gc[k]))
    return _Guidance(C.sizeof(_Guidance), float(main_weight), len(items), arr), gh, gc, alive


def _coder_guidance(guides, main_weight):
    """the lstm_hip_guidance block of the mixed coders, guides = [(model, weight), ...]: no states in or out (every model
    starts from zero).  (block, what has to stay alive until the call returns)"""
    items = [tuple(g) for g in guides]
    arr = (_Guide * max(len(items), 1))()
    for k, (model, weight) in enumerate(items):
        arr[k] = _Guide(model._h.value, float(weight), None, None, None, None)
    return _Guidance(C.sizeof(_Guidance), float(main_weight), len(items), arr), arr


def mix_coder_version():
    return int(load_library().lstm_hip_mix_coder_version())


def device_info(device=0):
    lib = load_library()
    name = C.create_string_buffer(64)
    cus, mhz = C.c_int32(), C.c_int32()
    _chk(lib.lstm_hip_device_info(device, name, C.byref(cus), C.byref(mhz)))
    return name.value.decode(), cus.value, mhz.value


def comm_unique_id():
    buf = (C.c_uint8 * UNIQUE_ID_BYTES)()
    _chk(load_library().lstm_hip_comm_unique_id(buf))
    return bytes(buf)


class Lstm:
    """cuParameters p,d,m + cuLSTM<S> (OV/lstm_eigen_class_CUDA/cu_lstm.h) behind one handle."""

    def __init__(self, N, S, B, device=0, flags=0, M=VOCAB):
        self.lib = load_library()
        self.N, self.M, self.S, self.B = N, M, S, B
        self.np = param_count(N, M)
        self._h = C.c_void_p()
        cfg = _Config(N, M, S, B, device, flags)
        _chk(self.lib.lstm_hip_create(C.byref(cfg), C.byref(self._h)))

    def close(self):
        if self._h:
            _chk(self.lib.lstm_hip_destroy(self._h))  # (refused while a student holds this handle as its teacher)
            self._h = C.c_void_p()
            self._teacher = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- copy_parameters_to_device / _to_host -------------------------------------------------
    def set_params(self, block, which=P_PARAMS):
        block = _f32(block)
        assert block.size == self.np, (block.size, self.np)
        _chk(self.lib.lstm_hip_set_params(self._h, which, _ptr(block)))

    def get_params(self, which=P_PARAMS):
        out = np.empty(self.np, np.float32)
        _chk(self.lib.lstm_hip_get_params(self._h, which, _ptr(out)))
        return out

    def get_grads(self):
        return self.get_params(P_GRADS)

    # ---- copy_lstm_to_device / copy_context_to_host -------------------------------------------
    def set_state(self, t, h=None, c=None):
        h = None if h is None else _f32(h)
        c = None if c is None else _f32(c)
        for a in (h, c):
            assert a is None or a.size == self.N * self.B
        _chk(self.lib.lstm_hip_set_state(self._h, t, _ptr(h) if h is not None else None,
                                         _ptr(c) if c is not None else None))

    def get_state(self, t):
        h = np.empty((self.B, self.N), np.float32)
        c = np.empty((self.B, self.N), np.float32)
        _chk(self.lib.lstm_hip_get_state(self._h, t, _ptr(h), _ptr(c)))
        return h, c

    def get_activations(self, t):
        g = np.empty((self.B, 4 * self.N), np.float32)
        p = np.empty((self.B, self.M), np.float32)
        _chk(self.lib.lstm_hip_get_activations(self._h, t, _ptr(g), _ptr(p)))
        return g, p

    # ---- copy_inputs_to_device ----------------------------------------------------------------
    def set_window(self, xi, ti):
        xi = np.ascontiguousarray(xi, dtype=np.int32)
        ti = np.ascontiguousarray(ti, dtype=np.int32)
        assert xi.shape == (self.S, self.B) and ti.shape == (self.S, self.B)
        _chk(self.lib.lstm_hip_set_window(self._h, _ptr(xi, C.c_int32), _ptr(ti, C.c_int32)))

    def set_inputs_dense(self, x, target, h0=None, c0=None):
        """copy_inputs_to_device with the reference's own operands: dense one-hot x[t], target[t] as [S, B, M] arrays
        (= M x B column-major matrices back to back) and optionally h[0], c[0] as [B, N]."""
        x, target = _f32(x), _f32(target)
        assert x.shape == (self.S, self.B, self.M) and target.shape == (self.S, self.B, self.M)
        h0 = None if h0 is None else _f32(h0)
        c0 = None if c0 is None else _f32(c0)
        _chk(self.lib.lstm_hip_set_inputs_dense(self._h, _ptr(h0) if h0 is not None else None,
                                                _ptr(c0) if c0 is not None else None, _ptr(x), _ptr(target)))

    def get_window(self):
        xi = np.empty((self.S, self.B), np.int32)
        ti = np.empty((self.S, self.B), np.int32)
        _chk(self.lib.lstm_hip_get_window(self._h, _ptr(xi, C.c_int32), _ptr(ti, C.c_int32)))
        return xi, ti

    def slide_state(self):
        _chk(self.lib.lstm_hip_slide_state(self._h))

    # ---- cuLSTM::forward / calculate_loss / backward, cuda_adagrad ------------------------------
    def forward(self):
        _chk(self.lib.lstm_hip_forward(self._h))
        self._kls = 1

    def loss(self):
        out = C.c_double()
        _chk(self.lib.lstm_hip_loss(self._h, C.byref(out)))
        return out.value

    def backward(self):
        _chk(self.lib.lstm_hip_backward(self._h))

    def adagrad(self, lr):
        steps = self._updates_in(1)
        _chk(self.lib.lstm_hip_adagrad(self._h, C.c_double(lr)))
        self._steps = steps

    # ---- global-norm gradient clipping (lstm_hip_set_grad_clip) --------------------------------
    def set_grad_clip(self, max_norm):
        """0: off; > 0: scale the step's gradient by max_norm / (norm + 1e-6) where that is below 1; inf: measure only."""
        _chk(self.lib.lstm_hip_set_grad_clip(self._h, C.c_double(max_norm)))

    def grad_norms(self, n=None):
        """pre-clip norms of the Adagrad steps of the last adagrad (1) / train_windows (count) call, oldest first;
        n=None: all of them."""
        k = getattr(self, "_steps", 0) if n is None else int(n)
        out = np.zeros(k, np.float64)
        _chk(self.lib.lstm_hip_get_grad_norms(self._h, _ptr(out, C.c_double), C.c_int64(k)))
        return out

    # ---- gradient accumulation (lstm_hip_set_grad_accumulation) --------------------------------
    def set_grad_accumulation(self, every, mean=False):
        """every = 1: off (the default).  every = K >= 2: the gradients of K consecutive windows (adagrad calls, windows of
        train_windows and of train_text_windows) are summed in fp32, divided by K with `mean`, and one update is made on the
        sum, at the K-th.  A different (every, mean) discards what is pending; the same pair again keeps it."""
        _chk(self.lib.lstm_hip_set_grad_accumulation(self._h, C.c_int32(every), C.c_int32(int(mean))))

    def grad_accumulation(self):
        """(every, mean, pending): the setting, and how many windows the accumulator holds (0 .. every - 1)."""
        every, mean, pending = C.c_int32(), C.c_int32(), C.c_int32()
        _chk(self.lib.lstm_hip_get_grad_accumulation(self._h, C.byref(every), C.byref(mean), C.byref(pending)))
        return every.value, bool(mean.value), pending.value

    def grad_accumulator(self):
        """the summed gradient of the pending windows (logical-N flat block; zeros while pending is 0)"""
        out = np.empty(self.np, np.float32)
        _chk(self.lib.lstm_hip_get_grad_accumulator(self._h, _ptr(out)))
        return out

    def set_grad_accumulator(self, block, pending):
        """resuming: after set_grad_accumulation, the saved block and its count of windows"""
        block = _f32(block)
        assert block.size == self.np, (block.size, self.np)
        _chk(self.lib.lstm_hip_set_grad_accumulator(self._h, _ptr(block), C.c_int32(pending)))

    def _updates_in(self, count):
        """updates that the next `count` windows make: all of them, or one per full cycle under gradient accumulation"""
        if not hasattr(self.lib, "lstm_hip_get_grad_accumulation"):  # (an older library named by LSTM_HIP_LIB lacks it)
            return count
        every, _, pending = self.grad_accumulation()
        return (pending + count) // every

    # ---- the update rule (lstm_hip_set_optimizer) ----------------------------------------------
    def set_optimizer(self, kind, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0):
        """OPT_ADAGRAD (the default rule) or OPT_ADAM (AdamW; weight_decay 0: plain Adam).  A new kind zeroes the
        optimizer state and the step count; the same kind again keeps them."""
        if kind == OPT_ADAGRAD:
            beta1 = beta2 = eps = weight_decay = 0.0
        _chk(self.lib.lstm_hip_set_optimizer(self._h, C.c_int32(kind), C.c_double(beta1), C.c_double(beta2), C.c_double(eps),
                                             C.c_double(weight_decay)))

    def optimizer_steps(self):
        out = C.c_int64()
        _chk(self.lib.lstm_hip_get_optimizer_steps(self._h, C.byref(out)))
        return out.value

    def set_optimizer_steps(self, t):
        _chk(self.lib.lstm_hip_set_optimizer_steps(self._h, C.c_int64(t)))

    # ---- the running weight average and inference from it (lstm_hip_set_averaging) ---------------
    def set_averaging(self, kind, decay=0.0, every=1):
        """AVG_OFF, AVG_EMA (0 <= decay < 1) or AVG_UNIFORM (decay 0): after every `every`-th update the average takes the
        new parameters, a = p at its first update and a + w * (p - a) after it (w = 1 - decay, or 1 / n).  A new kind
        zeroes the average and its counters; the same kind again keeps them."""
        _chk(self.lib.lstm_hip_set_averaging(self._h, C.c_int32(kind), C.c_double(decay), C.c_int32(every)))

    def get_average(self):
        out = np.empty(self.np, np.float32)
        _chk(self.lib.lstm_hip_get_average(self._h, _ptr(out)))
        return out

    def set_average(self, block):
        block = _f32(block)
        assert block.size == self.np, (block.size, self.np)
        _chk(self.lib.lstm_hip_set_average(self._h, _ptr(block)))

    def averaging_counts(self):
        """(seen, n): updates launched with averaging on, and how many of them the average has taken."""
        seen, n = C.c_int64(), C.c_int64()
        _chk(self.lib.lstm_hip_get_averaging_counts(self._h, C.byref(seen), C.byref(n)))
        return seen.value, n.value

    def set_averaging_counts(self, seen, n):
        _chk(self.lib.lstm_hip_set_averaging_counts(self._h, C.c_int64(seen), C.c_int64(n)))

    def set_inference_source(self, source):
        """SRC_PARAMS (the default) or SRC_AVERAGE: what eval_bits, sample, generate, beam_search, score, encode and decode
        read.  Training never reads it; the adaptive coders refuse SRC_AVERAGE."""
        _chk(self.lib.lstm_hip_set_inference_source(self._h, C.c_int32(source)))

    # ---- weight drop: DropConnect on U, one mask per training window (lstm_hip_set_weight_drop) ----
    def set_weight_drop(self, rate, seed=0, t=0):
        """rate 0: off (the default); 0 < rate < 1: every training window reads U masked by the Philox mask of (seed, t) and
        rescaled by 1 / (1 - rate), and dU gets the same mask and scale.  t advances with every update.  Everything that is
        not a training window reads the unmasked parameters.  Drops the forward pass."""
        _chk(self.lib.lstm_hip_set_weight_drop(self._h, C.c_double(rate), C.c_uint64(seed), C.c_uint64(t)))

    def weight_drop(self):
        """(rate, seed, t) of lstm_hip_get_weight_drop."""
        rate, seed, t = C.c_double(), C.c_uint64(), C.c_uint64()
        _chk(self.lib.lstm_hip_get_weight_drop(self._h, C.byref(rate), C.byref(seed), C.byref(t)))
        return rate.value, seed.value, t.value

    # ---- soft targets: label smoothing and distillation from a teacher (lstm_hip_set_soft_targets) ----
    def set_soft_targets(self, teacher=None, alpha=1.0, temperature=1.0, smoothing=0.0):
        """dy = alpha (p - r) + (1 - alpha) tau (softmax(z / tau) - softmax(z_T / tau)), r the target smoothed by `smoothing`
        and z_T the logits of `teacher`, an Lstm with the same S, B and device that this handle borrows: every forward pass
        here overwrites its window, states and logits.  The defaults turn the feature off.  Reported losses stay the
        hard-target bits.  Drops the forward pass.  The student keeps a reference to the teacher until it is re-set or closed."""
        opt = _SoftTargets(C.sizeof(_SoftTargets), alpha, temperature, smoothing)
        _chk(self.lib.lstm_hip_set_soft_targets(self._h, teacher._h if teacher is not None else None, C.byref(opt)))
        self._teacher = teacher

    def soft_targets(self):
        """(teacher, alpha, temperature, smoothing) of lstm_hip_get_soft_targets; teacher is the Lstm given to
        set_soft_targets, or None."""
        t, opt = C.c_void_p(), _SoftTargets()
        _chk(self.lib.lstm_hip_get_soft_targets(self._h, C.byref(t), C.byref(opt)))
        return (getattr(self, "_teacher", None) if t.value else None), opt.alpha, opt.temperature, opt.smoothing

    def teacher_kl(self, n=None):
        """KL(q || p_tau) in bits per window of the last forward (1) / train_windows (count) call, oldest first, summed over
        the window's steps as the loss is; n=None: all of them.  Needs a teacher."""
        k = getattr(self, "_kls", 0) if n is None else int(n)
        out = np.zeros(k, np.float64)
        _chk(self.lib.lstm_hip_get_teacher_kl(self._h, _ptr(out, C.c_double), C.c_int64(k)))
        return out

    # ---- data-parallel -----------------------------------------------------------------------
    def comm_init(self, unique_id, nranks, rank):
        buf = (C.c_uint8 * UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
        _chk(self.lib.lstm_hip_comm_init(self._h, buf, nranks, rank))

    def allreduce_grads(self):
        _chk(self.lib.lstm_hip_allreduce_grads(self._h))

    def set_stride(self, stride, carry_col=1):
        _chk(self.lib.lstm_hip_set_stride(self._h, stride, carry_col))

    def set_global_batch(self, gb):
        _chk(self.lib.lstm_hip_set_global_batch(self._h, gb))

    def set_loss_mode(self, mode):
        """LOSS_ALL_STEPS_BITS (R/lstm.cc:204-207), LOSS_LAST_STEP_NATS (OV/lstm_eigen_class_CUDA/lstm.h:200-221) or
        LOSS_LAST_STEP_BITS (cuLSTM::calculate_loss, OV/lstm_eigen_class_CUDA/cu_lstm.h:203-215)."""
        _chk(self.lib.lstm_hip_set_loss_mode(self._h, mode))

    # ---- device-resident loop ------------------------------------------------------------------
    def set_text(self, text):
        text = np.ascontiguousarray(text, dtype=np.uint8)
        _chk(self.lib.lstm_hip_set_text(self._h, _ptr(text, C.c_uint8), C.c_size_t(text.size)))

    def set_cursors(self, pos):
        pos = np.ascontiguousarray(pos, dtype=np.uint64)
        assert pos.size == self.B
        _chk(self.lib.lstm_hip_set_cursors(self._h, _ptr(pos, C.c_uint64)))

    def get_cursors(self):
        pos = np.empty(self.B, np.uint64)
        _chk(self.lib.lstm_hip_get_cursors(self._h, _ptr(pos, C.c_uint64)))
        return pos

    def reset_window(self):
        _chk(self.lib.lstm_hip_reset_window(self._h))

    def train_windows(self, count, lr, want_losses=True, want_time=False):
        losses = np.zeros(count, np.float64) if want_losses else None
        ms = C.c_float(0)
        steps = self._updates_in(count)
        _chk(self.lib.lstm_hip_train_windows(self._h, C.c_int64(count), C.c_double(lr),
                                             _ptr(losses, C.c_double) if want_losses else None,
                                             C.byref(ms) if want_time else None))
        self._steps, self._kls = steps, count
        if want_time:
            return losses, ms.value
        return losses

    # ---- training on separate texts, each from its zero state (lstm_hip_set_train_texts) -------------
    def set_train_texts(self, texts, weights=None):
        """lstm_hip_set_train_texts: the texts (bytes or uint8 arrays, one stream each) the next train_text_windows calls
        train on, placed on the B lanes by text_plan(S - 1, B, lengths).  Zeroes the streams' bits and starts at window 0;
        None or an empty list drops the texts.  Returns the plan's number of windows.
        weights (lstm_hip_set_train_texts_weighted): per text a float array of the text's length -- entry i weighs byte i as
        a target in the loss and the gradient -- or a scalar for the whole text; completion_weights(texts, sep) makes those
        of completion-only training.  None is the unweighted call."""
        if not texts:
            _chk(self.lib.lstm_hip_set_train_texts(self._h, C.c_int32(0), None, None))
            self._train_streams = 0
            return 0
        parts = _bytes_list(texts)
        data, off = _offsets(parts)
        if weights is None:
            _chk(self.lib.lstm_hip_set_train_texts(self._h, C.c_int32(len(parts)), _ptr(data, C.c_uint8), _ptr(off, C.c_uint64)))
        else:
            if len(weights) != len(parts):
                raise LstmHipError(f"set_train_texts: {len(weights)} weight arrays for {len(parts)} texts")
            ws = []
            for s, (t, w) in enumerate(zip(parts, weights)):
                w = np.asarray(w, np.float32)
                w = np.full(t.size, w, np.float32) if w.ndim == 0 else w.ravel()
                if w.size != t.size:
                    raise LstmHipError(f"set_train_texts: text {s} has {t.size} bytes and {w.size} weights")
                ws.append(w)
            wdata = np.ascontiguousarray(np.concatenate(ws) if off[-1] > 0 else np.zeros(1, np.float32))
            _chk(self.lib.lstm_hip_set_train_texts_weighted(self._h, C.c_int32(len(parts)), _ptr(data, C.c_uint8),
                                                            _ptr(off, C.c_uint64), _ptr(wdata, C.c_float)))
        self._train_streams = len(parts)
        return self.train_texts_progress()[0]

    def train_texts_progress(self):
        """lstm_hip_get_train_texts: (windows of the plan, the next window to run)."""
        windows, nxt = C.c_int64(), C.c_int64()
        _chk(self.lib.lstm_hip_get_train_texts(self._h, C.byref(windows), C.byref(nxt)))
        return windows.value, nxt.value

    def train_text_windows(self, count, lr, want_losses=True, want_time=False):
        """lstm_hip_train_text_windows: the next `count` windows of the plan, one update each; every text starts from
        h = c = 0 and a row without a target adds nothing to the gradient.  Returns the windows' losses (all-steps bits), and
        the HIP-event time of the loop with want_time."""
        losses = np.zeros(count, np.float64) if want_losses else None
        ms = C.c_float(0)
        steps = self._updates_in(count)
        _chk(self.lib.lstm_hip_train_text_windows(self._h, C.c_int64(count), C.c_double(lr),
                                                  _ptr(losses, C.c_double) if want_losses else None,
                                                  C.byref(ms) if want_time else None))
        self._steps = steps
        if want_time:
            return losses, ms.value
        return losses

    def train_texts_bits(self):
        """lstm_hip_get_train_texts_bits: float64 [streams], each text's summed surprisal so far, every byte scored under
        the parameters its window had before its update (prequential bits)."""
        bits = np.zeros(max(getattr(self, "_train_streams", 0), 1), np.float64)
        _chk(self.lib.lstm_hip_get_train_texts_bits(self._h, _ptr(bits, C.c_double)))
        return bits[:getattr(self, "_train_streams", 0)]

    # ---- evaluator / sampler -------------------------------------------------------------------
    def eval_bits(self, text):
        text = np.ascontiguousarray(text, dtype=np.uint8)
        out = C.c_double()
        _chk(self.lib.lstm_hip_eval_bits(self._h, _ptr(text, C.c_uint8), C.c_size_t(text.size), C.byref(out)))
        return out.value

    def eval_texts(self, texts, h0=None, c0=None, skip=None, lanes=0, surprisal=False, want_time=False):
        """lstm_hip_eval_texts: held-out bits of `texts` (bytes or uint8 arrays, one stream each) through the training
        window's forward path, `lanes` streams side by side (0: the handle's B).  Byte j >= 1 of a text is scored on the
        state after bytes 0..j-1, byte 0 never; bytes below skip[s] (None: no skip) are fed but not scored.  h0, c0:
        [streams, N] or None for zeros.  Returns a dict: "bits" float64 [streams], each stream's summed surprisal; "h", "c"
        [streams, N], the state after each text's last FED byte, its last but one (not score()'s state after the last byte:
        the next piece of a chained text starts with this piece's last byte again); "surprisal", with surprisal=True, one
        float32 array per text indexed like it (0 for unscored bytes), else None; "ms", with want_time=True, the HIP-event
        time of the device loop, else None."""
        parts = _bytes_list(texts)
        streams = len(parts)
        data, off = _offsets(parts)
        total = int(off[-1])
        hh = None if h0 is None else _f32(h0).reshape(streams, self.N)
        cc = None if c0 is None else _f32(c0).reshape(streams, self.N)
        sk = None if skip is None else np.ascontiguousarray(skip, dtype=np.uint64).reshape(streams)
        sur = np.zeros(max(total, 1), np.float32) if surprisal else None
        bits = np.zeros(max(streams, 1), np.float64)
        h, c = np.empty((max(streams, 1), self.N), np.float32), np.empty((max(streams, 1), self.N), np.float32)
        opt = _EvalOpt(C.sizeof(_EvalOpt), int(lanes))
        ms = C.c_float(0)
        _chk(self.lib.lstm_hip_eval_texts(self._h, C.c_int32(streams), _ptr(data, C.c_uint8), _ptr(off, C.c_uint64),
                                          _ptr(hh) if hh is not None else None, _ptr(cc) if cc is not None else None,
                                          _ptr(sk, C.c_uint64) if sk is not None else None, C.byref(opt), _ptr(bits, C.c_double),
                                          _ptr(sur) if sur is not None else None, _ptr(h), _ptr(c),
                                          C.byref(ms) if want_time else None))
        return {"bits": bits[:streams], "h": h[:streams], "c": c[:streams],
                "surprisal": [sur[int(off[s]):int(off[s + 1])] for s in range(streams)] if surprisal else None,
                "ms": ms.value if want_time else None}

    def embed_texts(self, texts, h0=None, c0=None, skip=None, lanes=0, pool=("mean", "max", "last"), cell=False, pick=None,
                    want_time=False):
        """lstm_hip_embed_texts: what the model computed about `texts` (bytes or uint8 arrays, one stream each), on
        eval_texts' engine.  Unlike eval_texts every byte is fed: position i of a text is the state after its bytes 0..i.
        pool: which of "mean", "max", "last" to return -- mean and max over the positions skip[s] .. L - 1 (None: all), last
        the state after the whole text; each comes back as pool + "_h" [streams, N], and with cell=True as pool + "_c" too.
        pick: positions indexed like the concatenated texts, strictly increasing, or "all" for every position; their
        states come back as "picked_h" (and "picked_c") [npick, N].  Also "count" int64 [streams], the pooled positions,
        "bits" float64 [streams], eval_texts' figure, and "ms" with want_time=True."""
        parts = _bytes_list(texts)
        streams = len(parts)
        data, off = _offsets(parts)
        total = int(off[-1])
        hh = None if h0 is None else _f32(h0).reshape(streams, self.N)
        cc = None if c0 is None else _f32(c0).reshape(streams, self.N)
        sk = None if skip is None else np.ascontiguousarray(skip, dtype=np.uint64).reshape(streams)
        pool = (pool,) if isinstance(pool, str) else tuple(pool)
        for name in pool:
            if name not in ("mean", "max", "last"):
                raise LstmHipError(f"embed_texts: pool {name!r} is none of mean, max, last")
        if isinstance(pick, str):
            if pick != "all":
                raise LstmHipError(f"embed_texts: pick {pick!r} is neither positions nor \"all\"")
            pick = np.arange(total, dtype=np.uint64)
        pk = None if pick is None else np.ascontiguousarray(pick, dtype=np.uint64).reshape(-1)
        npick = 0 if pk is None else int(pk.size)
        res = {}
        out = _Embedding(size=C.sizeof(_Embedding))
        for src in ("h", "c") if cell else ("h",):
            for name in pool:
                res[f"{name}_{src}"] = np.empty((max(streams, 1), self.N), np.float32)
                setattr(out, f"{name}_{src}", _ptr(res[f"{name}_{src}"]))
            if npick:
                res[f"picked_{src}"] = np.empty((npick, self.N), np.float32)
                setattr(out, f"picked_{src}", _ptr(res[f"picked_{src}"]))
        count, bits = np.zeros(max(streams, 1), np.int64), np.zeros(max(streams, 1), np.float64)
        out.count, out.bits = _ptr(count, C.c_int64), _ptr(bits, C.c_double)
        opt = _EvalOpt(C.sizeof(_EvalOpt), int(lanes))
        ms = C.c_float(0)
        _chk(self.lib.lstm_hip_embed_texts(self._h, C.c_int32(streams), _ptr(data, C.c_uint8), _ptr(off, C.c_uint64),
                                           _ptr(hh) if hh is not None else None, _ptr(cc) if cc is not None else None,
                                           _ptr(sk, C.c_uint64) if sk is not None else None, C.byref(opt),
                                           _ptr(pk, C.c_uint64) if npick else None, C.c_int64(npick), C.byref(out),
                                           C.byref(ms) if want_time else None))
        res = {k: (v if k.startswith("picked") else v[:streams]) for k, v in res.items()}
        if pk is not None and not npick:
            for src in ("h", "c") if cell else ("h",):
                res[f"picked_{src}"] = np.empty((0, self.N), np.float32)
        res.update(count=count[:streams], bits=bits[:streams], ms=ms.value if want_time else None)
        return res

    def eval_split(self, text, pieces, warm=0, lanes=0):
        """Bits per character of one text, cut into `pieces` streams that are evaluated side by side (eval_split_pieces):
        piece i > 0 starts from a zero state `warm` bytes before its first scored byte, so the figure is the single
        stream's only in the limit of a long warm-up (warm >= len(text): exactly the single stream's rule)."""
        text = _bytes_list([text])[0]
        cut = eval_split_pieces(text.size, pieces, warm)
        r = self.eval_texts([text[a:b] for a, b, _ in cut], skip=[k for _, _, k in cut], lanes=lanes)
        return float(r["bits"].sum()) / (text.size - 1)

    def sample(self, h0, c0, u):
        h0, c0 = _f32(h0).copy(), _f32(c0).copy()
        u = np.ascontiguousarray(u, dtype=np.float64)
        out = np.zeros(u.size, np.uint8)
        _chk(self.lib.lstm_hip_sample(self._h, _ptr(h0), _ptr(c0), _ptr(u, C.c_double), int(u.size),
                                      _ptr(out, C.c_uint8)))
        return out, h0, c0

    def generate(self, prompts=None, count=0, u=None, temperature=1.0, h0=None, c0=None, streams=None, score=False,
                 top_k=0, top_p=1.0, stop_byte=None, info=False, constraint=None, start_state=None, accept=None,
                 logit_bias=None, min_p=0.0, no_repeat_ngram=0, history=None, guides=None, main_weight=1.0):
        """lstm_hip_generate: `streams` independent streams, each fed its prompt (bytes or a uint8 array) and then `count`
        drawn bytes.  u: draws [count, streams] (may be None only at temperature 0); h0, c0: [streams, N] or None (zeros).
        Returns (out [count, streams] uint8, bits [streams] float64 -- the prompts' summed -log2 p, or None unless
        score --, h [streams, N], c [streams, N]: the state after each stream's last input).
        top_k (1..255), top_p (< 1) and stop_byte (0..255) are the sampling controls of lstm_hip_generate_ex: keep the k
        most likely bytes, the smallest most-likely-first prefix of mass top_p, and end a stream with its first drawn
        stop_byte (out is 0 behind it, h / c are the state after it).  info=True adds a fifth element
        {"out_len": int32 [streams], "kept": uint16 [count, streams]}: bytes each stream produced, bytes kept per draw.
        constraint: a (states, 256) uint16 table (dfa_utf8(), dfa_restrict(), or the caller's own: the state after byte b in
        state q, 0xFFFF where b is forbidden) for lstm_hip_generate_constrained: every stream draws only bytes its state
        allows, from start_state [streams] (None: 0) advanced over its prompt; info then also has "end_state": int32
        [streams].  With constraint=None the calls are those made without the argument.
        accept: [states] flags, nonzero where a stream may end, with the meaning it has in beam_search
        (lstm_hip_generate_accepting): a byte is drawn only where an accepted end can still be reached within `count`, so
        every stream ends in an accepting state, by its stop byte or with exactly `count` bytes.  accept=None is the call
        made without the argument.
        logit_bias (a 256-array or a {byte: value} dict, added to the logits of drawn bytes), min_p (0 < min_p <= 1: cut the
        terms below min_p times the largest) and no_repeat_ngram (n in 1..64: no byte is drawn that would complete an n-gram
        the stream's text already holds; history: per stream the bytes that precede its prompt for this rule only) are the
        logit processors of lstm_hip_generate_processed.  They go with every argument above; with all four at their
        defaults the calls are those made without them.
        guides: [(model, weight, h0, c0), ...] (lstm_hip_generate_guided; 1 to 4 entries, h0 / c0 [streams, model.N] or None
        or left out: zeros; model may be this object).  Every guide is fed this call's prompts and drawn bytes from its own
        state, and a drawn byte's logits become main_weight * z + the sum of weight * the guide's logits, ahead of every
        processor.  With info=True the guides' end states are info["guide_h"], info["guide_c"]: one [streams, model.N] array
        per guide.  Without guides the calls are those made without the argument."""
        if streams is None:
            streams = len(prompts) if prompts is not None else (np.asarray(h0).shape[0] if h0 is not None else
                                                                (np.asarray(u).reshape(count, -1).shape[1] if u is not None and count > 0 else 1))
        streams = int(streams)
        d_p = d_off = None
        if prompts is not None:
            assert len(prompts) == streams, (len(prompts), streams)
            parts = [np.frombuffer(bytes(p), np.uint8) if isinstance(p, (bytes, bytearray)) else np.asarray(p, np.uint8).ravel()
                     for p in prompts]
            off = np.zeros(streams + 1, np.uint64)
            off[1:] = np.cumsum([q.size for q in parts])
            d_p = np.ascontiguousarray(np.concatenate(parts) if off[-1] > 0 else np.zeros(1, np.uint8))
            d_off = off
        hh = None if h0 is None else _f32(h0).reshape(streams, self.N)
        cc = None if c0 is None else _f32(c0).reshape(streams, self.N)
        uu = None if u is None else np.ascontiguousarray(u, dtype=np.float64).reshape(count, streams)
        out = np.zeros((count, streams), np.uint8)
        bits = np.zeros(streams, np.float64) if score else None
        h = np.empty((streams, self.N), np.float32)
        c = np.empty((streams, self.N), np.float32)
        args = (self._h, C.c_int32(streams), _ptr(d_p, C.c_uint8) if d_p is not None else None,
                _ptr(d_off, C.c_uint64) if d_off is not None else None,
                _ptr(hh) if hh is not None else None, _ptr(cc) if cc is not None else None)
        tail = (_ptr(uu, C.c_double) if uu is not None else None, C.c_int32(count), _ptr(out, C.c_uint8),
                _ptr(bits, C.c_double) if score else None, _ptr(h), _ptr(c))
        if constraint is None and start_state is not None:
            raise LstmHipError("generate: start_state given without a constraint")
        if constraint is None and accept is not None:
            raise LstmHipError("generate: accept given without a constraint")
        if guides is None and main_weight != 1.0:
            raise LstmHipError("generate: main_weight given without guides")
        if logit_bias is not None or min_p != 0.0 or no_repeat_ngram != 0 or history is not None or guides is not None:
            return self._generate_processed(args, tail, streams, count, temperature, top_k, top_p, stop_byte, info, constraint,
                                            start_state, accept, logit_bias, min_p, no_repeat_ngram, history, out, bits, h, c,
                                            guides, main_weight)
        if constraint is None and top_k == 0 and top_p == 1.0 and stop_byte is None and not info:
            _chk(self.lib.lstm_hip_generate(*args, C.c_double(temperature), *tail))
            return out, bits, h, c
        opt = _Sampling(C.sizeof(_Sampling), float(temperature), int(top_k), float(top_p),
                        -1 if stop_byte is None else int(stop_byte))
        out_len = np.zeros(streams, np.int32)
        kept = np.zeros((count, streams), np.uint16)
        if constraint is not None:
            table = np.ascontiguousarray(constraint, dtype=np.uint16)
            assert table.ndim == 2 and table.shape[1] == 256, table.shape
            con = _Constraint(C.sizeof(_Constraint), table.shape[0], _ptr(table, C.c_uint16))
            q0 = None if start_state is None else np.ascontiguousarray(start_state, dtype=np.int32).reshape(streams)
            q1 = np.zeros(streams, np.int32)
            if accept is not None:
                acc = np.ascontiguousarray(np.asarray(accept).reshape(table.shape[0]) != 0, dtype=np.uint8)
                bc = _BeamConstraint(C.sizeof(_BeamConstraint), C.pointer(con), _ptr(acc, C.c_uint8))
                _chk(self.lib.lstm_hip_generate_accepting(
                    *args, C.byref(opt), *tail, _ptr(out_len, C.c_int32), _ptr(kept, C.c_uint16) if info else None, C.byref(bc),
                    _ptr(q0, C.c_int32) if q0 is not None else None, _ptr(q1, C.c_int32)))
                return (out, bits, h, c, {"out_len": out_len, "kept": kept, "end_state": q1}) if info else (out, bits, h, c)
            _chk(self.lib.lstm_hip_generate_constrained(
                *args, C.byref(opt), *tail, _ptr(out_len, C.c_int32), _ptr(kept, C.c_uint16) if info else None, C.byref(con),
                _ptr(q0, C.c_int32) if q0 is not None else None, _ptr(q1, C.c_int32)))
            return (out, bits, h, c, {"out_len": out_len, "kept": kept, "end_state": q1}) if info else (out, bits, h, c)
        _chk(self.lib.lstm_hip_generate_ex(*args, C.byref(opt), *tail, _ptr(out_len, C.c_int32),
                                           _ptr(kept, C.c_uint16) if info else None))
        return (out, bits, h, c, {"out_len": out_len, "kept": kept}) if info else (out, bits, h, c)

    def _generate_processed(self, args, tail, streams, count, temperature, top_k, top_p, stop_byte, info, constraint,
                            start_state, accept, logit_bias, min_p, no_repeat_ngram, history, out, bits, h, c, guides=None,
                            main_weight=1.0):
        """generate() with a logit processor on: one lstm_hip_generate_processed call (with guides: lstm_hip_generate_guided)"""
        opt = _Sampling(C.sizeof(_Sampling), float(temperature), int(top_k), float(top_p),
                        -1 if stop_byte is None else int(stop_byte))
        out_len = np.zeros(streams, np.int32)
        kept = np.zeros((count, streams), np.uint16)
        bc = q0 = q1 = None
        if constraint is not None:
            table = np.ascontiguousarray(constraint, dtype=np.uint16)
            assert table.ndim == 2 and table.shape[1] == 256, table.shape
            con = _Constraint(C.sizeof(_Constraint), table.shape[0], _ptr(table, C.c_uint16))
            q0 = None if start_state is None else np.ascontiguousarray(start_state, dtype=np.int32).reshape(streams)
            q1 = np.zeros(streams, np.int32)
            acc = None if accept is None else np.ascontiguousarray(np.asarray(accept).reshape(table.shape[0]) != 0, dtype=np.uint8)
            bc = _BeamConstraint(C.sizeof(_BeamConstraint), C.pointer(con), _ptr(acc, C.c_uint8) if acc is not None else None)
        bias = None
        if isinstance(logit_bias, dict):
            bias = np.zeros(256, np.float32)
            for b, v in logit_bias.items():
                bias[int(b)] = v
        elif logit_bias is not None:
            bias = _f32(logit_bias).reshape(256)
        d_h = d_hoff = None
        if history is not None:
            assert len(history) == streams, (len(history), streams)
            d_h, d_hoff = _offsets(_bytes_list(history))
        lp = _LogitProcessors(C.sizeof(_LogitProcessors), _ptr(bias) if bias is not None else None, float(min_p),
                              int(no_repeat_ngram), _ptr(d_h, C.c_uint8) if d_h is not None else None,
                              _ptr(d_hoff, C.c_uint64) if d_hoff is not None else None)
        call = self.lib.lstm_hip_generate_processed if guides is None else self.lib.lstm_hip_generate_guided
        gd, gh, gc, _alive = (None, None, None, None) if guides is None else _guidance(guides, main_weight, streams)
        _chk(call(*args, C.byref(opt), *tail, _ptr(out_len, C.c_int32), _ptr(kept, C.c_uint16) if info else None,
                  C.byref(bc) if bc is not None else None, _ptr(q0, C.c_int32) if q0 is not None else None,
                  _ptr(q1, C.c_int32) if q1 is not None else None, C.byref(lp), *(() if gd is None else (C.byref(gd),))))
        if not info:
            return out, bits, h, c
        extra = {"out_len": out_len, "kept": kept}
        if gd is not None:
            extra["guide_h"], extra["guide_c"] = gh, gc
        if q1 is not None:
            extra["end_state"] = q1
        return out, bits, h, c, extra

    def score(self, texts, h0=None, c0=None, first=False, top_n=0, constraint=None, start_state=None):
        """lstm_hip_score: what the model thinks of every byte of `texts` (bytes or uint8 arrays, one stream each; h0, c0:
        [streams, N] or None for zeros).  Byte j is scored on the state after bytes 0..j-1; byte 0 only with first=True
        (its entries are 0 otherwise).  Returns a dict: "surprisal", "entropy" (float32 [len]), "rank" (uint8 [len]),
        "top_byte" (uint8 [len, top_n]) and "top_bits" (float32 [len, top_n]) are lists with one array per text; "bits"
        float64 [streams], each stream's summed surprisal (with first=False and no constraint: generate(score=True)'s bits);
        "h", "c" [streams, N], the state after each text's last byte; "end_state" int32 [streams] under a constraint, else
        None.  constraint / start_state as in generate: forbidden bytes are masked out of the distribution every byte is
        scored under, and a text the table rejects is refused.  A long text scored in pieces, each later piece with
        first=True, h0 / c0 = the h / c and start_state = the end_state before it, gives the entries of the one call."""
        return self._score(texts, h0, c0, first, top_n, constraint, start_state, None, 1.0)

    def score_guided(self, texts, guides, main_weight=1.0, h0=None, c0=None, first=False, top_n=0, constraint=None,
                     start_state=None):
        """lstm_hip_score_guided: score() under a mix with other models.  guides / main_weight as in generate: every byte is
        scored under main_weight * z + the sum of weight * the guide's logits, the constraint mask behind the mix; the dict
        then also has "guide_h", "guide_c", one [streams, model.N] array per guide (to hand over with h / c when a text is
        scored in pieces).  score() keeps the signature it had: it makes the call it made before guides existed."""
        if guides is None:
            raise LstmHipError("score: score_guided without guides")
        return self._score(texts, h0, c0, first, top_n, constraint, start_state, guides, main_weight)

    def _score(self, texts, h0, c0, first, top_n, constraint, start_state, guides, main_weight):
        """score() and score_guided(): one lstm_hip_score / lstm_hip_score_guided call"""
        parts = _bytes_list(texts)
        streams, top_n = len(parts), int(top_n)
        data, off = _offsets(parts)
        total = int(off[-1])
        hh = None if h0 is None else _f32(h0).reshape(streams, self.N)
        cc = None if c0 is None else _f32(c0).reshape(streams, self.N)
        sur, ent = np.zeros(max(total, 1), np.float32), np.zeros(max(total, 1), np.float32)
        rank = np.zeros(max(total, 1), np.uint8)
        tby, tbi = np.zeros((max(total, 1), top_n), np.uint8), np.zeros((max(total, 1), top_n), np.float32)
        bits = np.zeros(streams, np.float64)
        h, c = np.empty((streams, self.N), np.float32), np.empty((streams, self.N), np.float32)
        if constraint is None and start_state is not None:
            raise LstmHipError("score: start_state given without a constraint")
        con = table = q0 = q1 = None
        if constraint is not None:
            table = np.ascontiguousarray(constraint, dtype=np.uint16)
            assert table.ndim == 2 and table.shape[1] == 256, table.shape
            con = _Constraint(C.sizeof(_Constraint), table.shape[0], _ptr(table, C.c_uint16))
            q0 = None if start_state is None else np.ascontiguousarray(start_state, dtype=np.int32).reshape(streams)
            q1 = np.zeros(streams, np.int32)
        opt = _Scoring(C.sizeof(_Scoring), int(bool(first)), top_n, C.pointer(con) if con is not None else None)
        out = _Scores(C.sizeof(_Scores), _ptr(sur), _ptr(ent), _ptr(rank, C.c_uint8), _ptr(tby, C.c_uint8) if top_n else None,
                      _ptr(tbi) if top_n else None, _ptr(bits, C.c_double), _ptr(q1, C.c_int32) if q1 is not None else None)
        if guides is None and main_weight != 1.0:
            raise LstmHipError("score: main_weight given without guides")
        call = self.lib.lstm_hip_score if guides is None else self.lib.lstm_hip_score_guided
        gd, gh, gc, _alive = (None, None, None, None) if guides is None else _guidance(guides, main_weight, streams)
        _chk(call(self._h, C.c_int32(streams), _ptr(data, C.c_uint8), _ptr(off, C.c_uint64),
                  _ptr(hh) if hh is not None else None, _ptr(cc) if cc is not None else None, C.byref(opt),
                  _ptr(q0, C.c_int32) if q0 is not None else None, C.byref(out), _ptr(h), _ptr(c),
                  *(() if gd is None else (C.byref(gd),))))
        cut = lambda a: [a[int(off[s]):int(off[s + 1])] for s in range(streams)]
        res = {"surprisal": cut(sur), "entropy": cut(ent), "rank": cut(rank), "top_byte": cut(tby), "top_bits": cut(tbi),
               "bits": bits, "h": h, "c": c, "end_state": q1}
        if gd is not None:
            res["guide_h"], res["guide_c"] = gh, gc
        return res

    def beam_search(self, prompts=None, count=0, beams=4, stop_byte=-1, h0=None, c0=None, streams=None, length_alpha=0.0,
                    trace=False, constraint=None, start_state=None, accept=None):
        """lstm_hip_beam_search: per stream the `beams` most likely continuations of its prompt the search finds.  Returns a
        list (one entry per stream) of lists of (bytes, bits), best first: the hypothesis cut to its length (a stop byte
        included) and its cost.  length_alpha > 0 re-ranks each stream's list on the host by bits / len**length_alpha (a
        stable sort; empty hypotheses rank by their bits); the ABI itself always returns raw cost order.  trace=True adds a
        second result {"out": uint8 [streams, beams, count], "out_len": int32 [streams, beams], "bits": float64 [streams,
        beams], "parent", "byte": uint8 [count, streams * beams]} with the call's raw arrays.
        constraint: a (states, 256) uint16 table as in generate, for lstm_hip_beam_search_constrained: the search is over the
        continuations the table accepts, from start_state [streams] (None: 0) advanced over the prompts.  accept: [states]
        flags, nonzero where a hypothesis may end (None: everywhere); with it every hypothesis of finite bits ends in an
        accepting state, by its stop byte or with exactly `count` bytes.  A stream whose table allows fewer than `beams`
        strings fills its list with (b"", inf) entries, "no such hypothesis": they are kept, last, and the length_alpha
        re-ranking leaves entries of infinite bits where they are.  Under a constraint the result is ALWAYS a pair: the
        second element has "end_state": int32 [streams, beams], the DFA state of every final slot in the ABI's raw cost
        order (like "out_len" and "bits", which it also holds), and with trace=True the other raw arrays as above.  With
        constraint=None the call and its result are those made without the argument."""
        if streams is None:
            streams = len(prompts) if prompts is not None else (np.asarray(h0).shape[0] if h0 is not None else 1)
        streams, count, W = int(streams), int(count), int(beams)
        d_p = d_off = None
        if prompts is not None:
            assert len(prompts) == streams, (len(prompts), streams)
            d_p, d_off = _offsets(_bytes_list(prompts))
        hh = None if h0 is None else _f32(h0).reshape(streams, self.N)
        cc = None if c0 is None else _f32(c0).reshape(streams, self.N)
        cols = max(streams * W, 1)
        out = np.zeros((cols, max(count, 0)), np.uint8)
        out_len = np.zeros(cols, np.int32)
        bits = np.zeros(cols, np.float64)
        tp = np.zeros((max(count, 0), cols), np.uint8)
        tb = np.zeros((max(count, 0), cols), np.uint8)
        opt = _Beam(C.sizeof(_Beam), W, int(stop_byte))
        args = (self._h, C.c_int32(streams), _ptr(d_p, C.c_uint8) if d_p is not None else None,
                _ptr(d_off, C.c_uint64) if d_off is not None else None, _ptr(hh) if hh is not None else None,
                _ptr(cc) if cc is not None else None, C.byref(opt), C.c_int32(count), _ptr(out, C.c_uint8),
                _ptr(out_len, C.c_int32), _ptr(bits, C.c_double), _ptr(tp, C.c_uint8) if trace else None,
                _ptr(tb, C.c_uint8) if trace else None)
        if constraint is None and (start_state is not None or accept is not None):
            raise LstmHipError("beam_search: start_state / accept given without a constraint")
        q1 = None
        if constraint is None:
            _chk(self.lib.lstm_hip_beam_search(*args))
        else:
            table = np.ascontiguousarray(constraint, dtype=np.uint16)
            assert table.ndim == 2 and table.shape[1] == 256, table.shape
            con = _Constraint(C.sizeof(_Constraint), table.shape[0], _ptr(table, C.c_uint16))
            acc = None if accept is None else np.ascontiguousarray(np.asarray(accept).reshape(table.shape[0]) != 0, dtype=np.uint8)
            bc = _BeamConstraint(C.sizeof(_BeamConstraint), C.pointer(con), _ptr(acc, C.c_uint8) if acc is not None else None)
            q0 = None if start_state is None else np.ascontiguousarray(start_state, dtype=np.int32).reshape(streams)
            q1 = np.zeros(cols, np.int32)
            _chk(self.lib.lstm_hip_beam_search_constrained(*args, C.byref(bc), _ptr(q0, C.c_int32) if q0 is not None else None,
                                                           _ptr(q1, C.c_int32)))
        res = []
        for s in range(streams):
            hyp = [(out[s * W + r, :out_len[s * W + r]].tobytes(), float(bits[s * W + r])) for r in range(W)]
            if length_alpha > 0:
                if constraint is None:
                    hyp.sort(key=lambda e: e[1] / max(len(e[0]), 1) ** length_alpha)
                else:  # entries of infinite bits (no such hypothesis) stay where they are
                    ranked = iter(sorted((e for e in hyp if e[1] != float("inf")),
                                         key=lambda e: e[1] / max(len(e[0]), 1) ** length_alpha))
                    hyp = [e if e[1] == float("inf") else next(ranked) for e in hyp]
            res.append(hyp)
        if trace:
            raw = {"out": out.reshape(streams, W, count), "out_len": out_len.reshape(streams, W),
                   "bits": bits.reshape(streams, W), "parent": tp, "byte": tb}
            if q1 is not None:
                raw["end_state"] = q1.reshape(streams, W)
            return res, raw
        if q1 is not None:
            return res, {"out_len": out_len.reshape(streams, W), "bits": bits.reshape(streams, W),
                         "end_state": q1.reshape(streams, W)}
        return res

    def encode(self, texts, trace=False):
        """lstm_hip_encode: each of `texts` (bytes or uint8 arrays) is one stream, coded from a zero state.  Returns
        (codes: list of bytes, bits: float64 [streams] -- the ideal length under the quantised model) and, with trace,
        a uint32 [total bytes, 3] array of (cum, freq, total) per coded byte in text order."""
        parts = _bytes_list(texts)
        streams = len(parts)
        data, off = _offsets(parts)
        cap = sum(code_bound(q.size) for q in parts)
        code = np.zeros(max(cap, 1), np.uint8)
        code_off = np.zeros(streams + 1, np.uint64)
        bits = np.zeros(streams, np.float64)
        tr = np.zeros((max(int(off[-1]), 1), 3), np.uint32) if trace else None
        _chk(self.lib.lstm_hip_encode(self._h, C.c_int32(streams), _ptr(data, C.c_uint8), _ptr(off, C.c_uint64),
                                      _ptr(code, C.c_uint8), C.c_uint64(cap), _ptr(code_off, C.c_uint64),
                                      _ptr(bits, C.c_double), _ptr(tr, C.c_uint32) if trace else None))
        codes = [code[int(code_off[s]):int(code_off[s + 1])].tobytes() for s in range(streams)]
        if trace:
            return codes, bits, tr[:int(off[-1])]
        return codes, bits

    def decode(self, codes, lengths):
        """lstm_hip_decode: stream s decodes `lengths[s]` bytes from codes[s].  Returns a list of bytes."""
        parts = _bytes_list(codes)
        streams = len(parts)
        assert len(lengths) == streams, (len(lengths), streams)
        data, code_off = _offsets(parts)
        text_off = np.zeros(streams + 1, np.uint64)
        text_off[1:] = np.cumsum([int(n) for n in lengths])
        text = np.zeros(max(int(text_off[-1]), 1), np.uint8)
        _chk(self.lib.lstm_hip_decode(self._h, C.c_int32(streams), _ptr(data, C.c_uint8), _ptr(code_off, C.c_uint64),
                                      _ptr(text_off, C.c_uint64), _ptr(text, C.c_uint8)))
        return [text[int(text_off[s]):int(text_off[s + 1])].tobytes() for s in range(streams)]

    def encode_mixed(self, texts, guides=None, main_weight=1.0, rate=0.0, trace=False, weights=False):
        """lstm_hip_encode_mixed: lstm_hip_encode on the log-linear mix of this model (weight main_weight) and
        guides = [(model, weight), ...]; with rate > 0 every stream learns its weights from the bytes it has coded.  Returns
        (codes, bits), then with trace the uint32 [total, 3] table entries, then with weights the float32 [streams, 1 + G]
        final weights and the float32 [total, 1 + G] weights each byte was coded under.  guides None: the call passes no
        guidance and no mix coding, which is lstm_hip_encode exactly (weights is then refused by the library)."""
        parts = _bytes_list(texts)
        streams = len(parts)
        data, off = _offsets(parts)
        total = int(off[-1])
        cap = sum(code_bound(q.size) for q in parts)
        code = np.zeros(max(cap, 1), np.uint8)
        code_off = np.zeros(streams + 1, np.uint64)
        bits = np.zeros(streams, np.float64)
        tr = np.zeros((max(total, 1), 3), np.uint32) if trace else None
        G1 = 1 + (len(guides) if guides is not None else 0)
        w_out = np.zeros((streams, G1), np.float32) if weights else None
        w_tr = np.zeros((max(total, 1), G1), np.float32) if weights else None
        gd = mx = alive = None
        if guides is not None:
            gd, alive = _coder_guidance(guides, main_weight)
            mx = _MixCoding(C.sizeof(_MixCoding), float(rate))
        _chk(self.lib.lstm_hip_encode_mixed(self._h, C.c_int32(streams), _ptr(data, C.c_uint8), _ptr(off, C.c_uint64),
                                            _ptr(code, C.c_uint8), C.c_uint64(cap), _ptr(code_off, C.c_uint64),
                                            _ptr(bits, C.c_double), _ptr(tr, C.c_uint32) if trace else None,
                                            C.byref(gd) if gd is not None else None, C.byref(mx) if mx is not None else None,
                                            _ptr(w_out) if weights else None, _ptr(w_tr) if weights else None))
        del alive
        res = ([code[int(code_off[s]):int(code_off[s + 1])].tobytes() for s in range(streams)], bits)
        if trace:
            res += (tr[:total],)
        if weights:
            res += (w_out, w_tr[:total])
        return res

    def decode_mixed(self, codes, lengths, guides=None, main_weight=1.0, rate=0.0, weights=False):
        """lstm_hip_decode_mixed: stream s decodes `lengths[s]` bytes from codes[s] under the same models, weights and rate
        as lstm_hip_encode_mixed.  Returns a list of bytes, and with weights the float32 [streams, 1 + G] final weights."""
        parts = _bytes_list(codes)
        streams = len(parts)
        assert len(lengths) == streams, (len(lengths), streams)
        data, code_off = _offsets(parts)
        text_off = np.zeros(streams + 1, np.uint64)
        text_off[1:] = np.cumsum([int(n) for n in lengths])
        text = np.zeros(max(int(text_off[-1]), 1), np.uint8)
        G1 = 1 + (len(guides) if guides is not None else 0)
        w_out = np.zeros((streams, G1), np.float32) if weights else None
        gd = mx = alive = None
        if guides is not None:
            gd, alive = _coder_guidance(guides, main_weight)
            mx = _MixCoding(C.sizeof(_MixCoding), float(rate))
        _chk(self.lib.lstm_hip_decode_mixed(self._h, C.c_int32(streams), _ptr(data, C.c_uint8), _ptr(code_off, C.c_uint64),
                                            _ptr(text_off, C.c_uint64), _ptr(text, C.c_uint8),
                                            C.byref(gd) if gd is not None else None, C.byref(mx) if mx is not None else None,
                                            _ptr(w_out) if weights else None))
        del alive
        out = [text[int(text_off[s]):int(text_off[s + 1])].tobytes() for s in range(streams)]
        return (out, w_out) if weights else out

    def encode_adaptive(self, texts, lr, trace=False):
        """lstm_hip_encode_adaptive: the handle's B streams coded block by block, the model trained on every block after it
        was coded (this CHANGES the handle: parameters, optimizer state and step count, window, carry).  Returns (codes: list
        of bytes, bits: float64 [B], block_bits: float64 [n_blocks + 1], the last entry the untrained tail's) and, with
        trace, the uint32 [total bytes, 3] array of (cum, freq, total) in text order."""
        parts = _bytes_list(texts)
        assert len(parts) == self.B, (len(parts), self.B)
        data, off = _offsets(parts)
        n_blocks = adaptive_blocks(self.S, self.B, off)
        cap = sum(code_bound(q.size) for q in parts)
        code = np.zeros(max(cap, 1), np.uint8)
        code_off = np.zeros(self.B + 1, np.uint64)
        bits = np.zeros(self.B, np.float64)
        block_bits = np.zeros(n_blocks + 1, np.float64)
        tr = np.zeros((max(int(off[-1]), 1), 3), np.uint32) if trace else None
        _chk(self.lib.lstm_hip_encode_adaptive(self._h, _ptr(data, C.c_uint8), _ptr(off, C.c_uint64), C.c_double(lr),
                                               _ptr(code, C.c_uint8), C.c_uint64(cap), _ptr(code_off, C.c_uint64),
                                               _ptr(bits, C.c_double), _ptr(block_bits, C.c_double),
                                               _ptr(tr, C.c_uint32) if trace else None))
        self._steps = n_blocks
        codes = [code[int(code_off[s]):int(code_off[s + 1])].tobytes() for s in range(self.B)]
        if trace:
            return codes, bits, block_bits, tr[:int(off[-1])]
        return codes, bits, block_bits

    def decode_adaptive(self, codes, lengths, lr):
        """lstm_hip_decode_adaptive on a handle identical to the encoder's before its call: stream s decodes lengths[s]
        bytes from codes[s], and the handle ends as the encoder's did.  Returns a list of bytes."""
        parts = _bytes_list(codes)
        assert len(parts) == self.B and len(lengths) == self.B, (len(parts), len(lengths), self.B)
        data, code_off = _offsets(parts)
        text_off = np.zeros(self.B + 1, np.uint64)
        text_off[1:] = np.cumsum([int(n) for n in lengths])
        text = np.zeros(max(int(text_off[-1]), 1), np.uint8)
        _chk(self.lib.lstm_hip_decode_adaptive(self._h, _ptr(data, C.c_uint8), _ptr(code_off, C.c_uint64),
                                               _ptr(text_off, C.c_uint64), C.c_double(lr), _ptr(text, C.c_uint8)))
        self._steps = adaptive_blocks(self.S, self.B, text_off)
        return [text[int(text_off[s]):int(text_off[s + 1])].tobytes() for s in range(self.B)]

    def plan_identity(self):
        """lstm_hip_plan_identity: what of the engine plan decides the order of a training window's sums."""
        buf = C.create_string_buffer(256)
        _chk(self.lib.lstm_hip_plan_identity(self._h, buf, C.c_size_t(256)))
        return buf.value.decode()

    def debug_stamps(self):
        out = np.zeros((4, self.S, 16), np.uint64)  # [fwd wg0, fwd wg1, bwd wg0, bwd wg1][step][slot]
        _chk(self.lib.lstm_hip_debug_stamps(self._h, _ptr(out, C.c_uint64), C.c_size_t(out.size)))
        return out

    # ---- measurement ---------------------------------------------------------------------------
    def synchronize(self):
        _chk(self.lib.lstm_hip_synchronize(self._h))

    def set_profiling(self, on):
        _chk(self.lib.lstm_hip_set_profiling(self._h, 1 if on else 0))

    def reset_kernel_stats(self):
        _chk(self.lib.lstm_hip_reset_kernel_stats(self._h))

    def kernel_stats(self):
        out = {}
        for i in range(self.lib.lstm_hip_kernel_stat_count(self._h)):
            name, n, ms = C.c_char_p(), C.c_int64(), C.c_double()
            _chk(self.lib.lstm_hip_kernel_stat(self._h, i, C.byref(name), C.byref(n), C.byref(ms)))
            out[name.value.decode()] = (n.value, ms.value)
        return out


# ---- the build's seeded stand-ins for the reference's unseeded randomness -----------------------
class MT19937Normal:
    """MT19937 (init_genrand seeding) + 53-bit uniforms (genrand_res53) + Marsaglia polar normals:
    the seeded replacement for the reference's `std::mt19937 mt(rd()); std::normal_distribution<>`
    (R/lstm.cc:370-372).  Spec shared with the C++ host driver (host/rng.h); independent of oracle/.

    numpy's legacy RandomState(seed).random_sample() IS init_genrand + genrand_res53, so the uniform
    stream comes from it; the polar transform is applied to consecutive uniform pairs in order and
    the normals are buffered, which is exactly the sequential algorithm (accepted pair -> u*m then v*m).
    """

    def __init__(self, seed):
        self._rs = np.random.RandomState(int(seed) & 0xFFFFFFFF)
        self._buf = np.empty(0, np.float64)

    def uniform(self):
        assert self._buf.size == 0, "uniform() after buffered normals would reorder the stream"
        return float(self._rs.random_sample())

    def _refill(self, need):
        chunks = [self._buf]
        have = self._buf.size
        while have < need:
            k = max(1024, int((need - have) * 0.7))
            uv = 2.0 * self._rs.random_sample(2 * k).reshape(k, 2) - 1.0
            s = (uv * uv).sum(axis=1)
            ok = (s < 1.0) & (s != 0.0)
            uv, s = uv[ok], s[ok]
            m = np.sqrt(-2.0 * np.log(s) / s)
            z = (uv * m[:, None]).ravel()  # u0*m0, v0*m0, u1*m1, ...
            chunks.append(z)
            have += z.size
        self._buf = np.concatenate(chunks)

    def normals(self, n):
        if self._buf.size < n:
            self._refill(n)
        out, self._buf = self._buf[:n], self._buf[n:]
        return out

    def randn(self, rows, cols, mean, std):
        """row-outer / column-inner fill order of R/lstm.cc:374-378; returns [cols, rows] C-order
        (= the bytes of a column-major rows x cols matrix)."""
        z = self.normals(rows * cols).reshape(rows, cols)
        return np.ascontiguousarray((mean + std * z).astype(np.float32).T)


def init_params(rng, N, M=VOCAB, forget_bias=0.0):
    """R/lstm.cc:113-119: W, U, Why ~ N(0, 0.01) in that order, b = by = 0; flat block.
    forget_bias = 1 reproduces the later variants' b[2N:3N] = 1 (OV/lstm_eigen_class_batch/lstm.cc:81)."""
    W = rng.randn(4 * N, M, 0.0, 0.01)
    U = rng.randn(4 * N, N, 0.0, 0.01)
    Why = rng.randn(M, N, 0.0, 0.01)
    b = np.zeros(4 * N, np.float32)
    b[2 * N:3 * N] = forget_bias
    return np.concatenate([W.ravel(), U.ravel(), b, Why.ravel(), np.zeros(M, np.float32)])


def initial_cursors(length, S, B, stream0=0, streams_total=None):
    """pos[b] = S + (b*(len-S))/B: deterministic stand-in for rand()%(len-S)+S (OV/lstm_eigen_opt/lstm.cc:140-144)."""
    total = B if streams_total is None else streams_total
    return np.array([S + ((stream0 + b) * (length - S)) // total for b in range(B)], dtype=np.uint64)
