"""CPU: the boundary of the adaptive coder (lstm_hip_encode_adaptive / lstm_hip_decode_adaptive) that
needs no device -- the symbols, the block count, null arguments -- and the argument and container checks of
`lstm_compress --adapt`, which must refuse a foreign LHAD container before anything touches a device."""
import ctypes as C
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CMP = os.path.join(ROOT, "eigen-lstm_amd", "lstm_compress")
USAGE = "usage: lstm_compress --load PREFIX (-c|-d) IN OUT [--streams K] [--fast-math] [--device D]\n"
NEW = ("lstm_hip_adaptive_version", "lstm_hip_adaptive_blocks", "lstm_hip_encode_adaptive", "lstm_hip_decode_adaptive")


def test_adaptive_calls_are_declared_exported_and_listed():
    import lstm_hip
    lib = lstm_hip.load_library()
    header = open(os.path.join(ROOT, "include", "lstm_hip.h")).read()
    for name in NEW + ("lstm_hip_plan_identity",):
        assert hasattr(lib, name) and name in lstm_hip.SYMBOLS, name
        assert re.search(r"\b%s\(" % name, header), name


def test_adaptive_version_and_the_static_coder_version():
    import lstm_hip
    assert lstm_hip.adaptive_version() >= 1
    assert lstm_hip.coder_version() == 1  # the static coder is untouched


@pytest.mark.parametrize("S,lengths", [
    (26, [100, 77, 130]),      # ragged
    (26, [100, 0, 130]),       # an empty stream: nothing is trained
    (26, [24, 24]),            # shorter than a block
    (26, [25, 25]),            # exactly one block
    (2, [5, 9, 7]),            # one byte per block
    (100, [6336]),
    (100, [99 * 3 + 98] * 64),
])
def test_adaptive_blocks_needs_no_device(S, lengths):
    import lstm_hip
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    assert lstm_hip.adaptive_blocks(S, len(lengths), off) == min(lengths) // (S - 1)


def test_adaptive_blocks_refuses_bad_arguments_with_a_message():
    import lstm_hip
    lib = lstm_hip.load_library()
    good = (C.c_uint64 * 3)(0, 10, 20)
    assert lib.lstm_hip_adaptive_blocks(26, 2, None) == lstm_hip.EINVAL
    assert b"text_off" in lib.lstm_hip_last_error()
    assert lib.lstm_hip_adaptive_blocks(1, 2, good) == lstm_hip.EINVAL
    assert lib.lstm_hip_adaptive_blocks(26, 0, good) == lstm_hip.EINVAL
    assert lib.lstm_hip_adaptive_blocks(26, 2, (C.c_uint64 * 3)(1, 10, 20)) == lstm_hip.EINVAL
    assert lib.lstm_hip_adaptive_blocks(26, 2, (C.c_uint64 * 3)(0, 10, 5)) == lstm_hip.EINVAL
    assert b"decreases" in lib.lstm_hip_last_error()
    with pytest.raises(lstm_hip.LstmHipError):
        lstm_hip.adaptive_blocks(26, 2, [0, 10, 5])


def test_adaptive_calls_refuse_a_null_handle_with_a_message():
    import lstm_hip
    lib = lstm_hip.load_library()
    text = (C.c_uint8 * 4)(1, 2, 3, 4)
    off = (C.c_uint64 * 2)(0, 4)
    code = (C.c_uint8 * 64)()
    code_off = (C.c_uint64 * 2)()
    lib.lstm_hip_encode_adaptive.restype = C.c_int
    lib.lstm_hip_decode_adaptive.restype = C.c_int
    rc = lib.lstm_hip_encode_adaptive(None, text, off, C.c_double(0.1), code, C.c_uint64(64), code_off, None, None, None)
    assert rc == lstm_hip.EINVAL and b"null handle" in lib.lstm_hip_last_error()
    rc = lib.lstm_hip_decode_adaptive(None, code, code_off, off, C.c_double(0.1), text)
    assert rc == lstm_hip.EINVAL and b"null handle" in lib.lstm_hip_last_error()
    buf = C.create_string_buffer(128)
    assert lib.lstm_hip_plan_identity(None, buf, C.c_size_t(128)) == lstm_hip.EINVAL


# ---- the program ------------------------------------------------------------------------------------------------------
def _run(args, cwd):
    return subprocess.run([CMP] + args, capture_output=True, text=True, timeout=60, cwd=cwd)


@pytest.mark.parametrize("args", [
    ["--adapt"],                                                   # nothing to do
    ["--adapt", "-c", "in"],                                       # OUT missing
    ["--adapt", "-c", "in", "out", "-d", "a", "b"],                # both directions
    ["--adapt", "-c", "in", "out", "--hidden", "0"],
    ["--adapt", "-c", "in", "out", "--hidden", "x"],
    ["--adapt", "-c", "in", "out", "--seq", "1"],
    ["--adapt", "-c", "in", "out", "--streams", "4097"],
    ["--adapt", "-c", "in", "out", "--lr", "-0.1"],
    ["--adapt", "-c", "in", "out", "--lr", "inf"],
    ["--adapt", "-c", "in", "out", "--lr", "nan"],
    ["--adapt", "-c", "in", "out", "--lr"],                        # missing value
    ["--adapt", "-c", "in", "out", "--clip-norm", "-1"],
    ["--adapt", "-c", "in", "out", "--optimizer", "sgd"],
    ["--adapt", "-c", "in", "out", "--adam-betas", "0.9"],
    ["--adapt", "-c", "in", "out", "--optimizer", "adam", "--adam-betas", "0.9,1.0"],
    ["--adapt", "-c", "in", "out", "--optimizer", "adam", "--adam-eps", "0"],
    ["--adapt", "-c", "in", "out", "--weight-decay", "0.1"],       # needs --optimizer adam
    ["--adapt", "-c", "in", "out", "--bogus"],
    ["--adapt", "-d", "in", "out", "--hidden", "64"],              # -d reads the model from the container
    ["--adapt", "-d", "in", "out", "--lr", "0.1"],
    ["--adapt", "-d", "in", "out", "--streams", "4"],
    ["--adapt", "-d", "in", "out", "--stable-softmax"],
    ["--load", "ck", "-c", "in", "out", "--hidden", "64"],         # model options need --adapt
    ["--load", "ck", "-c", "in", "out", "--lr", "0.1"],
    ["--load", "ck", "-c", "in", "out", "--bf16"],
])
def test_program_refuses_malformed_adaptive_arguments_with_usage(args, tmp_path):
    out = _run(args, tmp_path)
    assert out.returncode == 2, (args, out.returncode, out.stderr)
    assert USAGE in out.stderr  # the existing usage text, whole, is still the start of the usage
    assert "--adapt" in out.stderr.split(USAGE, 1)[1]
    assert out.stdout == ""


def test_help_starts_with_the_existing_usage(tmp_path):
    out = _run(["--help"], tmp_path)
    assert out.returncode == 0 and out.stdout.startswith(USAGE) and "--adapt" in out.stdout


PAD_HIDDEN = 256
HEADER = 312


def _lhad(text=b"hello world", magic=0x4441484C, fmt=1, coder=None, adaptive=None, N=4, S=4, B=1, flags=PAD_HIDDEN, lr=0.05,
          opt=0, prior=0, codes=None, cus=256, hash_=0):
    import lstm_hip
    coder = lstm_hip.coder_version() if coder is None else coder
    adaptive = lstm_hip.adaptive_version() if adaptive is None else adaptive
    codes = [b"\0" * 7] * B if codes is None else codes
    head = struct.pack("<IIIIIIIIdII4ddIIQQII", magic, fmt, coder, adaptive, N, S, B, flags, lr, opt, prior, 0.0, 0.0, 0.0, 0.0,
                       0.0, 1, cus, hash_, len(text), zlib.crc32(text), 0)
    head += b"some device".ljust(64, b"\0") + b"some plan".ljust(128, b"\0")
    assert len(head) == HEADER
    return head + b"".join(struct.pack("<Q", len(c)) for c in codes) + b"".join(codes)


@pytest.mark.parametrize("case,message", [
    ("magic", "bad magic"),
    ("short", "truncated header"),
    ("short_lengths", "truncated header"),
    ("format", "container format"),
    ("coder", "coder version"),
    ("adaptive", "adaptive version"),
    ("hidden", "hidden size"),
    ("window", "window of"),
    ("streams", "stream count"),
    ("flags", "unknown flags"),
    ("lr", "learning rate"),
    ("optimizer", "optimizer kind"),
    ("code_size", "code bytes"),
    ("hash", "parameter hash"),
    ("prior", "--load PREFIX"),
])
def test_program_refuses_a_foreign_adaptive_container_before_any_device_call(tmp_path, case, message):
    good = _lhad()
    data = {
        "magic": _lhad(magic=0x12345678),
        "short": good[:100],
        "short_lengths": good[:HEADER + 4],
        "format": _lhad(fmt=2),
        "coder": _lhad(coder=0xFFFF),
        "adaptive": _lhad(adaptive=0xFFFF),
        "hidden": _lhad(N=0),
        "window": _lhad(S=1),
        "streams": _lhad(B=0, codes=[]),
        "flags": _lhad(flags=PAD_HIDDEN | (1 << 20)),
        "lr": _lhad(lr=float("nan")),
        "optimizer": _lhad(opt=7),
        "code_size": good[:-1],
        "hash": good,                  # well-formed, but the seeded initialisation does not hash to 0
        "prior": _lhad(prior=1),       # coded from a checkpoint, none given
    }[case]
    f = tmp_path / "x.lhad"
    f.write_bytes(data)
    out = _run(["--adapt", "-d", str(f), str(tmp_path / "y")], tmp_path)
    assert out.returncode == 1, (case, out.returncode, out.stderr)
    assert message in out.stderr, (case, out.stderr)
    assert "lstm_hip_create" not in out.stderr  # refused before a handle was asked for
    assert not (tmp_path / "y").exists() and not (tmp_path / "y.tmp").exists()


def test_each_decoder_names_the_other_container(tmp_path):
    lhad = tmp_path / "x.lhad"
    lhad.write_bytes(_lhad())
    lhac = tmp_path / "x.lhac"
    lhac.write_bytes(struct.pack("<IIIIIQQII", 0x4341484C, 1, 1, 4, 0, 0, 5, 1, 0) + struct.pack("<Q", 7) + b"\0" * 7)
    out = _run(["--load", str(tmp_path / "none"), "-d", str(lhad), str(tmp_path / "y")], tmp_path)
    assert out.returncode == 1 and "LHAD" in out.stderr and "--adapt -d" in out.stderr, out.stderr
    out = _run(["--adapt", "-d", str(lhac), str(tmp_path / "y")], tmp_path)
    assert out.returncode == 1 and "LHAC" in out.stderr and "--load PREFIX -d" in out.stderr, out.stderr
    assert not (tmp_path / "y").exists()
