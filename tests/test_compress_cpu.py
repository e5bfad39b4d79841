"""CPU: the range coder's specification (tests/range_coder_ref.py, the Python copy of the device coder), the boundary of
lstm_hip_encode / lstm_hip_decode and the container checks of eigen-lstm_amd/lstm_compress, which must refuse a file that
does not belong to the checkpoint before anything touches a device."""
import ctypes as C
import itertools
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

import range_coder_ref as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CMP = os.path.join(ROOT, "eigen-lstm_amd", "lstm_compress")
USAGE = "usage: lstm_compress --load PREFIX (-c|-d) IN OUT"


def _code_table(q):
    cum = list(itertools.accumulate(q, initial=0))
    return cum


def _random_tables(rs, n, kind):
    tables = []
    for _ in range(n):
        if kind == "random":
            q = 1 + rs.randint(0, 250, size=256)
        else:  # worst case: the largest total the quantisation allows, everything else at the minimum frequency
            q = np.ones(256, np.int64)
            q[rs.randint(256)] += 65025
        tables.append([int(v) for v in q])
    return tables


@pytest.mark.parametrize("kind", ["random", "worst"])
def test_reference_coder_round_trips_within_the_bound(kind):
    import lstm_hip
    rs = np.random.RandomState(7 if kind == "random" else 8)
    for n in (0, 1, 2, 5, 100, 700):
        tables = _random_tables(rs, n, kind)
        if kind == "random":
            syms = [int(rs.randint(256)) for _ in range(n)]
        else:  # always the least likely symbol (random among the ties)
            syms = [int(rs.choice([m for m in range(256) if t[m] == 1])) for t in tables]
        cums = [_code_table(t) for t in tables]
        code = rc.encode((cums[i][s], tables[i][s], cums[i][-1]) for i, s in enumerate(syms))
        assert len(code) <= lstm_hip.code_bound(n), (n, len(code))
        if n == 0:
            assert code == b""
        assert rc.decode(code, n, rc.table_model(tables)) == syms
        if n:
            # the ideal length plus at most 4 flush bytes and the cut's loss
            ideal = sum(-np.log2(tables[i][s] / cums[i][-1]) for i, s in enumerate(syms))
            assert 8 * len(code) <= ideal + 32 + 1.1 * n, (8 * len(code), ideal)
            # a truncated code still decodes to the requested length (bytes past the end read as 0)
            assert len(rc.decode(code[: len(code) // 2], n, rc.table_model(tables))) == n


def test_reference_coder_refuses_totals_above_two_to_the_sixteen():
    with pytest.raises(rc.CoderError):
        rc.encode([(0, 1, (1 << 16) + 1)])
    with pytest.raises(rc.CoderError):
        rc.encode([(5, 0, 300)])


def test_code_bound_and_version_need_no_device():
    import lstm_hip
    assert lstm_hip.code_bound(0) == 0
    for n in (1, 2, 1000, 10 ** 9):
        assert lstm_hip.code_bound(n) == 3 * n + 4
    assert lstm_hip.code_bound(2 ** 64 - 1) == 2 ** 64 - 1  # overflow: SIZE_MAX
    assert lstm_hip.coder_version() >= 1


def test_coder_is_declared_exported_and_listed():
    import lstm_hip
    lib = lstm_hip.load_library()
    header = open(os.path.join(ROOT, "include", "lstm_hip.h")).read()
    for name in ("lstm_hip_coder_version", "lstm_hip_code_bound", "lstm_hip_encode", "lstm_hip_decode"):
        assert hasattr(lib, name) and name in lstm_hip.SYMBOLS
        assert re.search(r"\b%s\(" % name, header)


def test_coder_refuses_a_null_handle_with_a_message():
    import lstm_hip
    lib = lstm_hip.load_library()
    text = (C.c_uint8 * 4)(1, 2, 3, 4)
    off = (C.c_uint64 * 2)(0, 4)
    code = (C.c_uint8 * 64)()
    code_off = (C.c_uint64 * 2)()
    assert lib.lstm_hip_encode(None, 1, text, off, code, C.c_uint64(64), code_off, None, None) == lstm_hip.EINVAL
    assert lib.lstm_hip_last_error()
    assert lib.lstm_hip_decode(None, 1, code, code_off, off, text) == lstm_hip.EINVAL


# ---- the program's container checks ------------------------------------------------------------------------------------
N_SMALL = 4


def _write_checkpoint(prefix, seed):
    """the five-file text checkpoint (host/checkpoint.h) of a random N = 4 model; returns the flat block"""
    rs = np.random.RandomState(seed)
    N, M = N_SMALL, 256
    shapes = [("W", 4 * N, M), ("U", 4 * N, N), ("b", 4 * N, 1), ("Why", M, N), ("by", M, 1)]
    parts = []
    for name, r, c in shapes:
        a = (rs.randn(r, c) * 0.1).astype(np.float32)
        np.savetxt(f"{prefix}_{name}.txt", a, fmt="%.9g")
        parts.append(a.ravel(order="F"))
    return np.concatenate(parts)


def _fnv1a(P):
    h = 0xCBF29CE484222325
    for b in np.asarray(P, np.float32).tobytes():
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def _container(P, text=b"hello", magic=0x4341484C, fmt=1, version=None, N=N_SMALL, codes=(b"\0\0\0\0\0\0\0",)):
    import lstm_hip
    version = lstm_hip.coder_version() if version is None else version
    head = struct.pack("<IIIIIQQII", magic, fmt, version, N, 0, _fnv1a(P), len(text), len(codes), zlib.crc32(text))
    assert len(head) == 44
    return head + b"".join(struct.pack("<Q", len(c)) for c in codes) + b"".join(codes)


@pytest.fixture
def ck(tmp_path):
    prefix = str(tmp_path / "ck")
    return prefix, _write_checkpoint(prefix, seed=1)


def _run(args, cwd):
    return subprocess.run([CMP] + args, capture_output=True, text=True, timeout=60, cwd=cwd)


def test_hash_matches_the_program(ck, tmp_path):
    """the Python FNV-1a above is the program's: a container that differs only in its hash is refused for the hash"""
    prefix, P = ck
    other = P.copy()
    other[0] += 1.0
    f = tmp_path / "x.lhac"
    f.write_bytes(_container(other))
    out = _run(["--load", prefix, "-d", str(f), str(tmp_path / "y")], tmp_path)
    assert out.returncode == 1 and "parameter hash" in out.stderr, out.stderr
    assert not (tmp_path / "y").exists()


@pytest.mark.parametrize("case,message", [
    ("magic", "bad magic"),
    ("short", "truncated header"),
    ("short_lengths", "truncated header"),
    ("format", "container format"),
    ("version", "coder version"),
    ("hidden", "hidden size"),
    ("streams", "stream count"),
    ("code_size", "code bytes"),
])
def test_program_refuses_a_foreign_container_before_any_device_call(ck, tmp_path, case, message):
    prefix, P = ck
    good = _container(P)
    data = {
        "magic": _container(P, magic=0x12345678),
        "short": good[:30],
        "short_lengths": good[:44 + 4],
        "format": _container(P, fmt=2),
        "version": _container(P, version=0xFFFF),
        "hidden": _container(P, N=8),
        "streams": _container(P, codes=()),
        "code_size": good[:-1],
    }[case]
    f = tmp_path / "x.lhac"
    f.write_bytes(data)
    out = _run(["--load", prefix, "-d", str(f), str(tmp_path / "y")], tmp_path)
    assert out.returncode == 1, (case, out.returncode, out.stderr)
    assert message in out.stderr, (case, out.stderr)
    assert "lstm_hip_create" not in out.stderr  # refused before a handle was asked for
    assert not (tmp_path / "y").exists() and not (tmp_path / "y.tmp").exists()


def test_program_reports_a_missing_checkpoint(tmp_path):
    f = tmp_path / "in.txt"
    f.write_bytes(b"abc")
    out = _run(["--load", str(tmp_path / "nothing"), "-c", str(f), str(tmp_path / "out")], tmp_path)
    assert out.returncode == 1 and "nothing_W.txt" in out.stderr
    assert not (tmp_path / "out").exists()


@pytest.mark.parametrize("args", [
    [],                                                   # no --load
    ["--load", "ck"],                                     # nothing to do
    ["--load", "ck", "-c", "in"],                         # OUT missing
    ["--load", "ck", "-c", "in", "out", "-d", "a", "b"],  # both directions
    ["--load", "ck", "-c", "in", "out", "--streams", "0"],
    ["--load", "ck", "-c", "in", "out", "--streams", "4097"],
    ["--load", "ck", "-c", "in", "out", "--streams", "x"],
    ["--load", "ck", "-c", "in", "out", "--device"],      # missing value
    ["--load", "ck", "-d", "in", "out", "--streams", "4"],
    ["--load", "ck", "-d", "in", "out", "--fast-math"],
    ["--load", "ck", "-c", "in", "out", "--bogus"],
])
def test_program_refuses_malformed_arguments_with_usage(args, tmp_path):
    out = _run(args, tmp_path)
    assert out.returncode == 2, (args, out.returncode, out.stderr)
    assert USAGE in out.stderr
    assert out.stdout == ""
