"""CPU: the batched generator's boundary (lstm_hip_generate in include/lstm_hip.h) and the command line of the program that
uses it (eigen-lstm_amd/lstm_generate).  Argument errors must be refused before anything touches a device."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "eigen-lstm_amd", "lstm_generate")


def test_generate_is_declared_exported_and_listed():
    import lstm_hip
    lib = lstm_hip.load_library()
    assert hasattr(lib, "lstm_hip_generate")
    assert "lstm_hip_generate" in lstm_hip.SYMBOLS
    header = open(os.path.join(ROOT, "include", "lstm_hip.h")).read()
    assert re.search(r"int lstm_hip_generate\(lstm_hip_t \*h, int32_t streams,", header)


def test_return_codes_match_the_header():
    import lstm_hip
    header = open(os.path.join(ROOT, "include", "lstm_hip.h")).read()
    codes = {k: int(v) for k, v in re.findall(r"#define LSTM_HIP_(OK|E[A-Z]+) \(?(-?\d+)\)?", header)}
    assert codes == {"OK": lstm_hip.OK, "EINVAL": lstm_hip.EINVAL, "EHIP": lstm_hip.EHIP, "ENODEV": lstm_hip.ENODEV,
                     "ERCCL": lstm_hip.ERCCL, "ESTATE": lstm_hip.ESTATE}


def test_generate_refuses_a_null_handle_with_a_message():
    import lstm_hip
    lib = lstm_hip.load_library()
    out = (C.c_uint8 * 4)()
    rc = lib.lstm_hip_generate(None, 1, None, None, None, None, C.c_double(0.0), None, 4, out, None, None, None)
    assert rc == lstm_hip.EINVAL
    assert lib.lstm_hip_last_error()


@pytest.mark.parametrize("args", [
    [],                                                              # no --load
    ["--load", "ck"],                                                # nothing to do
    ["--load", "ck", "--count", "abc"],
    ["--load", "ck", "--count", "-3"],
    ["--load", "ck", "--count", "10", "--streams", "0"],
    ["--load", "ck", "--count", "10", "--streams", "5000"],
    ["--load", "ck", "--count", "10", "--temperature", "-1"],
    ["--load", "ck", "--count", "10", "--temperature", "nan"],
    ["--load", "ck", "--count", "10", "--prime", "a", "--prime-file", "f"],
    ["--load", "ck", "--prime", "a"],                                # sampling options without --count
    ["--load", "ck", "--prime-file", "f"],
    ["--load", "ck", "--score", "f", "--streams", "4"],
    ["--load", "ck", "--score", "f", "--temperature", "0.5"],
    ["--load", "ck", "--score", "f", "--seed", "3"],
    ["--load", "ck", "--count", "10", "--seed"],                     # missing value
    ["--load", "ck", "--bogus"],
])
def test_program_refuses_malformed_arguments_with_usage(args, tmp_path):
    out = subprocess.run([GEN] + args, capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert out.returncode == 2, (args, out.returncode, out.stdout, out.stderr)
    assert "usage: lstm_generate --load PREFIX" in out.stderr
    assert out.stdout == ""


def test_program_reports_a_missing_checkpoint_before_any_device_call(tmp_path):
    out = subprocess.run([GEN, "--load", str(tmp_path / "nothing"), "--count", "5"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 1
    assert "cannot read" in out.stderr and "nothing_W.txt" in out.stderr
