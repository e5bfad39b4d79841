"""CPU: global-norm gradient clipping at the boundary -- the two entry points are declared and bound, and the training
program's --clip-norm option refuses a negative or NaN value before any library call (also when linked against a library
that lacks the entry points, which it references weakly and then refuses the option for)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSTM = os.path.join(ROOT, "eigen-lstm_amd", "lstm")
HOST_DIR = os.path.join(ROOT, "eigen-lstm_amd", "host")


def test_entry_points_are_declared_and_bound():
    import lstm_hip
    header = open(os.path.join(ROOT, "include", "lstm_hip.h")).read()
    assert "int lstm_hip_set_grad_clip(lstm_hip_t *h, double max_norm);" in header
    assert "int lstm_hip_get_grad_norms(lstm_hip_t *h, double *norms, int64_t n);" in header
    assert {"lstm_hip_set_grad_clip", "lstm_hip_get_grad_norms"} <= set(lstm_hip.SYMBOLS)
    assert callable(lstm_hip.Lstm.set_grad_clip) and callable(lstm_hip.Lstm.grad_norms)


@pytest.fixture(scope="module")
def stub_exe(tmp_path_factory):
    """the program, unchanged, linked against the GPU-less stub of the C ABI (which does not export the clipping calls)"""
    d = tmp_path_factory.mktemp("clipstub")
    so = d / "liblstm_hip.so"
    subprocess.check_call(["gcc", "-O1", "-fPIC", "-shared", os.path.join(ROOT, "tests", "fake_gpu", "lstm_hip_stub.c"), "-o", str(so)])
    exe = d / "lstm_stub_linked"
    subprocess.check_call(["g++", "-O1", "-std=c++17", os.path.join(HOST_DIR, "lstm_main.cc"), "-o", str(exe), "-L" + str(d),
                           "-llstm_hip", "-Wl,-rpath," + str(d)])
    text = d / "corpus.txt"
    np.random.RandomState(3).randint(97, 123, size=2000).astype(np.uint8).tofile(text)
    return d, str(exe), str(text)


@pytest.mark.parametrize("value", ["-1", "nan", "-inf", "x"])
def test_bad_value_is_refused_before_any_library_call(stub_exe, value):
    d, exe, text = stub_exe
    log = d / f"calls_{value}.log"
    env = dict(os.environ, LSTM_STUB_LOG=str(log))
    out = subprocess.run([exe, text, "16", "8", "2", "0.1", "--windows", "3", "--sample", "0", "--clip-norm", value],
                         capture_output=True, text=True, env=env, timeout=60)
    assert out.returncode == 2 and "--clip-norm" in out.stderr, (out.returncode, out.stderr)
    assert not log.exists() or log.read_text() == "", log.read_text()


def test_missing_entry_points_refuse_the_option(stub_exe):
    d, exe, text = stub_exe
    log = d / "calls_missing.log"
    env = dict(os.environ, LSTM_STUB_LOG=str(log))
    out = subprocess.run([exe, text, "16", "8", "2", "0.1", "--windows", "3", "--sample", "0", "--clip-norm", "5"],
                         capture_output=True, text=True, env=env, timeout=60)
    assert out.returncode == 2 and "lstm_hip_set_grad_clip" in out.stderr, (out.returncode, out.stderr)
    assert not log.exists() or log.read_text() == "", log.read_text()
    # without the option the same binary runs as before
    out = subprocess.run([exe, text, "16", "8", "2", "0.1", "--windows", "3", "--sample", "0", "--epochs", "1", "--quiet"],
                         capture_output=True, text=True, env=env, timeout=60)
    assert out.returncode == 0 and "grad norm" not in out.stdout, out.stderr


@pytest.mark.parametrize("value", ["-1", "nan"])
def test_built_program_refuses_a_bad_value(tmp_path, value):
    f = tmp_path / "corpus.txt"
    f.write_bytes(b"the quick brown fox jumps over the lazy dog " * 20)
    out = subprocess.run([LSTM, str(f), "32", "8", "4", "0.1", "--windows", "5", "--sample", "0", "--clip-norm", value],
                         capture_output=True, text=True, errors="replace", timeout=60)
    assert out.returncode == 2 and "--clip-norm" in out.stderr, (out.returncode, out.stderr)
    assert "Read " not in out.stdout  # refused while parsing, before the corpus or the device


def test_usage_text_names_the_option():
    out = subprocess.run([LSTM, "--help"], capture_output=True, text=True, timeout=60)
    assert "--clip-norm" in out.stdout + out.stderr
