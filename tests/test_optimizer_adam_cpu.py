"""CPU: Adam / AdamW at the boundary -- the three entry points are declared, bound and exposed, and the training program's
--optimizer, --adam-betas, --adam-eps and --weight-decay options refuse bad values (and the Adam options without
--optimizer adam) before any library call.  Linked against a library that lacks the entry points (which the program
references weakly) it refuses --optimizer adam and otherwise runs exactly as before."""
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
    assert "#define LSTM_HIP_OPT_ADAGRAD 0" in header and "#define LSTM_HIP_OPT_ADAM 1" in header
    assert ("int lstm_hip_set_optimizer(lstm_hip_t *h, int32_t kind, double beta1, double beta2, double eps, "
            "double weight_decay);") in header
    assert "int lstm_hip_get_optimizer_steps(lstm_hip_t *h, int64_t *steps);" in header
    assert "int lstm_hip_set_optimizer_steps(lstm_hip_t *h, int64_t steps);" in header
    assert {"lstm_hip_set_optimizer", "lstm_hip_get_optimizer_steps", "lstm_hip_set_optimizer_steps"} <= set(lstm_hip.SYMBOLS)
    assert (lstm_hip.OPT_ADAGRAD, lstm_hip.OPT_ADAM, lstm_hip.P_ADAM_V) == (0, 1, 3)
    for name in ("set_optimizer", "optimizer_steps", "set_optimizer_steps"):
        assert callable(getattr(lstm_hip.Lstm, name)), name


def test_the_built_library_exports_them():
    import lstm_hip
    lib = lstm_hip.load_library()
    for name in ("lstm_hip_set_optimizer", "lstm_hip_get_optimizer_steps", "lstm_hip_set_optimizer_steps"):
        assert hasattr(lib, name), name


@pytest.fixture(scope="module")
def stub_exe(tmp_path_factory):
    """the program, unchanged, linked against the GPU-less stub of the C ABI (which does not export the optimizer calls)"""
    d = tmp_path_factory.mktemp("adamstub")
    so = d / "liblstm_hip.so"
    subprocess.check_call(["gcc", "-O1", "-fPIC", "-shared", os.path.join(ROOT, "tests", "fake_gpu", "lstm_hip_stub.c"), "-o", str(so)])
    exe = d / "lstm_stub_linked"
    subprocess.check_call(["g++", "-O1", "-std=c++17", os.path.join(HOST_DIR, "lstm_main.cc"), "-o", str(exe), "-L" + str(d),
                           "-llstm_hip", "-Wl,-rpath," + str(d)])
    text = d / "corpus.txt"
    np.random.RandomState(3).randint(97, 123, size=2000).astype(np.uint8).tofile(text)
    return d, str(exe), str(text)


BAD = [
    (["--optimizer", "sgd"], "--optimizer"),
    (["--optimizer", "adam", "--adam-betas", "1,0.999"], "--adam-betas"),
    (["--optimizer", "adam", "--adam-betas", "0.9,1"], "--adam-betas"),
    (["--optimizer", "adam", "--adam-betas", "-0.1,0.999"], "--adam-betas"),
    (["--optimizer", "adam", "--adam-betas", "0.9"], "--adam-betas"),
    (["--optimizer", "adam", "--adam-betas", "0.9,x"], "--adam-betas"),
    (["--optimizer", "adam", "--adam-betas", "nan,0.999"], "--adam-betas"),
    (["--optimizer", "adam", "--adam-eps", "0"], "--adam-eps"),
    (["--optimizer", "adam", "--adam-eps", "-1e-8"], "--adam-eps"),
    (["--optimizer", "adam", "--adam-eps", "inf"], "--adam-eps"),
    (["--optimizer", "adam", "--weight-decay", "-0.01"], "--weight-decay"),
    (["--optimizer", "adam", "--weight-decay", "nan"], "--weight-decay"),
    (["--weight-decay", "0.01"], "--weight-decay"),                 # Adam options need --optimizer adam
    (["--adam-eps", "1e-6", "--optimizer", "adagrad"], "--adam-eps"),
    (["--adam-betas", "0.9,0.99"], "--adam-betas"),
]


@pytest.mark.parametrize("args,name", BAD, ids=[" ".join(a) for a, _ in BAD])
def test_bad_option_is_refused_before_any_library_call(stub_exe, args, name):
    d, exe, text = stub_exe
    log = d / "calls_bad.log"
    if log.exists():
        log.unlink()
    env = dict(os.environ, LSTM_STUB_LOG=str(log))
    out = subprocess.run([exe, text, "16", "8", "2", "0.1", "--windows", "3", "--sample", "0"] + args,
                         capture_output=True, text=True, env=env, timeout=60)
    assert out.returncode == 2 and name in out.stderr, (out.returncode, out.stderr)
    assert not log.exists() or log.read_text() == "", log.read_text()


def test_missing_entry_points_refuse_adam_only(stub_exe):
    d, exe, text = stub_exe
    base = [exe, text, "16", "8", "2", "0.1", "--windows", "3", "--sample", "0", "--epochs", "1", "--quiet"]
    log = d / "calls_missing.log"
    env = dict(os.environ, LSTM_STUB_LOG=str(log))
    out = subprocess.run(base + ["--optimizer", "adam"], capture_output=True, text=True, env=env, timeout=60)
    assert out.returncode == 2 and "lstm_hip_set_optimizer" in out.stderr, (out.returncode, out.stderr)
    assert not log.exists() or log.read_text() == "", log.read_text()
    # without the option, and with the default rule named explicitly, the same binary runs as before: the same calls
    runs = []
    for extra in ([], ["--optimizer", "adagrad"]):
        calls = d / f"calls_{len(extra)}.log"
        out = subprocess.run(base + extra, capture_output=True, text=True, env=dict(os.environ, LSTM_STUB_LOG=str(calls)),
                             timeout=60)
        assert out.returncode == 0, out.stderr
        assert "Adam" not in out.stdout
        runs.append([" ".join(line.split()[2:]) for line in calls.read_text().splitlines()])  # (without pid and rank)
    assert runs[0] == runs[1]
    assert any(c.startswith("train_windows") for c in runs[0]), runs[0]


@pytest.mark.parametrize("args", [["--optimizer", "adam", "--adam-eps", "0"], ["--weight-decay", "0.1"]])
def test_built_program_refuses_a_bad_value(tmp_path, args):
    f = tmp_path / "corpus.txt"
    f.write_bytes(b"the quick brown fox jumps over the lazy dog " * 20)
    out = subprocess.run([LSTM, str(f), "32", "8", "4", "0.1", "--windows", "5", "--sample", "0"] + args,
                         capture_output=True, text=True, errors="replace", timeout=60)
    assert out.returncode == 2 and args[-2] in out.stderr, (out.returncode, out.stderr)
    assert "Read " not in out.stdout  # refused while parsing, before the corpus or the device


def test_usage_text_names_the_options():
    out = subprocess.run([LSTM, "--help"], capture_output=True, text=True, timeout=60)
    for opt in ("--optimizer adagrad|adam", "--adam-betas", "--adam-eps", "--weight-decay"):
        assert opt in out.stdout + out.stderr, opt
