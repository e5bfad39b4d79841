"""CPU: weight averaging at the boundary -- the six entry points are declared, bound and exported, the constants agree between
the header and Python, the pins that decide the design still hold (the average is no fifth `which` block and its launch has no
KernelId), the update launch is as it was, and the training program's --average options refuse bad values before any library
call.  Linked against a library that lacks the entry points (which the program references weakly) it refuses --average and
otherwise runs exactly as before."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSTM = os.path.join(ROOT, "eigen-lstm_amd", "lstm")
HOST_DIR = os.path.join(ROOT, "eigen-lstm_amd", "host")
CSRC = os.path.join(ROOT, "eigen-lstm_amd", "csrc")
NAMES = ("lstm_hip_set_averaging", "lstm_hip_get_average", "lstm_hip_set_average", "lstm_hip_get_averaging_counts",
         "lstm_hip_set_averaging_counts", "lstm_hip_set_inference_source")


def _header():
    return open(os.path.join(ROOT, "include", "lstm_hip.h")).read()


def test_entry_points_are_declared_and_bound():
    import lstm_hip
    header = _header()
    for line in ("int lstm_hip_set_averaging(lstm_hip_t *h, int32_t kind, double decay, int32_t every);",
                 "int lstm_hip_get_average(lstm_hip_t *h, float *host_block);",
                 "int lstm_hip_set_average(lstm_hip_t *h, const float *host_block);",
                 "int lstm_hip_get_averaging_counts(lstm_hip_t *h, int64_t *seen, int64_t *n);",
                 "int lstm_hip_set_averaging_counts(lstm_hip_t *h, int64_t seen, int64_t n);",
                 "int lstm_hip_set_inference_source(lstm_hip_t *h, int32_t source);"):
        assert line in header, line
    assert set(NAMES) <= set(lstm_hip.SYMBOLS)
    sig = {name: str(inspect.signature(getattr(lstm_hip.Lstm, name)))
           for name in ("set_averaging", "get_average", "set_average", "averaging_counts", "set_averaging_counts",
                        "set_inference_source")}
    assert sig == {"set_averaging": "(self, kind, decay=0.0, every=1)", "get_average": "(self)", "set_average": "(self, block)",
                   "averaging_counts": "(self)", "set_averaging_counts": "(self, seen, n)",
                   "set_inference_source": "(self, source)"}, sig


def test_constants_agree_between_header_and_python():
    import lstm_hip
    header = _header()
    for name in ("AVG_OFF", "AVG_EMA", "AVG_UNIFORM", "SRC_PARAMS", "SRC_AVERAGE"):
        m = re.search(rf"^#define LSTM_HIP_{name} (\d+)$", header, re.M)
        assert m, name
        assert int(m.group(1)) == getattr(lstm_hip, name), name
    assert (lstm_hip.AVG_OFF, lstm_hip.AVG_EMA, lstm_hip.AVG_UNIFORM) == (0, 1, 2)
    assert (lstm_hip.SRC_PARAMS, lstm_hip.SRC_AVERAGE) == (0, 1)


def test_the_built_library_exports_them():
    import lstm_hip
    lib = lstm_hip.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name


def _body(src, head):
    """the text of the function whose definition starts with `head`, braces matched"""
    at = src.index(head)
    i = src.index("{", at)
    depth = 0
    for j in range(i, len(src)):
        depth += {"{": 1, "}": -1}.get(src[j], 0)
        if depth == 0:
            return src[at:j + 1]
    raise AssertionError(head)


def test_the_average_has_a_launch_of_its_own():
    """no KernelId, no statistics row, no fifth block; one call behind the update launch, on handles that asked for it"""
    api = open(os.path.join(CSRC, "lstm_hip_api.cpp")).read()
    enum = api[api.index("enum KernelId {"):api.index("K_COUNT")]
    assert re.findall(r"\bK_\w+", re.sub(r"//.*", "", enum))[-2:] == ["K_BEAM_BACKTRACK", "K_SCORE_HEAD"]
    assert re.search(r'"beam_backtrack",\s*"score_head"\};', api)
    assert "which == 3 ? h->adam_v : nullptr;" in api
    body = _body(api, "int do_adagrad(lstm_hip_ctx *h, double lr, int64_t norm_idx)")
    update = body.index("RUN(adam ? K_ADAM : K_ADAGRAD, adagrad(job, h->st));")
    call = body.index("if (h->avg_kind != LSTM_HIP_AVG_OFF) return average_step(h);")
    assert update < call
    assert "avg" not in body[:update] and "average" not in body[:update]  # nothing of it before or in the update launch
    step = _body(api, "int average_step(lstm_hip_ctx *h)")
    assert "average(h->P, h->avg, h->pl.total, w, n == 1, h->plan.n_cus, h->st);" in step
    assert "RUN(" not in step and "Synchronize" not in step and "Memcpy" not in step and "st2" not in step
    # the update launch's job carries nothing of it
    kernels_h = open(os.path.join(CSRC, "kernels.h")).read()
    job = _body(kernels_h, "struct AdagradJob")
    assert "avg" not in job and "average" not in job
    kernels = open(os.path.join(CSRC, "kernels.hip")).read()
    k = _body(kernels, "__global__ __launch_bounds__(256) void k_average(")
    assert "atomic" not in k and "__shared__" not in k and "__syncthreads" not in k and "fma" not in k.lower()
    assert "float4" in k


@pytest.fixture(scope="module")
def stub_exe(tmp_path_factory):
    """the program linked against the GPU-less stub of the C ABI, which exports none of the averaging calls"""
    d = tmp_path_factory.mktemp("avgstub")
    so = d / "liblstm_hip.so"
    stub = os.path.join(ROOT, "tests", "fake_gpu", "lstm_hip_stub.c")
    for name in NAMES:
        assert name not in open(stub).read(), name
    subprocess.check_call(["gcc", "-O1", "-fPIC", "-shared", stub, "-o", str(so)])
    exe = d / "lstm_stub_linked"
    subprocess.check_call(["g++", "-O1", "-std=c++17", os.path.join(HOST_DIR, "lstm_main.cc"), "-o", str(exe), "-L" + str(d),
                           "-llstm_hip", "-Wl,-rpath," + str(d)])
    text = d / "corpus.txt"
    np.random.RandomState(3).randint(97, 123, size=2000).astype(np.uint8).tofile(text)
    return d, str(exe), str(text)


BAD = [
    (["--average", "mean"], "--average"),
    (["--average", ""], "--average"),
    (["--average", "ema", "--average-decay", "1"], "--average-decay"),
    (["--average", "ema", "--average-decay", "-0.1"], "--average-decay"),
    (["--average", "ema", "--average-decay", "nan"], "--average-decay"),
    (["--average", "ema", "--average-decay", "inf"], "--average-decay"),
    (["--average", "ema", "--average-decay", "0.9x"], "--average-decay"),
    (["--average", "uniform", "--average-decay", "0.9"], "--average-decay"),   # the uniform mean has no decay
    (["--average", "ema", "--average-every", "0"], "--average-every"),
    (["--average", "uniform", "--average-every", "-3"], "--average-every"),
    (["--average", "uniform", "--average-every", "2.5"], "--average-every"),
    (["--average", "uniform", "--average-every", "99999999999"], "--average-every"),
    (["--average", "ema", "--average-start", "-1"], "--average-start"),
    (["--average", "ema", "--average-start", "ten"], "--average-start"),
    (["--average-decay", "0.99"], "--average-decay"),                          # the averaging options need --average
    (["--average-every", "2"], "--average-every"),
    (["--average-start", "10"], "--average-start"),
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


def test_missing_entry_points_refuse_average_only(stub_exe):
    d, exe, text = stub_exe
    base = [exe, text, "16", "8", "2", "0.1", "--windows", "3", "--sample", "0", "--epochs", "1", "--quiet"]
    log = d / "calls_missing.log"
    env = dict(os.environ, LSTM_STUB_LOG=str(log))
    for kind in ("ema", "uniform"):
        out = subprocess.run(base + ["--average", kind], capture_output=True, text=True, env=env, timeout=60)
        assert out.returncode == 2 and "lstm_hip_set_averaging" in out.stderr, (out.returncode, out.stderr)
        assert not log.exists() or log.read_text() == "", log.read_text()
    # without the option the same binary runs as before
    calls = d / "calls_plain.log"
    out = subprocess.run(base, capture_output=True, text=True, env=dict(os.environ, LSTM_STUB_LOG=str(calls)), timeout=60)
    assert out.returncode == 0, out.stderr
    assert "average" not in out.stdout
    names = [line.split()[2] for line in calls.read_text().splitlines()]
    assert "train_windows" in names and not any("averag" in n or "inference" in n for n in names), names


@pytest.mark.parametrize("args", [["--average", "ema", "--average-decay", "1"], ["--average-every", "4"]])
def test_built_program_refuses_a_bad_value(tmp_path, args):
    f = tmp_path / "corpus.txt"
    f.write_bytes(b"the quick brown fox jumps over the lazy dog " * 20)
    out = subprocess.run([LSTM, str(f), "32", "8", "4", "0.1", "--windows", "5", "--sample", "0"] + args,
                         capture_output=True, text=True, errors="replace", timeout=60)
    assert out.returncode == 2 and args[-2] in out.stderr, (out.returncode, out.stderr)
    assert "Read " not in out.stdout  # refused while parsing, before the corpus or the device


def test_usage_text_names_the_options():
    out = subprocess.run([LSTM, "--help"], capture_output=True, text=True, timeout=60)
    for opt in ("--average ema|uniform", "--average-decay", "--average-every", "--average-start"):
        assert opt in out.stdout + out.stderr, opt
