"""CPU: weight drop at the boundary.  The Python transcription of the rule (weight_drop_ref.py) gives the header's known
answers; lstm_hip_weight_drop_mask, which is the shipped rule running on the CPU, equals it byte for byte and refuses bad
rates; the training program refuses bad --weight-drop values before any library call and, linked against a library without
the entry points, refuses the option and otherwise runs as before; the new launches stay outside the KernelId table and the
update launch carries nothing of the feature."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import weight_drop_ref as wd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSTM = os.path.join(ROOT, "eigen-lstm_amd", "lstm")
HOST_DIR = os.path.join(ROOT, "eigen-lstm_amd", "host")
CSRC = os.path.join(ROOT, "eigen-lstm_amd", "csrc")
NAMES = ("lstm_hip_set_weight_drop", "lstm_hip_get_weight_drop", "lstm_hip_weight_drop_mask")

KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,out", KNOWN, ids=["zeros", "ones", "pi"])
def test_reference_philox_known_answers(counter, key, out):
    assert wd.philox4x32_10(counter, key) == out
    # ... and the vectorised form the masks are made with: counter = (q lo, q hi, t lo, t hi), key = (seed lo, seed hi)
    q = counter[0] | counter[1] << 32
    t = counter[2] | counter[3] << 32
    seed = key[0] | key[1] << 32
    assert tuple(int(x) for x in wd._philox_quads(np.array([q], np.uint64), seed, t)[0]) == out


def test_reference_keep_count():
    keep = wd.mask(16, 0.25, seed=1, t=0)
    assert keep.shape == (64, 16) and keep.dtype == np.bool_
    assert int(keep.sum()) == 770


def test_reference_threshold_and_scale():
    assert wd.threshold(0.25) == 1 << 30 and wd.threshold(0.5) == 1 << 31 and wd.threshold(1e-12) == 0
    assert wd.threshold(0.999) == int(0.999 * 2.0 ** 32)
    assert wd.scale(0.5) == np.float32(2.0) and wd.scale(0.25) == np.float32(1.0 / 0.75)


def test_entry_points_are_declared_and_bound():
    import lstm_hip
    header = open(os.path.join(ROOT, "include", "lstm_hip.h")).read()
    for line in ("int lstm_hip_set_weight_drop(lstm_hip_t *h, double rate, uint64_t seed, uint64_t t);",
                 "int lstm_hip_get_weight_drop(lstm_hip_t *h, double *rate, uint64_t *seed, uint64_t *t);",
                 "int lstm_hip_weight_drop_mask(int32_t N, double rate, uint64_t seed, uint64_t t, uint8_t *keep);"):
        assert line in header, line
    assert set(NAMES) <= set(lstm_hip.SYMBOLS)
    lib = lstm_hip.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
    assert str(inspect.signature(lstm_hip.Lstm.set_weight_drop)) == "(self, rate, seed=0, t=0)"
    assert str(inspect.signature(lstm_hip.Lstm.weight_drop)) == "(self)"
    assert str(inspect.signature(lstm_hip.weight_drop_mask)) == "(N, rate, seed=0, t=0)"


SEED = 0x9E3779B97F4A7C15  # a non-zero high word


@pytest.mark.parametrize("t", [0, 1, 2 ** 32 + 5])
@pytest.mark.parametrize("rate", [1e-12, 0.25, 0.5, 0.999])
@pytest.mark.parametrize("N", [16, 30, 100, 128])
def test_library_mask_equals_the_reference(N, rate, t):
    import lstm_hip
    got = lstm_hip.weight_drop_mask(N, rate, SEED, t)
    assert got.shape == (4 * N, N) and got.dtype == np.bool_
    ref = wd.mask(N, rate, SEED, t)
    assert np.array_equal(got, ref), int((got != ref).sum())


def test_library_mask_known_count_and_raw_bytes():
    import ctypes as C
    import lstm_hip
    assert int(lstm_hip.weight_drop_mask(16, 0.25, 1, 0).sum()) == 770
    raw = np.full(4 * 16 * 16 + 8, 7, np.uint8)  # the call writes 4N * N bytes of 0 / 1 and nothing behind them
    rc = lstm_hip.load_library().lstm_hip_weight_drop_mask(C.c_int32(16), C.c_double(0.25), C.c_uint64(1), C.c_uint64(0),
                                                          raw.ctypes.data_as(C.POINTER(C.c_uint8)))
    assert rc == 0
    assert np.array_equal(raw[:1024], wd.flat_mask(16, 0.25, 1, 0).astype(np.uint8)) and (raw[1024:] == 7).all()
    assert lstm_hip.weight_drop_mask(16, 0.0).all()  # off keeps everything


@pytest.mark.parametrize("rate", [-0.1, 1.0, 1.5, float("nan"), float("inf"), float("-inf")])
def test_library_mask_refuses_bad_rates(rate):
    import lstm_hip
    with pytest.raises(lstm_hip.LstmHipError) as e:
        lstm_hip.weight_drop_mask(16, rate)
    assert "lstm_hip error -1:" in str(e.value), str(e.value)  # LSTM_HIP_EINVAL
    assert ("%g" % rate) in str(e.value), str(e.value)  # the message names the number


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


def test_the_mask_has_launches_of_its_own():
    """no KernelId, no RUN, no statistics row; nothing of it in the update launch or its job"""
    api = open(os.path.join(CSRC, "lstm_hip_api.cpp")).read()
    enum = re.sub(r"//.*", "", api[api.index("enum KernelId {"):api.index("K_COUNT")])
    assert not re.search(r"drop|mask", enum, re.I), enum
    names = api[api.index("kKernelNames[K_COUNT] = {"):api.index("};", api.index("kKernelNames[K_COUNT] = {"))]
    assert "drop" not in names
    launch = _body(api, "int weight_drop_launch(lstm_hip_ctx *h, const float *src, float *dst)")
    assert "weight_drop_mask(src, dst, h->cfg.N, h->N_log," in launch and 'return untimed_status("weight_drop");' in launch
    assert "RUN(" not in launch and "Synchronize" not in launch and "Memcpy" not in launch and "st2" not in launch
    assert not re.search(r"RUN\([^;]*weight_drop", api)
    kernels_h = open(os.path.join(CSRC, "kernels.h")).read()
    job = _body(kernels_h, "struct AdagradJob")
    kernels = open(os.path.join(CSRC, "kernels.hip")).read()
    upd = _body(kernels, "__global__ __launch_bounds__(256) void k_adagrad(")
    for text in (job, upd):
        assert not re.search(r"drop|philox|keep|\bwd_|\bUe\b", text, re.I)
    k = _body(kernels, "__global__ __launch_bounds__(256) void k_weight_drop(")
    assert "atomic" not in k and "__shared__" not in k and "__syncthreads" not in k and "fma" not in k.lower()
    assert "float4" in k and "in[c] * scale" in k
    # one rule: the kernel and the CPU entry point call the same header
    assert "weight_drop::quad_words(" in k and "weight_drop::keep_word(" in k
    cpu = _body(api, "int lstm_hip_weight_drop_mask(")
    assert "weight_drop::quad_words(" in cpu and "weight_drop::keep_word(" in cpu


@pytest.fixture(scope="module")
def stub_exe(tmp_path_factory):
    """the program linked against the GPU-less stub of the C ABI, which exports none of the weight-drop calls"""
    d = tmp_path_factory.mktemp("wdstub")
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
    (["--weight-drop", "0"], "--weight-drop"),
    (["--weight-drop", "1"], "--weight-drop"),
    (["--weight-drop", "-0.25"], "--weight-drop"),
    (["--weight-drop", "1.5"], "--weight-drop"),
    (["--weight-drop", "nan"], "--weight-drop"),
    (["--weight-drop", "inf"], "--weight-drop"),
    (["--weight-drop", "0.5x"], "--weight-drop"),
    (["--weight-drop", ""], "--weight-drop"),
    (["--weight-drop"], "--weight-drop"),                                   # no value at all
    (["--weight-drop", "0.5", "--weight-drop-seed", "-1"], "--weight-drop-seed"),
    (["--weight-drop", "0.5", "--weight-drop-seed", "2.5"], "--weight-drop-seed"),
    (["--weight-drop", "0.5", "--weight-drop-seed", "99999999999999999999999"], "--weight-drop-seed"),
    (["--weight-drop-seed", "3"], "--weight-drop-seed"),                    # the seed needs --weight-drop
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


def test_missing_entry_points_refuse_weight_drop_only(stub_exe):
    d, exe, text = stub_exe
    base = [exe, text, "16", "8", "2", "0.1", "--windows", "3", "--sample", "0", "--epochs", "1", "--quiet"]
    log = d / "calls_missing.log"
    out = subprocess.run(base + ["--weight-drop", "0.5"], capture_output=True, text=True,
                         env=dict(os.environ, LSTM_STUB_LOG=str(log)), timeout=60)
    assert out.returncode == 2 and "lstm_hip_set_weight_drop" in out.stderr, (out.returncode, out.stderr)
    assert not log.exists() or log.read_text() == "", log.read_text()
    # without the option the same binary makes the calls it made before
    calls = d / "calls_plain.log"
    out = subprocess.run(base, capture_output=True, text=True, env=dict(os.environ, LSTM_STUB_LOG=str(calls)), timeout=60)
    assert out.returncode == 0, out.stderr
    assert "weight drop" not in out.stdout
    names = [line.split()[2] for line in calls.read_text().splitlines()]
    assert "train_windows" in names and not any("drop" in n for n in names), names


def test_built_program_refuses_a_bad_value_and_names_the_options(tmp_path):
    f = tmp_path / "corpus.txt"
    f.write_bytes(b"the quick brown fox jumps over the lazy dog " * 20)
    out = subprocess.run([LSTM, str(f), "32", "8", "4", "0.1", "--windows", "5", "--sample", "0", "--weight-drop", "1"],
                         capture_output=True, text=True, errors="replace", timeout=60)
    assert out.returncode == 2 and "--weight-drop" in out.stderr, (out.returncode, out.stderr)
    assert "Read " not in out.stdout  # refused while parsing, before the corpus or the device
    out = subprocess.run([LSTM, "--help"], capture_output=True, text=True, timeout=60)
    for opt in ("--weight-drop R", "--weight-drop-seed K"):
        assert opt in out.stdout + out.stderr, opt
