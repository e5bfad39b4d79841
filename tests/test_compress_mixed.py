"""-m gpu: lstm_compress --guide -- files coded on a mix of checkpoints (lstm_hip_encode_mixed / lstm_hip_decode_mixed, DESIGN.md
section 3.25), beside tests/test_compress.py: a 2 KB file round-trips with fixed and with learned weights; the LHAM container's
fields are the ones the program documents and its codes are Lstm.encode_mixed's; -d with the guides swapped names the model
whose parameters differ and writes nothing; -d refuses weights and a rate of its own; each container kind is told from the
others; and without --guide the program writes the LHAC file it always wrote, byte for byte."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "eigen-lstm_amd", "lstm_compress")
M = 256


def _write_checkpoint(prefix, N, seed):
    """the five-file text checkpoint (host/checkpoint.h) of a random model; returns the flat block"""
    rs = np.random.RandomState(seed)
    parts = []
    for name, r, c, scale in (("W", 4 * N, M, 0.2), ("U", 4 * N, N, 0.2), ("b", 4 * N, 1, 0.2), ("Why", M, N, 1.0), ("by", M, 1, 1.0)):
        a = (rs.randn(r, c) * scale).astype(np.float32)
        np.savetxt(f"{prefix}_{name}.txt", a, fmt="%.9g")
        parts.append(a.ravel(order="F"))
    return np.concatenate(parts)


def _fnv1a(P):
    h = 0xCBF29CE484222325
    for b in np.asarray(P, np.float32).tobytes():
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def _run(*args):
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300)


def _handle(N, P):
    import lstm_hip
    L = lstm_hip.Lstm(N, 2, 1, flags=lstm_hip.PAD_HIDDEN)
    L.set_params(P)
    return L


def test_program_codes_with_guides(tmp_path):
    import lstm_hip
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    Pa, Pb = _write_checkpoint(a, 24, seed=1), _write_checkpoint(b, 16, seed=2)
    src = tmp_path / "in.bin"
    text = bytes(np.random.RandomState(3).randint(97, 123, size=2048).astype(np.uint8))
    src.write_bytes(text)
    packed, back = tmp_path / "x.lham", tmp_path / "x.out"
    La, Lb = _handle(24, Pa), _handle(16, Pb)
    f32bits = lambda x: struct.unpack("<I", struct.pack("<f", x))[0]
    for extra, weights, rate in (([], (0.5, 0.5), 0.0), (["--guide-weight", "0.3", "--main-weight", "0.9", "--mix-rate", "0.01"], (0.9, 0.3), 0.01)):
        out = _run("--load", a, "--guide", b, *extra, "-c", str(src), str(packed))
        assert out.returncode == 0, out.stderr
        codes, bits = La.encode_mixed([text], guides=[(Lb, weights[1])], main_weight=weights[0], rate=rate)
        head = struct.pack("<IIIII", 0x4D41484C, 1, lstm_hip.coder_version(), lstm_hip.mix_coder_version(), 2)
        head += struct.pack("<IIQ", 24, 0, _fnv1a(Pa)) + struct.pack("<IIQ", 16, 0, _fnv1a(Pb))
        head += struct.pack("<III", f32bits(weights[0]), f32bits(weights[1]), f32bits(rate))
        head += struct.pack("<QII", len(text), 1, zlib.crc32(text)) + struct.pack("<Q", len(codes[0]))
        assert packed.read_bytes() == head + codes[0], extra
        assert f"code {len(codes[0])} bytes in 1 streams, 2 models" in out.stdout, out.stdout
        assert ("final" in out.stdout) == (rate > 0), out.stdout
        out = _run("--load", a, "--guide", b, "-d", str(packed), str(back))
        assert out.returncode == 0, out.stderr
        assert back.read_bytes() == text
        back.unlink()
    # the guides swapped: the first model that differs is named, nothing is written
    out = _run("--load", b, "--guide", a, "-d", str(packed), str(back))
    assert out.returncode == 1 and "model 0 was coded with a hidden size of 24, the --load model" in out.stderr and b in out.stderr, out.stderr
    assert not back.exists()
    c = str(tmp_path / "c")
    _write_checkpoint(c, 16, seed=4)
    out = _run("--load", a, "--guide", c, "-d", str(packed), str(back))
    assert out.returncode == 1 and f"model 1 was coded with other parameters than guide 1 ({c}) (parameter hash differs)" in out.stderr, out.stderr
    assert not back.exists()
    out = _run("--load", a, "--guide", b, "--guide", c, "-d", str(packed), str(back))
    assert out.returncode == 1 and "coded with 1 guides, 2 given with --guide" in out.stderr, out.stderr
    # -d reads weights and rate from the container
    for opt in ("--guide-weight", "--main-weight", "--mix-rate"):
        out = _run("--load", a, "--guide", b, opt, "0.25", "-d", str(packed), str(back))
        assert out.returncode == 2 and f"{opt} is read from the container with -d" in out.stderr, out.stderr
    out = _run("--load", a, "--mix-rate", "0.1", "-c", str(src), str(packed))
    assert out.returncode == 2 and "--mix-rate needs --guide" in out.stderr, out.stderr
    # each kind names the other
    out = _run("--load", a, "-d", str(packed), str(back))
    assert out.returncode == 1 and "a mixed lstm_compress file (LHAM): decode it with --load PREFIX --guide PREFIX2 -d" in out.stderr, out.stderr
    out = _run("--adapt", "-d", str(packed), str(back))
    assert out.returncode == 1 and "a mixed lstm_compress file (LHAM)" in out.stderr, out.stderr
    # without --guide: the LHAC container, byte for byte what the unmixed call gives
    plain = tmp_path / "x.lhac"
    out = _run("--load", a, "-c", str(src), str(plain))
    assert out.returncode == 0, out.stderr
    codes, _ = La.encode([text])
    head = struct.pack("<IIIIIQQII", 0x4341484C, 1, lstm_hip.coder_version(), 24, 0, _fnv1a(Pa), len(text), 1, zlib.crc32(text))
    assert plain.read_bytes() == head + struct.pack("<Q", len(codes[0])) + codes[0]
    out = _run("--load", a, "--guide", b, "-d", str(plain), str(back))
    assert out.returncode == 1 and "a static lstm_compress file (LHAC), coded without guides: decode it without --guide" in out.stderr, out.stderr
    out = _run("--load", a, "-d", str(plain), str(back))
    assert out.returncode == 0 and back.read_bytes() == text, out.stderr
    assert not any(p.name.endswith(".tmp") for p in tmp_path.iterdir())
    La.close()
    Lb.close()
