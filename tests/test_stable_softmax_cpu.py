"""CPU: LSTM_HIP_STABLE_SOFTMAX at the boundary -- its bit, and the programs' --stable-softmax option (accepted: they get past
argument parsing to the device check)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSTM = os.path.join(ROOT, "eigen-lstm_amd", "lstm")
GEN = os.path.join(ROOT, "eigen-lstm_amd", "lstm_generate")


def _has_gpu():
    try:
        import torch
        return torch.cuda.device_count() > 0
    except Exception:
        return False


def test_flag_value_matches_the_header_and_is_a_free_bit():
    import lstm_hip
    header = open(os.path.join(ROOT, "include", "lstm_hip.h")).read()
    m = re.search(r"#define LSTM_HIP_STABLE_SOFTMAX (\d+)u", header)
    assert m and int(m.group(1)) == lstm_hip.STABLE_SOFTMAX == 512
    assert lstm_hip.STABLE_SOFTMAX & (2 | 8 | 32 | lstm_hip.FAST_MATH | lstm_hip.STEP_KERNELS | lstm_hip.DEBUG_STAMPS |
                                      lstm_hip.NO_FUSED_GRADS | lstm_hip.BF16_RECURRENCE | lstm_hip.PAD_HIDDEN) == 0


@pytest.mark.skipif(_has_gpu(), reason="checks that the option is parsed on a machine without a GPU")
def test_training_program_accepts_the_option(tmp_path):
    f = tmp_path / "corpus.txt"
    f.write_bytes(b"the quick brown fox jumps over the lazy dog " * 20)
    out = subprocess.run([LSTM, str(f), "32", "8", "4", "0.1", "--windows", "5", "--sample", "0", "--stable-softmax"],
                         capture_output=True, text=True, errors="replace", timeout=60)
    assert "unknown option" not in out.stderr, out.stderr
    assert out.returncode != 0 and "device" in (out.stdout + out.stderr).lower(), (out.returncode, out.stdout, out.stderr)


@pytest.mark.skipif(_has_gpu(), reason="checks that the option is parsed on a machine without a GPU")
def test_generate_program_accepts_the_option(tmp_path):
    N = 16
    for name, rows, cols in (("W", 4 * N, 256), ("U", 4 * N, N), ("b", 4 * N, 1), ("Why", 256, N), ("by", 256, 1)):
        (tmp_path / f"ck_{name}.txt").write_text("\n".join(" ".join(["0"] * cols) for _ in range(rows)) + "\n")
    f = tmp_path / "t.txt"
    f.write_bytes(b"hello world")
    out = subprocess.run([GEN, "--load", str(tmp_path / "ck"), "--score", str(f), "--stable-softmax"],
                         capture_output=True, text=True, errors="replace", timeout=60)
    assert "unknown argument" not in out.stderr and "usage:" not in out.stderr, out.stderr
    assert out.returncode != 0 and "device" in (out.stdout + out.stderr).lower(), (out.returncode, out.stdout, out.stderr)


def test_usage_text_names_the_option():
    for prog in (LSTM, GEN):
        out = subprocess.run([prog, "--help"], capture_output=True, text=True, timeout=60)
        assert "--stable-softmax" in out.stdout + out.stderr, prog
