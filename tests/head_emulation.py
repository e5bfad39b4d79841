"""Builds the host emulations of the inference heads (tests/*_head*_emulation.cc) for the test_*_head_emulation_cpu.py modules.
Each program includes tests/device_shim.h and then the files kernels.hip itself includes, eigen-lstm_amd/csrc/heads/*, so what
it runs is the kernel's shipped text."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_dir, name):
    """compile tests/<name>.cc into tmp_dir; the program's path"""
    exe = os.path.join(str(tmp_dir), name)
    subprocess.check_call(["g++", "-O1", "-std=c++20", "-pthread", "-ffp-contract=off",
                           "-I", os.path.join(ROOT, "eigen-lstm_amd", "csrc"), "-I", os.path.join(ROOT, "tests"),
                           os.path.join(ROOT, "tests", name + ".cc"), "-o", exe])
    return exe
