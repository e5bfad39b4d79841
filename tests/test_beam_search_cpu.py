"""CPU: the beam-search references of tests/beam_ref.py -- what the rule implies (one beam is arg-max with the lowest index
on ties, a first selection is the 32 best ranks, hypotheses are distinct and ordered, a finished hypothesis ends in its only
stop byte) on logits full of ties -- and the control of the oracle comparison in tests/test_beam_search.py: on its case the
float64 reference keeps a margin between the last selected and the first rejected candidate that float32 cannot cross.
Also the boundary: the call is declared, exported and listed, and refuses a null handle."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import beam_ref as br
import sampling_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN = os.path.join(ROOT, "eigen-lstm_amd", "lstm_generate")
f32 = np.float32


def _tied_model(seed, levels=9):
    """logits(prefixes) of a toy model: a table row per (position, last byte), few levels (multiples of 1/4), so that most
    logits of a row tie with many others and different parents often give equal costs"""
    T = (np.random.RandomState(seed).randint(0, levels, size=(64, 257, 256)) / 4).astype(f32)

    def logits(prefixes):
        return np.stack([T[len(p), p[-1] if p else 256] for p in prefixes])
    return logits, T


def test_beam_search_is_declared_exported_and_listed():
    import lstm_hip
    lib = lstm_hip.load_library()
    assert hasattr(lib, "lstm_hip_beam_search") and "lstm_hip_beam_search" in lstm_hip.SYMBOLS
    header = open(os.path.join(ROOT, "include", "lstm_hip.h")).read()
    assert re.search(r"int lstm_hip_beam_search\(lstm_hip_t \*h, int32_t streams,", header)
    assert re.search(r"typedef struct lstm_hip_beam \{\s*uint32_t size;[^}]*int32_t\s+beams;[^}]*int32_t\s+stop_byte;", header)
    assert C.sizeof(lstm_hip._Beam) == 12
    assert lstm_hip.coder_version() == 1  # the search moves nothing the coder depends on


def test_beam_search_refuses_a_null_handle_with_a_message():
    import lstm_hip
    lib = lstm_hip.load_library()
    opt = lstm_hip._Beam(C.sizeof(lstm_hip._Beam), 4, -1)
    out, n, bits = (C.c_uint8 * 16)(), (C.c_int32 * 4)(), (C.c_double * 4)()
    rc = lib.lstm_hip_beam_search(None, 1, None, None, None, None, C.byref(opt), 4, out, n, bits, None, None)
    assert rc != 0 and lib.lstm_hip_last_error()


def test_program_refuses_beam_options_that_mean_nothing():
    for args in (["--beams", "0"], ["--beams", "33"], ["--nbest", "2"], ["--beams", "2", "--nbest", "3"],
                 ["--beams", "4", "--temperature", "0.5"], ["--beams", "4", "--top-k", "5"], ["--beams", "8", "--streams", "513"],
                 ["--length-alpha", "0.5"]):
        out = subprocess.run([GEN, "--load", "nowhere", "--count", "5"] + args, capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and "usage: lstm_generate" in out.stderr, (args, out.stderr)


def test_one_beam_is_argmax_with_the_lowest_index_on_ties():
    logits, T = _tied_model(1, levels=4)  # 64 bytes share the largest logit of a row
    res = br.beam32(logits, 1, 30)
    pre, cost = (), 0.0
    for i in range(30):
        z = T[len(pre), pre[-1] if pre else 256]
        assert (z == z.max()).sum() > 1
        x = int(np.argmax(z))  # (the first of the largest)
        assert res["byte"][i] == [x] and res["parent"][i] == [0]
        cost += float(br.surprisal32(z)[x])
        pre += (x,)
    assert res["hyps"] == [bytes(pre)] and res["bits"] == [cost]


def test_a_first_selection_of_32_is_the_32_best_ranks_in_order():
    for seed in (2, 3):
        logits, T = _tied_model(seed)
        res = br.beam32(logits, 32, 1)
        r = sr.ranks(T[0, 256])
        assert [h[0] for h in res["hyps"]] == [int(np.nonzero(r == k)[0][0]) for k in range(32)]
        assert res["parent"][0] == [0] * 32


@pytest.mark.parametrize("W", [1, 4, 32])
def test_hypotheses_are_distinct_and_ordered_and_stop_once(W):
    logits, _ = _tied_model(10 + W)
    free = br.beam32(logits, W, 12)
    stop = free["hyps"][0][4]
    finished = 0
    for s in (-1, stop):
        res = br.beam32(logits, W, 12, s)
        assert len(set(res["hyps"])) == W
        assert all(res["bits"][r] <= res["bits"][r + 1] for r in range(W - 1))
        for hyp, fin, n in zip(res["hyps"], res["fin"], res["length"]):
            assert len(hyp) == n
            if fin:
                assert hyp[-1] == s and s not in hyp[:-1]
                finished += 1
            else:
                assert n == 12 and (s < 0 or s not in hyp)
    assert finished >= 1


def _control_cases(orc):
    """(prompt byte, W, stop byte or -1, beam64's result) of the oracle comparison"""
    N, count, P = br.CONTROL_N, br.CONTROL_COUNT, br.control_params()
    for b in br.CONTROL_PROMPTS:
        for W in br.CONTROL_BEAMS:
            free = br.beam64(orc, N, P, [b], W, count)
            yield b, W, -1, free
            stop = free["hyps"][0][br.CONTROL_STOP_AT]
            yield b, W, stop, br.beam64(orc, N, P, [b], W, count, stop)


def test_control_of_the_oracle_comparison(oracle64, oracle32):
    """The float64 reference separates the W-th from the (W+1)-th candidate by at least 5e-5 bits at every selection of every
    case (measured: 1.16e-4), and the float32 restatement -- the oracle's float32 recurrence with the device's selection
    arithmetic -- finds the same hypotheses with costs within 1e-4 bits (measured: 1.0e-5), so the GPU test skips nothing."""
    N, count, P = br.CONTROL_N, br.CONTROL_COUNT, br.control_params()
    smallest, worst, stopped = br.INF, 0.0, 0
    for b, W, stop, ref in _control_cases(oracle64):
        smallest = min(smallest, ref["margin"])
        low = br.beam32_oracle(oracle32, N, P, [b], W, count, stop)
        assert low["hyps"] == ref["hyps"] and low["length"] == ref["length"], (b, W, stop)
        worst = max(worst, np.abs(np.array(low["bits"]) - np.array(ref["bits"])).max())
        if stop >= 0:
            assert any(ref["fin"]), (b, W)
            stopped += 1
    print("smallest margin %.3g bits, largest float32 - float64 cost difference %.3g bits" % (smallest, worst))
    assert stopped == 12
    assert smallest >= 5e-5, smallest
    assert worst <= 1e-4, worst
