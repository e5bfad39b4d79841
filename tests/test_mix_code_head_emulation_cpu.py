"""CPU: the logic of the mixed coder's two launches per step -- k_guide_logits in coder mode and k_code_head's MIX instantiation
(eigen-lstm_amd/csrc/heads/guide_logits.inc, code_head.inc) -- run on the host: the kernels' own text
compiled with one thread per work-item (tests/mix_code_head_emulation.cc), against tests/mix_coder_ref.py, bit for bit: the
trace row of every coded byte (so cum, freq and T of the table built on the mix), the weights every byte was coded under, the
weights after every stream's last byte, the codes and every sentinel around them, the bits, the inputs handed to the
recurrences, the guides' logits of every step and the rows the guide kernel must leave alone; then the decoder on the
emulated encoder's codes.  Parameters and states are multiples of 1/16, so every model's logits are exact; the weights are not
dyadic, so every multiply and add of the mix and of the update rounds.  expf and log2 are the C library's on both sides.
The MIX = false instantiation, run on the same inputs, must write what tests/code_head_emulation.cc writes."""
import ctypes
import subprocess

import numpy as np
import pytest

import head_emulation
import mix_coder_ref as mr

f32 = np.float32
M = 256
N = 16
GN = (16, 32)  # the guides' widths
SENTINEL = 0xA5
FRONT, TAIL = 5, 7

_libm = ctypes.CDLL("libm.so.6")
_libm.log2.restype, _libm.log2.argtypes = ctypes.c_double, [ctypes.c_double]


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    return head_emulation.build(tmp_path_factory.mktemp("mix_code_head"), "mix_code_head_emulation")


@pytest.fixture(scope="module")
def unmixed_emulator(tmp_path_factory):
    return head_emulation.build(tmp_path_factory.mktemp("code_head_for_mix"), "code_head_emulation")


def _logits(Why, by, h):
    """sequentially in k, separate multiply and add, by last (exact here)"""
    y = np.zeros(M, f32)
    for k in range(Why.shape[0]):
        y = (y + (Why[k] * h[k]).astype(f32)).astype(f32)
    return (y + by).astype(f32)


def _model(rs, n, steps, K, why_scale):
    Why = (rs.randint(-why_scale, why_scale + 1, size=(n, 256)) / 16).astype(f32)  # [k][m]
    by = (rs.randint(-16, 17, size=256) / 16).astype(f32)
    Hs = (rs.randint(-16, 17, size=(steps + 1, K, n)) / 16).astype(f32)  # the state before each step: any will do
    return Why, by, Hs


def _bound(n):
    return 3 * n + 4 if n else 0


def _write(d, **arrays):
    for name, arr in arrays.items():
        np.ascontiguousarray(arr).tofile(f"{d}/{name}.bin")


def _run(exe, d, K, steps, sb, decode, mix, G, rate, total):
    subprocess.check_call([exe, d, str(N), str(K), str(steps), str(sb), str(int(decode)), str(int(mix)), str(G), repr(float(rate))],
                          timeout=600)
    return dict(code=np.fromfile(f"{d}/code_out.bin", np.uint8), text=np.fromfile(f"{d}/text_out.bin", np.uint8),
                trace=np.fromfile(f"{d}/trace.bin", np.uint32).reshape(total + 1, 3), bits=np.fromfile(f"{d}/bits.bin", np.float64),
                code_len=np.fromfile(f"{d}/code_len.bin", np.uint64), xlog=np.fromfile(f"{d}/xlog.bin", np.int32).reshape(steps + 1, K),
                err=int(np.fromfile(f"{d}/err.bin", np.uint32)[0]),
                w_trace=np.fromfile(f"{d}/w_trace.bin", f32).reshape(total + 1, 1 + G),
                w_out=np.fromfile(f"{d}/w_out.bin", f32).reshape(K, 1 + G),
                zklog=np.fromfile(f"{d}/zklog.bin", f32).reshape(steps + 1, K, G, M))


# (streams, SB, lengths, weights (v_0, v_1, ..), rate, seed): lengths 0, 1 and longer, one stream ending before the others
CASES = {
    "sb1_one_guide_fixed": (5, 1, [0, 1, 6, 3, 9], (0.7, 0.3), 0.0, 1),
    "sb1_two_guides_learned": (5, 1, [4, 0, 1, 7, 2], (0.7, 0.3, -0.2), 0.011, 2),
    "sb2_three_guides_learned": (7, 2, [2, 0, 1, 5, 3, 0, 8], (0.3, 0.9, -0.7, 1.1), 0.013, 3),
    "sb2_one_guide_learned": (6, 2, [1, 0, 2, 0, 1, 5], (1.3, -0.35), 0.007, 4),
    "sb2_two_guides_fixed": (3, 2, [3, 4, 1], (0.45, 0.35, 0.2), 0.0, 5),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_emulated_mixed_coder_matches_the_reference(emulator, unmixed_emulator, tmp_path, name):
    K, sb, lengths, v0, rate, seed = CASES[name]
    rs = np.random.RandomState(seed)
    d = str(tmp_path)
    G = len(v0) - 1
    steps = max(lengths)
    main = _model(rs, N, steps, K, 32)
    guides = [_model(rs, GN[k % 2], steps, K, 16) for k in range(G)]
    texts = [rs.randint(0, 256, size=n).astype(np.uint8) for n in lengths]
    text_off = np.zeros(K + 1, np.uint64)
    text_off[1:] = np.cumsum(lengths)
    total = int(text_off[-1])
    caps = [_bound(n) for n in lengths]
    code_base = (FRONT + np.concatenate([[0], np.cumsum(caps)])).astype(np.uint64)
    code0 = np.full(int(code_base[-1]) + TAIL, SENTINEL, np.uint8)
    text = np.concatenate(texts + [np.zeros(1, np.uint8)])
    vs = np.tile(np.array(v0, f32), (K, 1))
    _write(d, why=main[0], by=main[1], hs=main[2], text_off=text_off, text=text, code=code0, code_base=code_base,
           gn=np.array([g[0].shape[0] for g in guides], np.int32), v0=vs)
    for k, g in enumerate(guides):
        _write(d, **{f"g{k}_why": g[0], f"g{k}_by": g[1], f"g{k}_hs": g[2]})
    got = _run(emulator, d, K, steps, sb, False, True, G, rate, total)
    assert got["err"] == 0

    def members(s):
        return lambda j: [_logits(main[0], main[1], main[2][j, s])] + [_logits(g[0], g[1], g[2][j, s]) for g in guides]

    want_code = code0.copy()
    codes, w_outs, moved = [], [], 0
    for s in range(K):
        L, o = lengths[s], int(text_off[s])
        code, trace, w_trace, w_out, _ = mr.encode(texts[s], members(s), v0, rate)
        codes.append(code)
        w_outs.append(w_out)
        assert np.array_equal(got["trace"][o:o + L], trace), (name, s)
        assert got["w_trace"][o:o + L].tobytes() == w_trace.tobytes(), (name, s)
        assert got["w_out"][s].tobytes() == w_out.tobytes(), (name, s)
        if L:
            assert got["w_trace"][o].tobytes() == np.array(v0, f32).tobytes()
        moved += L > 1 and w_trace[-1].tobytes() != w_trace[0].tobytes()
        beg = int(code_base[s])
        want_code[beg:beg + len(code)] = np.frombuffer(code, np.uint8)
        assert int(got["code_len"][s]) == len(code) <= caps[s], (name, s)
        assert list(got["xlog"][:, s]) == [int(b) for b in texts[s]] + [-1] * (steps + 1 - L), (name, s)
        bits = 0.0
        for _, freq, T in trace:
            bits += -_libm.log2(int(freq) / int(T))
        assert got["bits"][s] == bits, (name, s)
        for t in range(steps + 1):
            if t < L:
                for k, z in enumerate(members(s)(t)[1:]):
                    assert got["zklog"][t, s, k].tobytes() == z.tobytes(), (name, s, t, k)
            else:
                assert (got["zklog"][t, s] == -7).all(), (name, s, t)  # an ended stream's rows are not written
    assert np.array_equal(got["code"], want_code)  # every code, and every sentinel outside the codes
    assert np.array_equal(got["text"], text) and not got["trace"][-1].any() and not got["w_trace"][-1].any()
    assert (moved > 0) == (rate > 0), (name, moved)  # learning moves the weights, rate 0 never does

    # the decoder on the emulated encoder's codes, back to back
    code = np.frombuffer(b"".join(codes) + b"\xff", np.uint8)
    base = np.concatenate([[0], np.cumsum([len(c) for c in codes])]).astype(np.uint64)
    _write(d, text=np.full(total + 1, SENTINEL, np.uint8), code=code, code_base=base, v0=vs)
    dec = _run(emulator, d, K, steps, sb, True, True, G, rate, total)
    assert dec["err"] == 0
    assert np.array_equal(dec["text"][:total], text[:total]) and dec["text"][total] == SENTINEL
    assert np.array_equal(dec["xlog"], got["xlog"])
    for s in range(K):
        assert dec["w_out"][s].tobytes() == w_outs[s].tobytes(), (name, s)
        back, w_dec = mr.decode(codes[s], lengths[s], members(s), v0, rate)
        assert back == texts[s].tobytes() and w_dec.tobytes() == w_outs[s].tobytes(), (name, s)

    # MIX = false on the same inputs: the unmixed emulation's bytes
    _write(d, text=text, code=code0, code_base=code_base, v0=vs)
    plain = _run(emulator, d, K, steps, sb, False, False, G, rate, total)
    subprocess.check_call([unmixed_emulator, d, str(N), str(K), str(steps), str(sb), "0"], timeout=600)
    for out in ("code_out", "text_out", "trace", "bits", "code_len", "xlog", "err"):
        assert open(f"{d}/{out}.bin", "rb").read() == {"code_out": plain["code"], "text_out": plain["text"], "trace": plain["trace"],
                                                      "bits": plain["bits"], "code_len": plain["code_len"], "xlog": plain["xlog"],
                                                      "err": np.array([plain["err"]], np.uint32)}[out].tobytes(), (name, out)
    assert plain["w_out"].tobytes() == vs.tobytes() and (plain["zklog"] == -7).all() and not plain["w_trace"].any()
    assert not np.array_equal(plain["trace"], got["trace"]) or total == 0  # (the guides do change the tables)
