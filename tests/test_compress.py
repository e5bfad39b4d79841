"""-m gpu: lstm_hip_encode / lstm_hip_decode -- arithmetic coding of bytes with the model (include/lstm_hip.h, DESIGN.md
section 3.6).  Codes must come back bit-exact, match the model's predicted size, not depend on the batch, the flags that
do not change the model, or anything of the handle but its parameters; and the device coder must be exactly the Python
copy in tests/range_coder_ref.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gpu_util as gu
import range_coder_ref as rc
from test_pad_hidden import pad_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "eigen-lstm_amd")
M = 256


def _params(N, seed, scale=0.3):
    return gu.random_case(N, 2, 1, seed=seed, scale=scale)[0]


def _texts(streams, seed, max_len):
    """ragged streams: empty and one-byte ones, every byte value, long runs of one byte, random bytes"""
    rs = np.random.RandomState(seed)
    out = []
    for s in range(streams):
        kind = s % 6
        if kind == 0:
            out.append(b"")
        elif kind == 1:
            out.append(bytes([int(rs.randint(256))]))
        elif kind == 2:
            out.append(bytes(rs.permutation(256).astype(np.uint8))[:max_len])
        elif kind == 3:
            out.append(bytes([int(rs.randint(256))]) * int(rs.randint(2, max_len + 1)))
        else:
            out.append(bytes(rs.randint(0, 256, size=int(rs.randint(2, max_len + 1))).astype(np.uint8)))
    if streams == 1:
        out = [bytes(range(256)) + b"a" * 40 + bytes(rs.randint(0, 256, size=30).astype(np.uint8))]
    return out


def _handle(N, P, flags=0, B=1):
    import lstm_hip
    L = lstm_hip.Lstm(N, 2, B, flags=flags)
    L.set_params(P)
    return L


@pytest.mark.parametrize("streams", [1, 3, 64, 513, 4096])
@pytest.mark.parametrize("N", [32, 128, 192, 512, 1024, 1040])   # (192, 1040: no persistent recurrence at these widths)
def test_round_trip_is_bit_exact(N, streams):
    import lstm_hip
    P = _params(N, seed=N + streams)
    max_len = {1: 326, 3: 300, 64: 200, 513: 60, 4096: 24}[streams]
    texts = _texts(streams, seed=streams, max_len=max_len)
    L = _handle(N, P)
    codes, bits = L.encode(texts)
    assert len(codes) == streams and bits.shape == (streams,)
    for t, c in zip(texts, codes):
        assert len(c) <= lstm_hip.code_bound(len(t))
        assert (len(c) == 0) == (len(t) == 0)
    back = L.decode(codes, [len(t) for t in texts])
    L.close()
    assert back == texts


@pytest.mark.parametrize("N", [32, 512])
def test_text_the_model_finds_very_unlikely(N):
    """a model sure of byte 0 and text of every other byte: every coded byte sits at the minimum frequency 1"""
    import lstm_hip
    P = _params(N, seed=9, scale=0.01)
    P[-M:] = 0.0
    P[-M] = 40.0  # by: p(0) ~ 1 - 255 e^-40 whatever h is
    rs = np.random.RandomState(10)
    texts = [bytes(rs.randint(1, 256, size=n).astype(np.uint8)) for n in (1, 50, 400)]
    L = _handle(N, P)
    codes, bits, tr = L.encode(texts, trace=True)
    assert (tr[:, 1] == 1).all() and (tr[:, 2] == 256 + 65024).all(), (tr[:, 1].max(), np.unique(tr[:, 2]))
    for t, c in zip(texts, codes):
        assert len(c) <= lstm_hip.code_bound(len(t))
    assert L.decode(codes, [len(t) for t in texts]) == texts
    L.close()


def test_size_matches_the_model_on_fixture_a():
    """fixture A (the reference's N = 32 enwik5 model, 3.24396 bits/char on its text slice)"""
    fx = np.load(os.path.join(ROOT, "tests", "golden", "fixture_A.npz"))
    N, P, text = int(fx["N"]), fx["params"], fx["text"]
    L = _handle(N, P)
    codes, bits, tr = L.encode([text], trace=True)
    _, gbits, _, _ = L.generate([text], score=True)
    back = L.decode(codes, [text.size])
    L.close()
    assert back[0] == text.tobytes()
    per = -np.log2(tr[:, 1].astype(np.float64) / tr[:, 2])
    assert abs(per.sum() - bits[0]) <= 1e-9 * max(1.0, bits[0])
    n = text.size
    assert abs(per[1:].sum() / (n - 1) - gbits[0] / (n - 1)) <= 0.01, (per[1:].sum() / (n - 1), gbits[0] / (n - 1))
    assert abs(per[1:].sum() / (n - 1) - float(fx["expected_bits"])) <= 0.01
    by = P[-M:].astype(np.float64)
    p0 = np.exp(by - by.max()) / np.exp(by - by.max()).sum()
    assert abs(per[0] + np.log2(p0[text[0]])) <= 0.01, (per[0], -np.log2(p0[text[0]]))
    # the code is the ideal length plus the flush allowance (32 bits) and the coder's rounding (<= 0.01 bit per byte)
    assert 8 * len(codes[0]) <= bits[0] + 32 + 0.01 * n, (8 * len(codes[0]), bits[0])


def test_a_stream_codes_the_same_alone_or_anywhere_in_any_batch():
    """streams 1, 513, 1024, 2048 and 4096 put 1, 2, 4, 8 and 16 streams in a workgroup of code_head (gen_head_group)"""
    N = 128
    P = _params(N, seed=21)
    rs = np.random.RandomState(22)
    pool = [bytes(rs.randint(0, 256, size=int(rs.randint(0, 24))).astype(np.uint8)) for _ in range(4096)]
    target = bytes(rs.randint(0, 256, size=23).astype(np.uint8))
    L = _handle(N, P)
    alone = L.encode([target])[0][0]
    for size in (513, 1024, 2048, 4096):
        for pos in (0, 1, 7, 15, size - 1):
            texts = list(pool[:size])
            texts[pos] = target
            codes, _ = L.encode(texts)
            assert codes[pos] == alone, (size, pos)
    # and every other stream of the full batch is its own single-stream code (a sample: every workgroup slot)
    codes, _ = L.encode(pool)
    for s in list(range(16)) + list(range(4080, 4096)):
        assert codes[s] == L.encode([pool[s]])[0][0], s
    L.close()


def test_stable_softmax_flag_and_bf16_handles_give_the_same_code():
    import lstm_hip
    N = 256
    P = _params(N, seed=31)
    texts = _texts(40, seed=32, max_len=120)
    L = _handle(N, P)
    ref, _ = L.encode(texts)
    L.close()
    for flags in (lstm_hip.STABLE_SOFTMAX, lstm_hip.BF16_RECURRENCE, lstm_hip.BF16_RECURRENCE | lstm_hip.STABLE_SOFTMAX):
        L = _handle(N, P, flags=flags, B=8)
        got, _ = L.encode(texts)
        assert got == ref, flags
        assert L.decode(got, [len(t) for t in texts]) == texts
        L.close()


def test_padded_handle_codes_as_the_explicit_padded_model():
    import lstm_hip
    N, Np = 500, 512
    P = _params(N, seed=41)
    texts = _texts(30, seed=42, max_len=150)
    L = _handle(N, P, flags=lstm_hip.PAD_HIDDEN)
    got, bits = L.encode(texts)
    assert L.decode(got, [len(t) for t in texts]) == texts
    L.close()
    E = _handle(Np, pad_params(P, N, Np))
    want, wbits = E.encode(texts)
    E.close()
    assert got == want
    assert np.array_equal(bits, wbits)


def test_fast_math_round_trips():
    import lstm_hip
    N = 128
    P = _params(N, seed=51)
    texts = _texts(20, seed=52, max_len=200)
    L = _handle(N, P, flags=lstm_hip.FAST_MATH)
    codes, _ = L.encode(texts)
    assert L.decode(codes, [len(t) for t in texts]) == texts
    L.close()


def test_device_coder_is_the_python_coder():
    N = 64
    P = _params(N, seed=61)
    texts = _texts(12, seed=62, max_len=300)
    L = _handle(N, P)
    codes, bits, tr = L.encode(texts, trace=True)
    L.close()
    assert tr.shape == (sum(len(t) for t in texts), 3)
    assert (tr[:, 1] >= 1).all() and (tr[:, 2] >= 256).all() and (tr[:, 2] <= 256 + 65025).all()
    assert (tr[:, 0] + tr[:, 1] <= tr[:, 2]).all()
    o = 0
    for s, t in enumerate(texts):
        rows = tr[o:o + len(t)]
        o += len(t)
        assert rc.encode(rows) == codes[s], s
        assert bytes(rc.decode(codes[s], len(t), rc.trace_model(rows, t))) == t
        assert abs(bits[s] - float(-np.log2(rows[:, 1].astype(np.float64) / rows[:, 2]).sum())) <= 1e-9 * max(1.0, bits[s])


def test_truncated_codes_decode_to_their_length_and_leave_the_neighbours_alone():
    N = 64
    P = _params(N, seed=71)
    rs = np.random.RandomState(72)
    texts = [bytes(rs.randint(0, 256, size=n).astype(np.uint8)) for n in (80, 120, 90)]
    L = _handle(N, P)
    codes, _ = L.encode(texts)
    lengths = [len(t) for t in texts]
    for cut in (0, 1, 3, len(codes[1]) // 2, len(codes[1]) - 1):
        back = L.decode([codes[0], codes[1][:cut], codes[2]], lengths)
        assert [len(b) for b in back] == lengths
        assert back[0] == texts[0] and back[2] == texts[2], cut
    # an exact code followed by junk is still the stream's code (its bytes are all read first)
    assert L.decode([codes[0]], [lengths[0]]) == [texts[0]]
    L.close()


def test_handle_state_is_untouched():
    import lstm_hip
    N, S, B = 64, 8, 4
    P = _params(N, seed=81, scale=0.1)
    L = lstm_hip.Lstm(N, S, B)
    L.set_params(P)
    text = np.frombuffer(b"the quick brown fox jumps over the lazy dog " * 40, np.uint8)
    L.set_text(text)
    L.set_cursors(lstm_hip.initial_cursors(text.size, S, B))
    L.reset_window()
    L.set_optimizer(lstm_hip.OPT_ADAM)
    L.set_grad_clip(5.0)
    L.set_loss_mode(lstm_hip.LOSS_LAST_STEP_BITS)
    losses = L.train_windows(3, 0.01)

    def snap():
        xi, ti = L.get_window()
        out = [L.get_params(w) for w in (0, 1, 2, 3)] + [xi, ti, L.get_cursors(), np.array([L.optimizer_steps()]),
                                                        L.grad_norms()]
        for t in range(S):
            out += list(L.get_state(t))
        return out

    before = snap()
    codes, _ = L.encode([b"hello world", b"", b"xyz" * 50])
    assert L.decode(codes, [11, 0, 150]) == [b"hello world", b"", b"xyz" * 50]
    after = snap()
    for i, (a, b) in enumerate(zip(before, after)):
        assert np.array_equal(a, b), i
    # the loss mode and the clip setting are still in force: the next windows report last-step losses, clipped steps
    more = L.train_windows(2, 0.01)
    assert more.shape == (2,) and np.isfinite(more).all() and np.isfinite(losses).all()
    assert L.grad_norms().shape == (2,)
    L.close()


def test_arguments_are_checked():
    import lstm_hip
    L = _handle(32, _params(32, seed=91))
    lib, h = L.lib, L._h
    text = (C.c_uint8 * 8)(*range(8))
    code = (C.c_uint8 * 64)()
    code_off = (C.c_uint64 * 3)()

    def off(*v):
        return (C.c_uint64 * len(v))(*v)

    def enc(streams, t, toff, cd, cap, coff):
        return lib.lstm_hip_encode(h, streams, t, toff, cd, C.c_uint64(cap), coff, None, None)

    cases = {
        "streams 0": enc(0, text, off(0, 8), code, 64, code_off),
        "streams 4097": enc(4097, text, off(0, 8), code, 64, code_off),
        "offsets not from 0": enc(1, text, off(1, 8), code, 64, code_off),
        "offsets decrease": enc(2, text, off(0, 5, 3), code, 64, code_off),
        "null offsets": enc(1, text, None, code, 64, code_off),
        "null text": enc(1, None, off(0, 8), code, 64, code_off),
        "null code": enc(1, text, off(0, 8), None, 64, code_off),
        "null code_off": enc(1, text, off(0, 8), code, 64, None),
        "cap below bound": enc(2, text, off(0, 4, 8), code, 2 * (3 * 4 + 4) - 1, code_off),
        "decode streams 0": lib.lstm_hip_decode(h, 0, code, off(0, 4), off(0, 8), text),
        "decode streams 4097": lib.lstm_hip_decode(h, 4097, code, off(0, 4), off(0, 8), text),
        "decode null code": lib.lstm_hip_decode(h, 1, None, off(0, 4), off(0, 8), text),
        "decode null text": lib.lstm_hip_decode(h, 1, code, off(0, 4), off(0, 8), None),
        "decode code_off not from 0": lib.lstm_hip_decode(h, 1, code, off(2, 4), off(0, 8), text),
        "decode code_off decreases": lib.lstm_hip_decode(h, 2, code, off(0, 4, 2), off(0, 4, 8), text),
        "decode text_off decreases": lib.lstm_hip_decode(h, 2, code, off(0, 4, 8), off(0, 6, 2), text),
        "decode null offsets": lib.lstm_hip_decode(h, 1, code, None, off(0, 8), text),
    }
    for name, got in cases.items():
        assert got == lstm_hip.EINVAL, (name, got)
    assert enc(2, text, off(0, 4, 8), code, 2 * (3 * 4 + 4) - 1, code_off) == lstm_hip.EINVAL
    assert b"code_cap" in lib.lstm_hip_last_error()
    assert enc(2, text, off(0, 4, 8), code, 2 * (3 * 4 + 4), code_off) == 0  # exactly the bound is enough
    assert enc(1, None, off(0, 0), None, 0, code_off) == 0  # nothing to code: no buffers due
    L.close()


def test_code_head_shows_in_the_kernel_stats():
    L = _handle(64, _params(64, seed=95))
    L.set_profiling(True)
    L.reset_kernel_stats()
    L.encode([b"abcdefgh" * 4, b"xy"])
    st = L.kernel_stats()
    L.close()
    assert st["code_head"][0] == 32 and st["fwd_step"][0] == 31, st


# ---- the program ---------------------------------------------------------------------------------------------------------
def _corpus(n, seed):
    rs = np.random.RandomState(seed)
    words = [bytes(rs.randint(97, 123, size=rs.randint(2, 8)).astype(np.uint8)) for _ in range(80)]
    return b" ".join(words[i] for i in rs.randint(0, 80, size=n))[:n]


def _train(tmp_path, name, seed):
    corpus = tmp_path / f"{name}.txt"
    corpus.write_bytes(_corpus(20000, seed=seed))
    out = subprocess.run([os.path.join(PKG, "lstm"), str(corpus), "64", "16", "8", "0.1", "--epochs", "1", "--windows", "300",
                          "--seed", str(seed), "--sample", "0", "--save", str(tmp_path / name), "--quiet"],
                         capture_output=True, text=True, errors="replace", timeout=300)
    assert out.returncode == 0, out.stderr
    return str(tmp_path / name)


def test_program_round_trips_a_file_and_refuses_another_checkpoint(tmp_path):
    ck = _train(tmp_path, "ck", seed=1)
    other = _train(tmp_path, "other", seed=2)
    src = tmp_path / "held_out.txt"
    src.write_bytes(_corpus(30000, seed=3))
    exe = os.path.join(PKG, "lstm_compress")
    packed, back = tmp_path / "x.lhac", tmp_path / "x.out"
    for extra in ([], ["--streams", "7"], ["--streams", "4096"], ["--fast-math"]):
        out = subprocess.run([exe, "--load", ck, "-c", str(src), str(packed)] + extra, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        m = re.fullmatch(r"in (\d+) bytes, out (\d+) bytes, code (\d+) bytes in (\d+) streams: ([\d.]+) bits/char "
                         r"\(model ([\d.]+) bits/char\)\n", out.stdout)
        assert m, out.stdout
        n_in, n_out, n_code, k = (int(m.group(i)) for i in range(1, 5))
        assert n_in == src.stat().st_size and n_out == packed.stat().st_size
        assert n_out == 44 + 8 * k + n_code
        assert abs(float(m.group(5)) - 8 * n_code / n_in) <= 1e-4
        # the code is the model's ideal length plus 32 flush bits per stream and the coder's rounding (<= 0.01 bit per byte)
        assert float(m.group(6)) <= float(m.group(5)) <= float(m.group(6)) + 0.01 + 32.0 * k / n_in + 1e-5, out.stdout
        if not extra:  # the default split of a 30 KB file: one stream, and a trained model below 8 bits/char
            assert k == 1 and float(m.group(6)) < 7.0, out.stdout
        out = subprocess.run([exe, "--load", ck, "-d", str(packed), str(back)], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        assert subprocess.run(["cmp", str(src), str(back)]).returncode == 0, extra
        back.unlink()
    out = subprocess.run([exe, "--load", other, "-d", str(packed), str(back)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 1 and "parameter hash" in out.stderr, out.stderr
    assert not back.exists()
    # a damaged code decodes to something else: the CRC32 check refuses it and writes nothing
    data = bytearray(packed.read_bytes())
    data[-20] ^= 0xFF
    packed.write_bytes(bytes(data))
    out = subprocess.run([exe, "--load", ck, "-d", str(packed), str(back)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 1 and "CRC32" in out.stderr, out.stderr
    assert not back.exists()
