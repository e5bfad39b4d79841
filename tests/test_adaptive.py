"""-m gpu: lstm_hip_encode_adaptive / lstm_hip_decode_adaptive -- the model trains on the bytes it has coded (include/lstm_hip.h,
DESIGN.md section 3.7).  The decoder must rebuild the encoder's model bit for bit at every block; the coding half must be
the static coder and the training half the documented training loop, each pinned against a twin handle driven through the
existing calls only; and `lstm_compress --adapt` must restore a file from its container alone."""
import os
import struct
import subprocess
import zlib
import lzma

import numpy as np
import pytest

import range_coder_ref as rc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "eigen-lstm_amd")
CMP = os.path.join(PKG, "lstm_compress")

FAST_MATH, STEP_KERNELS, NO_FUSED_GRADS, BF16, PAD_HIDDEN, STABLE = 1, 4, 64, 128, 256, 512


def word_text(n, seed=11):
    """the word corpus of tools/make_text.py (400 random lower-case words, Zipf-distributed, space-separated), rebuilt from
    its fixed seed: text with context structure, unlike bench.synthetic_text"""
    rs = np.random.RandomState(seed)
    words = [bytes(rs.randint(97, 123, size=rs.randint(2, 9)).astype(np.uint8)) for _ in range(400)]
    p = 1.0 / np.arange(1, 401)
    p /= p.sum()
    return b" ".join(words[i] for i in rs.choice(400, size=n // 4 + 1, p=p))[:n]


def split(text, lengths):
    off = np.concatenate([[0], np.cumsum(lengths)])
    assert off[-1] <= len(text)
    return [text[int(off[s]):int(off[s + 1])] for s in range(len(lengths))]


# name -> (N, S, B, flags, optimizer, clip, lr)
CASES = {
    "single_cu_128_26_1": (128, 26, 1, 0, "adagrad", 0.0, 0.05),
    "256_50_32": (256, 50, 32, 0, "adagrad", 0.0, 0.05),
    "headline_512_100_64": (512, 100, 64, 0, "adagrad", 0.0, 0.05),
    "padded_100": (100, 20, 8, PAD_HIDDEN, "adagrad", 0.0, 0.05),
    "bf16_256_20_8": (256, 20, 8, BF16, "adagrad", 0.0, 0.05),
    "step_kernels": (64, 16, 4, STEP_KERNELS, "adagrad", 0.0, 0.05),
    "no_fused_grads": (256, 30, 16, NO_FUSED_GRADS, "adagrad", 0.0, 0.05),
    "adam_wd_clip": (128, 26, 8, 0, "adam", 1.0, 0.002),
    "stable_fast": (128, 26, 8, STABLE | FAST_MATH, "adagrad", 0.0, 0.05),
}


def make(case, seed=1):
    import lstm_hip
    N, S, B, flags, opt, clip, lr = CASES[case] if isinstance(case, str) else case
    L = lstm_hip.Lstm(N, S, B, flags=flags)
    L.set_params(lstm_hip.init_params(lstm_hip.MT19937Normal(seed), N))
    if opt == "adam":
        L.set_optimizer(lstm_hip.OPT_ADAM, 0.9, 0.999, 1e-8, 0.01)
    if clip:
        L.set_grad_clip(clip)
    return L


def snapshot(L, adam):
    """everything the decoder must share with the encoder: P, optimizer state, step count (as bit patterns: NaN-safe)"""
    out = [L.get_params(0).view(np.uint32), L.get_params(2).view(np.uint32), np.array([L.optimizer_steps()])]
    if adam:
        out.append(L.get_params(3).view(np.uint32))
    return out


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def even_texts(case, blocks, tail, seed=11):
    N, S, B = CASES[case][:3]
    n = blocks * (S - 1) + tail
    return split(word_text(n * B, seed), [n] * B)


# ---- 4. round trip ----------------------------------------------------------------------------------------------------
def _round_trip(case, texts):
    import lstm_hip
    cfg = CASES[case] if isinstance(case, str) else case
    adam, lr = cfg[4] == "adam", cfg[6]
    E, D = make(cfg), make(cfg)
    codes, bits, block_bits = E.encode_adaptive(texts, lr)
    for t, c in zip(texts, codes):
        assert len(c) <= lstm_hip.code_bound(len(t)) and (len(c) == 0) == (len(t) == 0)
    back = D.decode_adaptive(codes, [len(t) for t in texts], lr)
    se, sd = snapshot(E, adam), snapshot(D, adam)
    E.close()
    D.close()
    assert back == texts
    assert same(se, sd)
    n_blocks = min(len(t) for t in texts) // (cfg[1] - 1)
    assert int(se[2][0]) == n_blocks and block_bits.shape == (n_blocks + 1,)
    return codes, bits, block_bits


@pytest.mark.parametrize("case", sorted(CASES))
def test_round_trip_rebuilds_the_text_and_the_model(case):
    blocks = 4 if case != "headline_512_100_64" else 3
    _round_trip(case, even_texts(case, blocks, tail=7))


def test_round_trip_with_an_empty_stream_trains_nothing():
    cfg = (128, 26, 4, 0, "adagrad", 0.0, 0.05)
    texts = split(word_text(400), [90, 0, 120, 61])
    _, _, block_bits = _round_trip(cfg, texts)
    assert block_bits.shape == (1,)  # n_blocks = 0: everything is tail


def test_round_trip_with_streams_differing_by_a_few_bytes():
    cfg = (128, 26, 4, 0, "adagrad", 0.0, 0.05)
    texts = split(word_text(600), [103, 100, 111, 107])  # 4 blocks of 25, tails of 3, 0, 11, 7
    _round_trip(cfg, texts)


def test_round_trip_of_a_text_shorter_than_one_block():
    cfg = (128, 26, 2, 0, "adagrad", 0.0, 0.05)
    _round_trip(cfg, split(word_text(60), [24, 13]))


# ---- 5. the coding half is the static coder ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["single_cu_128_26_1", "256_50_32", "bf16_256_20_8"])
def test_with_a_zero_learning_rate_the_code_is_the_static_code(case):
    """Adagrad with lr = 0 leaves every parameter as it is (adagrad1: p - lr * (d / den), den >= 1e-5), so all blocks are
    coded with the initial parameters: code, bits and trace must be lstm_hip_encode's, which pins the carry of the coder's
    (h, c), of the range coder state and the remade image of U across every block boundary."""
    texts = even_texts(case, blocks=4, tail=9)
    A, T = make(case), make(case)
    P0 = A.get_params(0).copy()
    codes, bits, block_bits, tr = A.encode_adaptive(texts, 0.0, trace=True)
    P1 = A.get_params(0)
    steps = A.optimizer_steps()
    s_codes, s_bits, s_tr = T.encode(texts, trace=True)
    A.close()
    T.close()
    assert np.array_equal(P0.view(np.uint32), P1.view(np.uint32))
    assert steps == 4  # lr = 0 still runs the train passes
    assert codes == s_codes
    assert np.array_equal(bits.view(np.uint64), s_bits.view(np.uint64))
    assert np.array_equal(tr, s_tr)


@pytest.mark.parametrize("case", ["256_50_32", "adam_wd_clip"])
def test_block_zero_is_coded_with_the_initial_parameters(case):
    N, S, B = CASES[case][:3]
    L = S - 1
    texts = even_texts(case, blocks=3, tail=5)
    A, T = make(case), make(case)
    _, _, _, tr = A.encode_adaptive(texts, CASES[case][6], trace=True)
    _, _, s_tr = T.encode([t[:L] for t in texts], trace=True)
    _, _, full_tr = T.encode(texts, trace=True)
    A.close()
    T.close()
    n = len(texts[0])
    for s in range(B):
        assert np.array_equal(tr[s * n:s * n + L], s_tr[s * L:(s + 1) * L]), s
    assert not np.array_equal(tr, full_tr)  # ... and the later blocks with other parameters: the model moved


# ---- 6. the training half is the documented training ------------------------------------------------------------------
@pytest.mark.parametrize("case", ["single_cu_128_26_1", "bf16_256_20_8", "adam_wd_clip", "headline_512_100_64"])
def test_the_model_after_encoding_is_the_one_train_windows_makes(case):
    N, S, B, flags, opt, clip, lr = CASES[case]
    adam = opt == "adam"
    n = 3
    texts = even_texts(case, blocks=n, tail=4)
    A, T = make(case), make(case)
    A.encode_adaptive(texts, lr)
    text = np.frombuffer(b"".join(texts), np.uint8)
    off = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.uint64)
    T.set_text(text)
    T.reset_window()
    T.set_cursors(off[:B])
    T.set_stride(S - 1, S - 1)
    T.train_windows(n, lr)
    sa, st = snapshot(A, adam), snapshot(T, adam)
    wa, wt = A.get_window(), T.get_window()
    ha, ht = A.get_state(S - 1), T.get_state(S - 1)
    na = A.grad_norms(n) if clip else None
    nt = T.grad_norms(n) if clip else None
    A.close()
    T.close()
    assert same(sa, st)
    assert int(sa[2][0]) == n
    assert np.array_equal(wa[0], wt[0]) and np.array_equal(wa[1], wt[1])  # k_block_window's windows are k_slide_window's
    assert np.array_equal(ha[0].view(np.uint32), ht[0].view(np.uint32)) and np.array_equal(ha[1].view(np.uint32), ht[1].view(np.uint32))
    if clip:
        assert np.array_equal(na.view(np.uint64), nt.view(np.uint64)) and np.all(na > 0)


def test_the_callers_stride_text_and_cursors_are_left_alone():
    """the header's choice: stride, loss mode, text and cursors are neither read nor written by the adaptive calls"""
    case = "single_cu_128_26_1"
    N, S, B = CASES[case][:3]
    corpus = np.frombuffer(word_text(4000, seed=5), np.uint8)
    A, T = make(case), make(case)
    for L in (A, T):
        L.set_text(corpus)
        L.reset_window()
        L.set_cursors([700])
        L.set_stride(3, 2)
    A.encode_adaptive(even_texts(case, blocks=2, tail=3), 0.05)
    assert list(A.get_cursors()) == [700]
    A.set_params(T.get_params(0))
    A.set_params(T.get_params(2), which=2)
    A.set_optimizer_steps(0)
    A.reset_window()
    for t in range(S):
        A.set_state(t, *T.get_state(t))
    la, lt = A.train_windows(5, 0.05), T.train_windows(5, 0.05)
    pa, pt, ca, ct = A.get_params(0), T.get_params(0), A.get_cursors(), T.get_cursors()
    A.close()
    T.close()
    assert np.array_equal(la, lt) and np.array_equal(pa.view(np.uint32), pt.view(np.uint32))
    assert list(ca) == list(ct) == [715]


# ---- 7. the coder is the specified coder ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["256_50_32", "stable_fast"])
def test_the_device_trace_reencodes_to_the_code(case):
    import lstm_hip
    texts = even_texts(case, blocks=4, tail=6)
    A = make(case)
    codes, bits, block_bits, tr = A.encode_adaptive(texts, CASES[case][6], trace=True)
    A.close()
    assert tr[:, 2].max() <= 65281 and tr[:, 1].min() >= 1
    n = len(texts[0])
    for s, (t, c) in enumerate(zip(texts, codes)):
        rows = tr[s * n:(s + 1) * n]
        assert rc.encode(rows) == c, s
        per = -np.log2(rows[:, 1].astype(np.float64) / rows[:, 2])
        assert abs(per.sum() - bits[s]) <= 1e-9 * max(1.0, bits[s])
        assert len(c) <= lstm_hip.code_bound(len(t))
        # the static coder's documented slack: the flush allowance (32 bits) and the coder's rounding (<= 0.01 bit per byte)
        assert 8 * len(c) <= bits[s] + 32 + 0.01 * n, (s, 8 * len(c), bits[s])
        assert 8 * len(c) >= bits[s] - 1e-6
    assert abs(block_bits.sum() - bits.sum()) <= 1e-12 * bits.sum()
    S = CASES[case][1]
    per_all = -np.log2(tr[:, 1].astype(np.float64) / tr[:, 2]).reshape(len(texts), n)
    for k in range(4):
        want = per_all[:, k * (S - 1):(k + 1) * (S - 1)].sum()
        assert abs(block_bits[k] - want) <= 1e-9 * want, k
    assert abs(block_bits[4] - per_all[:, 4 * (S - 1):].sum()) <= 1e-9 * block_bits[4]


# ---- 8. it learns -----------------------------------------------------------------------------------------------------
LEARN = (128, 26, 8, STABLE, "adagrad", 5.0, 0.05)  # Adagrad, lr 0.05, global-norm clip 5: stays finite on this text


def test_it_learns_the_text_it_codes():
    """>= 200 blocks of the word corpus.  Orderings only: the figures are in DESIGN.md section 3.7 and profiles/adaptive/."""
    N, S, B = LEARN[:3]
    L = S - 1
    blocks = 240
    n = blocks * L
    texts = split(word_text(n * B), [n] * B)
    A, T = make(LEARN), make(LEARN)
    codes, bits, block_bits = A.encode_adaptive(texts, LEARN[6])
    norms = A.grad_norms(blocks)
    s_codes, s_bits = T.encode(texts)
    A.close()
    T.close()
    assert block_bits.shape == (blocks + 1,) and np.all(np.isfinite(block_bits)) and np.all(np.isfinite(norms))
    adaptive, static = sum(len(c) for c in codes), sum(len(c) for c in s_codes)
    q = blocks // 4
    first, last = block_bits[:q].sum() / (q * L * B), block_bits[blocks - q:blocks].sum() / (q * L * B)
    raw = b"".join(texts)
    print(f"adaptive {adaptive} B ({8 * adaptive / len(raw):.4f} bits/char), static-initial {static} B "
          f"({8 * static / len(raw):.4f}), zlib-9 {len(zlib.compress(raw, 9))} B, lzma-9 {len(lzma.compress(raw, preset=9))} B; "
          f"bits/char by quarter: " + ", ".join(f"{block_bits[i * q:(i + 1) * q].sum() / (q * L * B):.4f}" for i in range(4)))
    assert adaptive < static, (adaptive, static)
    assert last < first, (first, last)


# ---- 9. a truncated code stays inside its stream ----------------------------------------------------------------------
def test_a_truncated_code_decodes_to_its_length_and_is_right_up_to_the_cut():
    """The decoder reads 0 past the end of a stream's code and clamps (section 3.6), so the call succeeds and returns the
    requested lengths.  Until the first wrong byte both sides hold the same model; within that byte's block the other
    streams are still coded with the same parameters, so they are right to the end of that block.  From the next block on
    the decoder has trained on other bytes than the encoder and every stream may differ: the container's CRC32 catches it."""
    cfg = (128, 26, 4, 0, "adagrad", 0.0, 0.05)
    S, L, cut = cfg[1], cfg[1] - 1, 1
    texts = split(word_text(4 * 140), [140] * 4)  # 5 blocks and a tail of 15
    E, D = make(cfg), make(cfg)
    codes, _, _ = E.encode_adaptive(texts, cfg[6])
    broken = list(codes)
    broken[cut] = codes[cut][:len(codes[cut]) // 3]
    back = D.decode_adaptive(broken, [len(t) for t in texts], cfg[6])
    E.close()
    D.close()
    assert [len(b) for b in back] == [len(t) for t in texts]
    wrong = [i for i in range(len(texts[cut])) if back[cut][i] != texts[cut][i]]
    assert wrong, "a third of the code cannot hold the whole stream"
    j = wrong[0]
    block = j // L
    for s in range(4):
        good = j if s == cut else min((block + 1) * L, len(texts[s]))
        assert back[s][:good] == texts[s][:good], (s, good)


# ---- 10. the program --------------------------------------------------------------------------------------------------
def _run(args, cwd):
    return subprocess.run([CMP] + args, capture_output=True, text=True, timeout=600, cwd=cwd)


MODEL = ["--hidden", "128", "--seq", "26", "--streams", "8", "--lr", "0.05", "--clip-norm", "5", "--stable-softmax"]


def test_program_restores_a_file_from_the_container_alone(tmp_path):
    raw = word_text(65536, seed=3)
    (tmp_path / "in").write_bytes(raw)
    out = _run(["--adapt", "-c", "in", "out.lhad"] + MODEL, tmp_path)
    assert out.returncode == 0, out.stderr
    print(out.stdout.strip())
    blob = (tmp_path / "out.lhad").read_bytes()
    assert blob[:4] == b"LHAD" and len(blob) < len(raw)
    N, S, B = struct.unpack_from("<III", blob, 16)
    assert (N, S, B) == (128, 26, 8) and struct.unpack_from("<Q", blob, 104)[0] == len(raw)
    assert struct.unpack_from("<I", blob, 112)[0] == zlib.crc32(raw)
    out = _run(["--adapt", "-d", "out.lhad", "back"], tmp_path)
    assert out.returncode == 0, out.stderr
    assert (tmp_path / "back").read_bytes() == raw
    assert sorted(p.name for p in tmp_path.iterdir()) == ["back", "in", "out.lhad"]  # no checkpoint, no temporary file

    # a recorded CU count or plan identity that is not this device's: refused after create, by name, nothing written
    for offset, field in ((92, "CU count"), (184 + 3, "plan identity"), (120 + 1, "device name")):
        bad = bytearray(blob)
        bad[offset] ^= 0x01
        (tmp_path / "bad.lhad").write_bytes(bytes(bad))
        out = _run(["--adapt", "-d", "bad.lhad", "bad_out"], tmp_path)
        assert out.returncode == 1 and field in out.stderr, (field, out.stderr)
        assert not (tmp_path / "bad_out").exists() and not (tmp_path / "bad_out.tmp").exists()

    # a damaged code decodes to something else: the CRC32 refuses it before OUT exists
    bad = bytearray(blob)
    bad[312 + 8 * 8 + 2000] ^= 0x10
    (tmp_path / "bad.lhad").write_bytes(bytes(bad))
    out = _run(["--adapt", "-d", "bad.lhad", "bad_out"], tmp_path)
    assert out.returncode == 1 and "CRC32" in out.stderr, out.stderr
    assert not (tmp_path / "bad_out").exists() and not (tmp_path / "bad_out.tmp").exists()


def test_program_with_a_checkpoint_as_prior(tmp_path):
    import lstm_hip
    N, M = 32, 256
    P = lstm_hip.init_params(lstm_hip.MT19937Normal(9), N)
    shapes = [("W", 4 * N, M), ("U", 4 * N, N), ("b", 4 * N, 1), ("Why", M, N), ("by", M, 1)]
    at = 0
    for name, r, c in shapes:
        np.savetxt(tmp_path / f"ck_{name}.txt", P[at:at + r * c].reshape(r, c, order="F"), fmt="%.9g")
        at += r * c
    raw = word_text(20000, seed=4)
    (tmp_path / "in").write_bytes(raw)
    out = _run(["--adapt", "--load", "ck", "-c", "in", "out.lhad", "--seq", "20", "--streams", "4"], tmp_path)
    assert out.returncode == 0, out.stderr
    blob = (tmp_path / "out.lhad").read_bytes()
    assert struct.unpack_from("<I", blob, 16)[0] == N and struct.unpack_from("<I", blob, 44)[0] == 1
    out = _run(["--adapt", "-d", "out.lhad", "back"], tmp_path)  # the prior is part of the model: it must be given
    assert out.returncode == 1 and "--load PREFIX" in out.stderr and not (tmp_path / "back").exists()
    out = _run(["--adapt", "--load", "ck", "-d", "out.lhad", "back"], tmp_path)
    assert out.returncode == 0, out.stderr
    assert (tmp_path / "back").read_bytes() == raw
