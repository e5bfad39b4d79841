"""The cases of tests/test_products.py (-m gpu) and of its numpy control, tests/test_products_cpu.py: one table, one set of
operands, one set of checks, so that the control covers exactly what the GPU file asserts.

Under test are the dense products that run once per window and the bf16 packers, each called on its own through the driver
tests/product_check.hip (built as eigen-lstm_amd/product_check): gemm / gemm_slabs / gemm_fold (csrc/gemm.hip k_gemm_regs,
five instantiations; csrc/kernels.hip k_gemm_reduce), gemm_bf16 (k_gemm_bf16, 64 x 64 and 128 x 128 tiles),
transpose_pack_bf16 and pack_bf16.  They are pure functions of their operands, so the checks are sharp:

  exact     operands from {+-1, +-2, +-3} (exact in bf16 too): every product and partial sum is an integer below 2^24, the
            result does not depend on the summation order and must equal the int64 product bit for bit; every sentinel
            (guards, rows M..ldc-1, slabs not used) must be untouched, every element of C written, two runs identical.
  accuracy  N(0,1) operands: e = |C - ref64| / (2^-24 sum_k |a_k b_k|) per output, against the same figure of a plain ascending
            float32 multiply-then-add loop over the same operands (the yardstick: reference side only).  Conditions:
            RMS(e) <= 1.25 x the yardstick's, max(e) <= 2 x the yardstick's (RMS_MARGIN, MAX_MARGIN).
  packers   bit for bit against round-to-nearest-even, zeros in K <= k < Kpad, sentinels everywhere else.

A `run` is what a driver process (or the control's emulation of one) leaves: {(id, buffer, rep): whole allocation as bytes}
and {(id, rep, key): value}.  An output allocation is [GUARD bytes | payload | GUARD bytes], pre-filled with a NaN pattern.

contract_violations() is the written contract of csrc/kernels.h (the comment above gemm) as code; every case here and every
product library_products() lists -- the ones do_forward / do_backward issue -- must satisfy it.
"""
import collections
import zlib

import numpy as np

GUARD = 256                   # bytes before and after every output payload (tests/product_check.hip)
SENT_F32 = 0x7FC5A5A5         # a quiet NaN with a payload no arithmetic here produces
SENT_U16 = 0x7FC57FC5         # two bf16 NaNs
RMS_MARGIN, MAX_MARGIN = 1.25, 2.0
NW = 4                        # waves of a k_gemm_regs workgroup: wave w takes the 8-deep k-groups w, w + NW, ...
BF16_KTILE = 64               # HBK_ of k_gemm_bf16
BLOCK_CAP = 2048              # grid cap of k_gemm_reduce and k_pack_bf16 (256 threads each)
POISON = 1000.0               # fills operand padding (ld > rows): a read of it breaks every check

Job = collections.namedtuple("Job", "kind id what p A B a B_logical mode")
# p: the manifest keys; A, B: the flat operand images as uploaded; a[m, k], B_logical[n, k]: the logical operands (float64)


def ceil_div(a, b):
    return -(-a // b)


# ---- bfloat16 on the host -----------------------------------------------------------------------------------------------
def bf16_rne(x):
    """float32 -> bf16 bits, round to nearest even; NaN -> a quiet NaN."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r)


def bf16_truncate(x):
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bf16_to_f32(h):
    return (np.asarray(h, np.uint16).astype(np.uint32) << 16).view(np.float32)


def is_bf16_nan(h):
    return (np.asarray(h, np.uint16) & 0x7FFF) > 0x7F80


# ---- the shape rules of the library, restated (csrc/gemm.hip gemm_regs / gemm_regs_splits, csrc/kernels.hip gemm_bf16) ----
def regs_plan(akf, bkf, M, Nn, K, splits, small_ok=True):
    """(slabs used, kchunk, instantiation (akf, bkf, VA, VB)) of gemm_regs for a request of `splits`."""
    splits = max(splits, 1)
    kchunk = ceil_div(ceil_div(K, splits), 8) * 8
    used = ceil_div(K, kchunk)
    small = small_ok and ceil_div(M, 128) * ceil_div(Nn, 64) * used < 128
    if akf and bkf:
        inst = (True, True, 2, 2)
    elif akf:
        raise ValueError("k fast x k slow: no product of the window has this form")
    else:
        inst = (False, bkf, 2 if small else 4, 2)
    return used, kchunk, inst


INSTANTIATIONS = {(False, False, 2, 2), (False, False, 4, 2), (False, True, 2, 2), (False, True, 4, 2), (True, True, 2, 2)}


def regs_pick_splits(akf, bkf, M, Nn, K, n_cus):
    if akf or bkf:
        return 1
    tiles, splits = ceil_div(M, 128) * ceil_div(Nn, 64), 1
    while tiles * splits * 2 <= n_cus and K // (splits * 2) >= 256:
        splits *= 2
    return splits


def bf16_plan(M, Nn, K, splits, force_tile=0):
    splits = max(splits, 1)
    kchunk = ceil_div(ceil_div(K, splits), BF16_KTILE) * BF16_KTILE
    used = ceil_div(K, kchunk)
    tile = force_tile if force_tile in (64, 128) else (64 if ceil_div(M, 128) * ceil_div(Nn, 128) * used < 128 else 128)
    return used, kchunk, tile


def bf16_pick_splits(M, Nn, K):
    tiles, splits = ceil_div(M, 128) * ceil_div(Nn, 128), 1
    while tiles * splits < 256 and K // (splits * 2) >= 4 * BF16_KTILE:
        splits *= 2
    return splits


# ---- the contract of csrc/kernels.h, as code -------------------------------------------------------------------------------
def contract_violations(p):
    """p: kind ('gemm' | 'gemm_bf16'), TA, TB, M, Nn, K, lda, ldb, ldc and a_off, b_off, c_off: element offsets of the three
    bases from 16-byte aligned addresses.  Returns the list of broken clauses (empty: inside the contract)."""
    bad = []
    M, Nn, K, lda, ldb, ldc = (p[k] for k in ("M", "Nn", "K", "lda", "ldb", "ldc"))
    a_off, b_off, c_off = p.get("a_off", 0), p.get("b_off", 0), p.get("c_off", 0)
    if min(M, Nn, K) < 1:
        bad.append("M, Nn, K >= 1")
    if ldc < M:
        bad.append("ldc >= M")
    if p["kind"] == "gemm_bf16":
        if K % 64:
            bad.append("bf16: K % 64 == 0")
        if lda % 8 or ldb % 8 or lda < K or ldb < K:
            bad.append("bf16: lda, ldb multiples of 8, >= K")
        if a_off % 8 or b_off % 8:
            bad.append("bf16: A, B 16-byte aligned")
        return bad
    akf, bkf = bool(p["TA"]), not p["TB"]
    if akf and not bkf:
        bad.append("TA && TB does not exist")
        return bad
    if (akf or bkf) and K % 8:
        bad.append("K % 8 == 0 when an operand is k fast")
    if akf:                                   # A[m*lda + k]: any M; C written one float at a time
        if lda % 4 or lda < K or a_off % 4:
            bad.append("k-fast A: lda % 4 == 0, lda >= K, A 16-byte aligned")
    else:                                     # A[k*lda + m]: four consecutive rows per lane, C stored the same way
        if M % 4 or lda % 4 or lda < M or a_off % 4:
            bad.append("k-slow A: M % 4 == 0, lda % 4 == 0, lda >= M, A 16-byte aligned")
        if ldc % 4 or c_off % 4:
            bad.append("k-slow A: ldc % 4 == 0, C 16-byte aligned")
    if bkf:                                   # B[n*ldb + k]: any Nn
        if ldb % 4 or ldb < K or b_off % 4:
            bad.append("k-fast B: ldb % 4 == 0, ldb >= K, B 16-byte aligned")
    else:                                     # B[k*ldb + n]: two consecutive rows per lane
        if Nn % 2 or ldb % 2 or ldb < Nn or b_off % 2:
            bad.append("k-slow B: Nn % 2 == 0, ldb % 2 == 0, ldb >= Nn, B 8-byte aligned")
    # lane offsets and group offsets are 32-bit: the operands' extents in floats stay below 2^32
    ext_a = (M - 1) * lda + K if akf else (K - 1) * lda + M
    ext_b = (Nn - 1) * ldb + K if bkf else (K - 1) * ldb + Nn
    if max(ext_a, ext_b) >= 2 ** 32:
        bad.append("operand extents below 2^32 floats")
    return bad


def padded_hidden(N, bf16=False, step=False):
    """csrc/lstm_hip_api.cpp padded_hidden: the internal width LSTM_HIP_PAD_HIDDEN gives a logical N (0: refused)."""
    up = lambda n, k: ceil_div(n, k) * k
    if step:
        return up(N, 16)
    if bf16:
        return up(N, 128) if up(N, 128) <= 1024 else 0
    if N <= 64 or N > 1024:
        return up(N, 16)
    if N % 64 == 0:
        return N
    return next((w for w in (128, 256, 512) if N <= w), 1024)


def library_products(Np, S, B, fused=False, bf16=False, du_split=False):
    """The products do_forward / do_backward (csrc/lstm_hip_api.cpp) issue for internal width Np, as contract_violations()
    takes them.  Offsets are in elements from the hipMalloc'ed buffer (or from the flat parameter block for Why / dWhy / dU).
    The superset over the engine forms: a form that computes a product inside its recurrence simply does not issue it."""
    N, G4, T = Np, 4 * Np, (S - 1) * B
    why = 4 * N * 256 + 4 * N * N + 4 * N     # ParamLayout: [W | U | b | Why | by]
    u = 4 * N * 256
    out = []
    if bf16:
        Tpad = ceil_div(T, 64) * 64
        SBpad = ceil_div(B + Tpad, 64) * 64
        g = dict(kind="gemm_bf16", TA=0, TB=0)
        out += [dict(g, name="Y", M=256, Nn=T, K=N, lda=N, ldb=N, ldc=256, b_off=N * B, c_off=256 * B),
                dict(g, name="DHy", M=N, Nn=T, K=256, lda=256, ldb=256, ldc=N, c_off=N * B),
                dict(g, name="dWhy", M=256, Nn=N, K=Tpad, lda=Tpad, ldb=SBpad, ldc=256, b_off=B, c_off=why),
                dict(g, name="dU", M=G4, Nn=N, K=Tpad, lda=Tpad, ldb=SBpad, ldc=G4, c_off=u)]
        return out
    g = dict(kind="gemm")
    out.append(dict(g, name="Y", TA=0, TB=0, M=256, Nn=T, K=N, lda=256, ldb=N, ldc=256, a_off=why, b_off=N * B, c_off=256 * B))
    if not fused:
        out.append(dict(g, name="DHy", TA=1, TB=0, M=N, Nn=T, K=256, lda=256, ldb=256, ldc=N, a_off=why, b_off=256 * B,
                        c_off=N * B))
        out.append(dict(g, name="dWhy", TA=0, TB=1, M=256, Nn=N, K=T, lda=256, ldb=N, ldc=256, a_off=256 * B, b_off=N * B,
                        c_off=why))
    if du_split:
        n1 = (N // 2) // 64 * 64 or N // 2
        out.append(dict(g, name="dU half 0", TA=0, TB=1, M=G4, Nn=n1, K=T, lda=G4, ldb=N, ldc=G4, a_off=G4 * B, c_off=u))
        out.append(dict(g, name="dU half 1", TA=0, TB=1, M=G4, Nn=N - n1, K=T, lda=G4, ldb=N, ldc=G4, a_off=G4 * B, b_off=n1,
                        c_off=u + G4 * n1))
    out.append(dict(g, name="dU", TA=0, TB=1, M=G4, Nn=N, K=T, lda=G4, ldb=N, ldc=G4, a_off=G4 * B, c_off=u))
    return out


# ---- the table -------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "id kind what p")


def _gemm(what, TA, TB, M, Nn, K, splits=1, kind="gemm", lda=None, ldb=None, ldc=None, **extra):
    akf, bkf = bool(TA), not TB
    p = dict(TA=int(TA), TB=int(TB), M=M, Nn=Nn, K=K, splits=splits, lda=lda or (K if akf else M), ldb=ldb or (K if bkf else Nn),
             ldc=ldc or M, **extra)
    form = ("kf" if akf else "ks") + ("kf" if bkf else "ks")
    cid = f"{kind}-{form}-{M}x{Nn}x{K}-s{splits}" + (f"-lda{lda}" if lda else "") + (f"-ldb{ldb}" if ldb else "") + \
          (f"-ldc{ldc}" if ldc else "") + ("-fold" if extra.get("fold") else "")
    return Case(cid, kind, what, p)


def _kss():
    """k slow x k slow (dU, dWhy): gemm(TA = 0, TB = 1)."""
    c = []
    tails = {1: "tail only, one term: no full group, the tail wave is wave 0", 7: "tail only, 7 terms, both k-slots of the tail",
             8: "exactly one group, no tail: waves 1-3 contribute zeros", 9: "one group and a one-term tail on wave 1",
             63: "7 groups and a 7-term tail on wave 3", 64: "NW x DEPTH = 8 groups exactly: every wave's pipeline full once, no tail",
             65: "8 groups and a one-term tail that wraps to wave 0", 72: "9 groups: wave 0 starts a second round of its pipeline",
             531: "66 groups and a 3-term tail on wave 2: many rounds"}
    for K, what in tails.items():
        c.append(_gemm(what, 0, 1, 192, 80, K))
    for M in (64, 192, 256, 320):
        for Nn in (16, 48, 80, 144):
            for K in (9, 72):
                if (M, Nn) != (192, 80):
                    c.append(_gemm(f"M = {M}: {M / 64:g} tiles of 64, {M / 128:g} of 128; Nn = {Nn}: {Nn / 64:g} tiles of 64; "
                                   + ("one group and a tail" if K == 9 else "9 groups"), 0, 1, M, Nn, K))
    c += [
        _gemm("second slab is tail only (kchunk 16, one term left)", 0, 1, 64, 16, 17, 2),
        _gemm("second slab is tail only, through gemm_slabs + gemm_fold", 0, 1, 192, 48, 17, 2, "gemm_slabs", fold=1),
        _gemm("request of 8 with K / 8 = 1: recomputed to 2 slabs of 8 and 1", 0, 1, 192, 80, 9, 8),
        _gemm("request of 8 recomputed to 2 slabs, the count returned", 0, 1, 64, 48, 9, 8, "gemm_slabs"),
        _gemm("3 slabs of 24, 24, 17: a tail in the last slab only", 0, 1, 192, 80, 65, 3),
        _gemm("2 slabs of 40 and 32, no tail", 0, 1, 256, 144, 72, 2),
        _gemm("request of 8 at K = 72: kchunk 16, 5 slabs, the last of 8", 0, 1, 64, 16, 72, 8),
        _gemm("3 slabs of 184, 184, 163 with a 3-term tail", 0, 1, 320, 144, 531, 3),
        _gemm("8 slabs of 72 (last 27): split-K and a k tail, slabs returned unfolded", 0, 1, 320, 80, 531, 8, "gemm_slabs"),
        _gemm("2 slabs of 272 and 259, folded by gemm_fold from the returned count", 0, 1, 256, 48, 531, 2, "gemm_slabs", fold=1),
        _gemm("one slab through gemm_slabs: the product itself, ld = M", 0, 1, 192, 16, 63, 1, "gemm_slabs"),
        _gemm("ldc = M + 4: rows M..ldc-1 of every column keep their sentinels", 0, 1, 192, 80, 72, 1, ldc=196),
        _gemm("ldc = M + 4 behind a fold of 2 slabs", 0, 1, 320, 48, 65, 2, ldc=324),
        _gemm("ldc = M + 4, M a multiple of both tiles", 0, 1, 256, 16, 9, 1, ldc=260),
        _gemm("lda = M + 4, ldb = Nn + 2: operand lines longer than the rows read", 0, 1, 192, 80, 65, 1, lda=196, ldb=82),
    ]
    return c


NN_EDGE = (1, 2, 31, 32, 33, 63, 64, 65, 531)


def _ksf():
    """k slow x k fast (Y = Why H): gemm(0, 0), M = 256."""
    what = {1: "one column: every lane of the B fragment clamps to row 0", 2: "two columns", 31: "one short of a fragment",
            32: "one fragment of a 64 tile", 33: "one column into the second subtile", 63: "one short of a tile",
            64: "one tile exactly", 65: "one column into a second tile", 531: "9 tiles, the last with 19 columns"}
    c = [_gemm(f"K = {K}: {K // 8} groups; Nn = {Nn}: {what[Nn]}", 0, 0, 256, Nn, K) for K in (16, 48, 80, 1040) for Nn in NN_EDGE]
    c.append(_gemm("ldb = K + 4: k-fast rows longer than K; ldc = M + 4", 0, 0, 256, 33, 48, ldb=52, ldc=260))
    return c


def _kff():
    """k fast x k fast (DHy = Why^T dY): gemm(1, 0), K = 256."""
    c = [_gemm(f"M = {M}: {M / 64:g} tiles of 64 with clamped A rows; Nn = {Nn}", 1, 0, M, Nn, 256) for M in (16, 48, 80)
         for Nn in NN_EDGE]
    c.append(_gemm("ldc = M + 4 with scalar stores; lda = K + 8", 1, 0, 48, 33, 256, lda=264, ldc=52))
    return c


def _fold():
    f = lambda what, splits, M, Nn, stride=0, ldc=None: Case(
        f"fold-{M}x{Nn}-z{splits}-st{stride}" + (f"-ldc{ldc}" if ldc else ""), "gemm_fold", what,
        dict(splits=splits, M=M, Nn=Nn, stride=stride, ldc=ldc or M))
    return [
        f("stride 0 means M*Nn: densely packed slabs", 3, 192, 80),
        f("slab stride larger than M*Nn: poison between the slabs", 3, 192, 80, 192 * 80 + 36),
        f("one slab: a copy; ldc = M + 4", 1, 64, 16, 0, 68),
        f("the per-group partial blocks of the fused backward pass: one column, a stride far beyond it", 5, 1000, 1, 4096),
        f("256 x 2049 is more than 2048 x 256 elements: the grid-stride loop runs twice for the first 256 threads' worth", 2, 256, 2049),
        f("grid-stride loop with a given stride and ldc = M + 4", 2, 256, 2049, 256 * 2049 + 4, 260),
    ]


def _bf16_case(name, what, M, Nn, K, splits=1, b_off=0, ldb=None, lda=None, ldc=None):
    p = dict(M=M, Nn=Nn, K=K, splits=splits, lda=lda or K, ldb=ldb or K, ldc=ldc or M, b_off=b_off)
    return Case(f"bf16-{name}-{M}x{Nn}x{K}-s{splits}" + (f"-off{b_off}" if b_off else "") + (f"-ldc{ldc}" if ldc else ""), "gemm_bf16", what, p)


T_EDGE = (8, 56, 64, 72, 136)


def _bf16():
    c = []
    for T in T_EDGE:
        for K in (64, 128, 192, 320):
            c.append(_bf16_case("Y", f"Y: T = {T} columns ({T / 64:g} tiles of 64, {T / 128:g} of 128), {K // 64} k-tiles", 256, T, K))
    for N in (128, 256):
        for T in T_EDGE:
            c.append(_bf16_case("DHy", f"DHy: N = {N} rows, T = {T} columns, 4 k-tiles", N, T, 256))
    sb = lambda B, Tpad: ceil_div(B + Tpad, 64) * 64
    for N, Tpad, splits, B in ((128, 64, 1, 8), (256, 128, 2, 24), (128, 192, 3, 8), (256, 320, 2, 24), (128, 320, 3, 24), (256, 192, 1, 8)):
        c.append(_bf16_case("dWhy", f"dWhy: B operand offset by {B} elements in lines of {sb(B, Tpad)}; {splits} slab(s) of K = {Tpad}"
                            + ("; slabs of 192 and 128" if (Tpad, splits) == (320, 2) else ""), 256, N, Tpad, splits, B, sb(B, Tpad)))
    for N, Tpad, splits in ((128, 64, 1), (128, 128, 2), (256, 192, 3), (128, 320, 2), (256, 320, 3), (256, 128, 1)):
        c.append(_bf16_case("dU", f"dU: 4N = {4 * N} rows, {splits} slab(s) of K = {Tpad}"
                            + ("; slabs of 192 and 128" if (Tpad, splits) == (320, 2) else ""), 4 * N, N, Tpad, splits, 0, sb(8, Tpad)))
    c.append(_bf16_case("Y", "ldc = M + 4 and 2 slabs", 256, 72, 128, 2, ldc=260))
    c.append(_bf16_case("Y", "request of 3 with 2 k-tiles: recomputed to 2 slabs", 256, 56, 128, 3))
    return c


def _tpack():
    c = []
    for K in (1, 63, 64, 65, 100):
        for R, ld in ((16, 16), (100, 104), (256, 256), (100, 100), (16, 20), (256, 260)):
            for extra in (0, 64):
                Kpad = ceil_div(K, 64) * 64 + extra
                c.append(Case(f"tpack-K{K}-R{R}-ld{ld}-Kpad{Kpad}", "transpose_pack_bf16",
                              f"K = {K} of Kpad = {Kpad}: {Kpad - K} zeros per row; R = {R} ({R / 64:g} tiles), ld = {ld}",
                              dict(K=K, R=R, ld=ld, Kpad=Kpad)))
    return c


def _pack():
    what = {1: "one element", 255: "one short of a block", 256: "one block", 257: "one element into a second block",
            524291: "2048 blocks x 256 threads + 3: past the block cap, the grid-stride loop runs twice for three threads"}
    return [Case(f"pack-{n}", "pack_bf16", w, dict(n=n)) for n, w in what.items()]


KSS, KSF, KFF, FOLD, BF16, TPACK, PACK = _kss(), _ksf(), _kff(), _fold(), _bf16(), _tpack(), _pack()

# the headline shape (Np 512, S 100, B 64: T = 6336), splits = -1: what the library's own rule picks for the device
_T, _N, _B = 99 * 64, 512, 64
_TPAD = ceil_div(_T, 64) * 64
_SBPAD = ceil_div(_B + _TPAD, 64) * 64
REAL_FP32 = [
    _gemm("headline dU: 2048 x 512, K = 6336", 0, 1, 2048, 512, _T, -1),
    _gemm("headline dU as the fused loop runs it: slabs left for the update launch", 0, 1, 2048, 512, _T, -1, "gemm_slabs"),
    _gemm("headline dWhy: 256 x 512, K = 6336", 0, 1, 256, 512, _T, -1),
    _gemm("headline Y: 256 x 6336, K = 512", 0, 0, 256, _T, 512, -1),
    _gemm("headline DHy: 512 x 6336, K = 256", 1, 0, 512, _T, 256, -1),
]
REAL_BF16 = [
    _bf16_case("dU", "headline dU", 2048, 512, _TPAD, -1, 0, _SBPAD),
    _bf16_case("dWhy", "headline dWhy, B operand offset by the batch", 256, 512, _TPAD, -1, _B, _SBPAD),
    _bf16_case("Y", "headline Y", 256, _T, 512, -1),
    _bf16_case("DHy", "headline DHy", 512, _T, 256, -1),
]
MAX_CUS = 512        # the real-shape jobs allocate slabs for what the rule picks on up to this many compute units

# accuracy: the chains that differ -- tail only, one round, many rounds, slabs, each operand form, both bf16 tiles' shapes
_by_id = {c.id: c for c in KSS + KSF + KFF + BF16}
ACC_FP32 = [_by_id[i] for i in (
    "gemm-ksks-192x80x9-s1", "gemm-ksks-192x80x64-s1", "gemm-ksks-192x80x531-s1", "gemm-ksks-320x144x531-s3",
    "gemm_slabs-ksks-256x48x531-s2-fold", "gemm-ksks-256x144x72-s2", "gemm-kskf-256x33x80-s1", "gemm-kskf-256x531x1040-s1",
    "gemm-kfkf-80x65x256-s1")]
ACC_BF16 = [_by_id[i] for i in ("bf16-Y-256x72x320-s1", "bf16-DHy-256x136x256-s1", "bf16-dWhy-256x256x320-s2-off24",
                                "bf16-dU-1024x256x320-s3")]

FAMILIES = dict(kss=KSS, ksf=KSF, kff=KFF, fold=FOLD, bf16=BF16, tpack=TPACK, pack=PACK, real_fp32=REAL_FP32, real_bf16=REAL_BF16)
ALL_CASES = [c for f in FAMILIES.values() for c in f]


def case_contract(case):
    """The case as contract_violations() takes it (operands and outputs start at allocation bases)."""
    if case.kind in ("gemm", "gemm_slabs"):
        return dict(case.p, kind="gemm")
    if case.kind == "gemm_bf16":
        return dict(case.p, kind="gemm_bf16", TA=0, TB=0)
    return None


# ---- operands --------------------------------------------------------------------------------------------------------------
def _rng(case, mode):
    return np.random.default_rng(zlib.crc32(f"{case.id}/{mode}".encode()))


def _draw(rng, shape, mode):
    if mode == "exact":
        return rng.choice(np.array([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0]), size=shape)
    return rng.standard_normal(shape).astype(np.float32).astype(np.float64)


def _image(x, kfast, ld, off=0):
    """Flat image of the logical operand x[r, k] with exactly the elements the layout spans; padding holds POISON."""
    R, K = x.shape
    n = off + ((R - 1) * ld + K if kfast else (K - 1) * ld + R)
    flat = np.full(n, POISON, np.float32)
    r, k = np.meshgrid(np.arange(R), np.arange(K), indexing="ij")
    flat[off + (r * ld + k if kfast else k * ld + r)] = x
    return flat


SPECIALS = np.array([0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00008000, 0x00018000, 0x3F808000, 0x3F818000, 0xBF808000,
                     0xBF818000, 0x3F808001, 0x3F807FFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001,
                     0xFFFFFFFF, 0x7F7F8000, 0x00FF8000, 0x3F7FFFFF], np.uint32)
# +-0, denormals (smallest, largest, exact ties at bit 15), ties to even in both directions and both signs, just above / below a
# tie, the largest finite float (rounds to inf), +-inf, quiet / signalling / all-ones NaN, a tie that carries into the exponent


def pack_source(rng, n):
    """n floats: normal draws, with every entry of SPECIALS spread over them (all of them once n allows)."""
    x = rng.standard_normal(n).astype(np.float32)
    x.view(np.uint32)[:] |= rng.integers(0, 2, n, dtype=np.uint32) << 15          # half of them at or past a tie bit
    x.view(np.uint32)[rng.random(n) < 0.25] &= 0xFFFF8000                         # a quarter exact ties
    pos = (np.arange(len(SPECIALS)) * 37 + 3) % n if n >= 4 * len(SPECIALS) else np.arange(min(n, len(SPECIALS)))
    x.view(np.uint32)[pos] = SPECIALS[:len(pos)]
    return x


def make_job(case, mode="exact"):
    p, rng = dict(case.p), _rng(case, mode)
    if case.kind in ("gemm", "gemm_slabs"):
        akf, bkf = bool(p["TA"]), not p["TB"]
        a, b = _draw(rng, (p["M"], p["K"]), mode), _draw(rng, (p["Nn"], p["K"]), mode)
        A, B = _image(a, akf, p["lda"]), _image(b, bkf, p["ldb"])
        want = regs_pick_splits(akf, bkf, p["M"], p["Nn"], p["K"], MAX_CUS) if p["splits"] < 0 else \
            regs_plan(akf, bkf, p["M"], p["Nn"], p["K"], p["splits"])[0]
        p.update(a_n=len(A), b_n=len(B), b_off=0, sent=SENT_F32,
                 slab_n=(max(p["splits"], want) * p["M"] * p["Nn"] + 8) if (max(p["splits"], want) > 1 or case.kind == "gemm_slabs") else 0)
        return Job(case.kind, case.id, case.what, p, A, B, a, b, mode)
    if case.kind == "gemm_bf16":
        a, b = _draw(rng, (p["M"], p["K"]), mode), _draw(rng, (p["Nn"], p["K"]), mode)
        ha, hb = bf16_rne(a.astype(np.float32)), bf16_rne(b.astype(np.float32))
        a, b = bf16_to_f32(ha).astype(np.float64), bf16_to_f32(hb).astype(np.float64)  # the images are the operands
        A, B = bf16_rne(_image(a, True, p["lda"])), bf16_rne(_image(b, True, p["ldb"], p["b_off"]))
        want = bf16_pick_splits(p["M"], p["Nn"], p["K"]) if p["splits"] < 0 else p["splits"]
        p.update(a_n=len(A), b_n=len(B), sent=SENT_F32, slab_n=(want * p["M"] * p["Nn"] + 8) if want > 1 else 0)
        return Job(case.kind, case.id, case.what, p, A, B, a, b, mode)
    if case.kind == "gemm_fold":
        step = p["stride"] or p["M"] * p["Nn"]
        n = (p["splits"] - 1) * step + p["M"] * p["Nn"]
        A = np.full(n, POISON, np.float32)
        slabs = _draw(rng, (p["splits"], p["M"] * p["Nn"]), mode)
        for z in range(p["splits"]):
            A[z * step:z * step + p["M"] * p["Nn"]] = slabs[z]
        p.update(a_n=n, sent=SENT_F32)
        return Job(case.kind, case.id, case.what, p, A, None, slabs, None, mode)
    if case.kind == "transpose_pack_bf16":
        n = (p["K"] - 1) * p["ld"] + p["R"]
        A = pack_source(rng, n)
        p.update(a_n=n, sent=SENT_U16)
        return Job(case.kind, case.id, case.what, p, A, None, None, None, mode)
    if case.kind == "pack_bf16":
        p.update(sent=SENT_U16)
        return Job(case.kind, case.id, case.what, p, pack_source(rng, p["n"]), None, None, None, mode)
    raise ValueError(case.kind)


def manifest_line(job, rep):
    keys = " ".join(f"{k}={v:x}" if k == "sent" else f"{k}={v}" for k, v in job.p.items())
    return f"{job.kind} {job.id} rep={rep} {keys}"


# ---- reading a run ---------------------------------------------------------------------------------------------------------
def split_alloc(raw, dtype, n):
    """(guard before, payload[:n], whatever follows the payload up to the end of the allocation) of an output dump."""
    raw = np.frombuffer(raw, np.uint8)
    item = np.dtype(dtype).itemsize
    assert len(raw) == GUARD + ceil_div(n * item, 4) * 4 + GUARD, (len(raw), n, dtype)
    return raw[:GUARD], raw[GUARD:GUARD + n * item].view(dtype), raw[GUARD + n * item:]


def assert_untouched(part, sent, where):
    """Every part checked here starts at a multiple of 4 bytes and is a multiple of 4 long, except behind a 16-bit image of odd
    length; the 16-bit outputs' pattern has two equal halves, so those are compared halfword by halfword."""
    b = np.ascontiguousarray(part).view(np.uint8)
    if (sent >> 16) == (sent & 0xFFFF):
        hit = np.flatnonzero(b.view(np.uint16) != np.uint16(sent & 0xFFFF)) * 2
    else:
        hit = np.flatnonzero(b.view(np.uint32) != np.uint32(sent)) * 4
    assert hit.size == 0, f"{where}: {hit.size} sentinel words overwritten, first at byte {hit[0]}"


def f32_bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def expected_used(job, run):
    """Slabs the call must have used: from the request (or the library's own pick, which must agree with the rule restated
    here for the device's CU count) through the recomputation of gemm_regs / gemm_bf16."""
    p = job.p
    req = p["splits"]
    if req < 0:
        req = run["results"][(job.id, 0, "picked")]
        n_cus = run["results"]["n_cus"]
        rule = bf16_pick_splits(p["M"], p["Nn"], p["K"]) if job.kind == "gemm_bf16" else \
            regs_pick_splits(bool(p["TA"]), not p["TB"], p["M"], p["Nn"], p["K"], n_cus)
        assert req == rule, f"{job.id}: the library picked {req} slabs, the shape rule says {rule} on {n_cus} CUs"
        # The fp32 rule's value comes back unchanged from the recomputation (gemm_slabs returns it).  The bf16 rule's is an upper
        # bound: slabs are whole k-tiles of 64, so its 16 at the headline dWhy (K = 6336) are 15 slabs of 448 -- gemm_bf16
        # returns nothing, the 16th slab must keep its sentinels.  (lstm_hip_plan_identity prints the rule's value into the
        # adaptive coder's container, so the rule is left as it is.)
        if job.kind == "gemm_bf16":
            assert bf16_plan(p["M"], p["Nn"], p["K"], req)[0] <= req
        else:
            used = regs_plan(bool(p["TA"]), not p["TB"], p["M"], p["Nn"], p["K"], req)[0]
            assert used == req, f"{job.id}: the rule picks {req} slabs, the call recomputes them to {used}"
    if job.kind == "gemm_bf16":
        return bf16_plan(p["M"], p["Nn"], p["K"], req)[:2]
    return regs_plan(bool(p["TA"]), not p["TB"], p["M"], p["Nn"], p["K"], req)[:2]


def check_product_layout(job, run, rep):
    """Sentinels, slabs and the returned count of one product job; returns C as [Nn][M] float32 (None: the job has no C) and
    the slabs as [used][Nn][M] (None: not split, or folded away)."""
    p = job.p
    M, Nn, ldc = p["M"], p["Nn"], p["ldc"]
    used, kchunk = expected_used(job, run)
    C = None
    if (job.id, "C", rep) in run["out"]:
        g0, pay, g1 = split_alloc(run["out"][(job.id, "C", rep)], np.uint32, ldc * Nn)
        assert_untouched(g0, p["sent"], f"{job.id}: guard before C")
        assert_untouched(g1, p["sent"], f"{job.id}: guard after C")
        pay = pay.reshape(Nn, ldc)
        assert_untouched(np.ascontiguousarray(pay[:, M:]), p["sent"], f"{job.id}: rows M..ldc-1 of C")
        C = np.ascontiguousarray(pay[:, :M])
        unwritten = np.argwhere(C == np.uint32(p["sent"]))
        assert unwritten.size == 0, f"{job.id}: {len(unwritten)} elements of C never written, first (n, m) = {tuple(unwritten[0])}"
        C = C.view(np.float32)
    slabs = None
    if p.get("slab_n"):
        g0, pay, g1 = split_alloc(run["out"][(job.id, "S", rep)], np.uint32, p["slab_n"])
        assert_untouched(g0, p["sent"], f"{job.id}: guard before the slabs")
        assert_untouched(g1, p["sent"], f"{job.id}: guard after the slabs")
        wrote = used if (used > 1 or job.kind == "gemm_slabs") else 0
        assert_untouched(np.ascontiguousarray(pay[wrote * M * Nn:]), p["sent"], f"{job.id}: slabs past the {wrote} used")
        if wrote:
            slabs = np.ascontiguousarray(pay[:wrote * M * Nn]).reshape(wrote, Nn, M)
            assert not (slabs == np.uint32(p["sent"])).any(), f"{job.id}: elements of a used slab never written"
            slabs = slabs.view(np.float32)
    if job.kind == "gemm_slabs":
        ret = run["results"][(job.id, rep, "ret")]
        assert ret == used, f"{job.id}: gemm_slabs returned {ret}, the recomputed count is {used}"
    return C, slabs, used, kchunk


def assert_same_bits(got, want, where):
    got, want = f32_bits(got), f32_bits(np.asarray(want, np.float32))
    bad = np.argwhere(got != want)
    assert bad.size == 0, (f"{where}: {len(bad)} of {got.size} elements differ from the integer product, first at "
                           f"{tuple(bad[0])}: got {got.view(np.float32)[tuple(bad[0])]!r}, want {want.view(np.float32)[tuple(bad[0])]!r}")


def assert_two_runs_identical(job, run):
    for (jid, buf, rep), raw in run["out"].items():
        if jid == job.id and rep == 1:
            assert raw == run["out"][(jid, buf, 0)], f"{job.id}: buffer {buf} differs between two runs in one process"


def check_exact(job, run, reps=2):
    """Every exact check of one job (module docstring)."""
    p = job.p
    for rep in range(reps):
        if job.kind in ("gemm", "gemm_slabs", "gemm_bf16"):
            C, slabs, used, kchunk = check_product_layout(job, run, rep)
            a, b = job.a, job.B_logical
            if C is not None:
                assert_same_bits(C, b @ a.T, f"{job.id} ({job.what}) C")
            if slabs is not None:
                for z in range(slabs.shape[0]):
                    k0, k1 = z * kchunk, min((z + 1) * kchunk, p["K"])
                    assert_same_bits(slabs[z], b[:, k0:k1] @ a[:, k0:k1].T, f"{job.id} ({job.what}) slab {z} = k [{k0}, {k1})")
        elif job.kind == "gemm_fold":
            g0, pay, g1 = split_alloc(run["out"][(job.id, "C", rep)], np.uint32, p["ldc"] * p["Nn"])
            assert_untouched(g0, p["sent"], f"{job.id}: guard before C")
            assert_untouched(g1, p["sent"], f"{job.id}: guard after C")
            pay = pay.reshape(p["Nn"], p["ldc"])
            assert_untouched(np.ascontiguousarray(pay[:, p["M"]:]), p["sent"], f"{job.id}: rows M..ldc-1 of C")
            assert_same_bits(np.ascontiguousarray(pay[:, :p["M"]]).view(np.float32), job.a.sum(0).reshape(p["Nn"], p["M"]),
                             f"{job.id} ({job.what}) C")
        else:
            check_pack(job, run, rep)
    if reps > 1:
        assert_two_runs_identical(job, run)


def check_pack(job, run, rep=0):
    p = job.p
    if job.kind == "pack_bf16":
        n, want = p["n"], bf16_rne(job.A)
    else:
        K, R, ld, Kpad = p["K"], p["R"], p["ld"], p["Kpad"]
        n = R * Kpad
        want = np.zeros((R, Kpad), np.uint16)
        r, k = np.meshgrid(np.arange(R), np.arange(K), indexing="ij")
        want[:, :K] = bf16_rne(job.A[k * ld + r])
        want = want.reshape(-1)
    g0, got, g1 = split_alloc(run["out"][(job.id, "C", rep)], np.uint16, n)
    assert_untouched(g0, p["sent"], f"{job.id}: guard before the image")
    assert_untouched(g1, p["sent"], f"{job.id}: guard (and padding) after the image")
    nan = is_bf16_nan(want)
    bad = np.flatnonzero((got != want) & ~nan)
    assert bad.size == 0, (f"{job.id} ({job.what}): {bad.size} of {n} halfwords differ from round-to-nearest-even, first at {bad[0]}: "
                           f"got {got[bad[0]]:#06x}, want {want[bad[0]]:#06x}")
    assert is_bf16_nan(got[nan]).all(), f"{job.id} ({job.what}): a NaN did not stay a NaN"


# ---- accuracy --------------------------------------------------------------------------------------------------------------
SAMPLE_WORK = 5e7     # M * Nn * K above which the figures are taken on a 64 x 64 sample of the outputs


def sample_of(M, Nn, K):
    """Rows and columns of C the accuracy figures are taken over: all of them for the small cases; for the headline shapes 64
    evenly spaced rows and columns, first and last included (4096 outputs: the RMS of e is then known to about 1 %).  The kernel
    and the yardstick are always compared over the SAME outputs."""
    if M * Nn * K <= SAMPLE_WORK:
        return np.arange(M), np.arange(Nn)
    pick = lambda n: np.unique(np.linspace(0, n - 1, min(n, 64)).round().astype(np.int64))
    return pick(M), pick(Nn)


def ascending_f32(a, b):
    """The yardstick: C[n, m] by a plain ascending float32 loop, product rounded, then added."""
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    acc = np.zeros((b.shape[0], a.shape[0]), np.float32)
    for k in range(a.shape[1]):
        acc = acc + b32[:, k, None] * a32[None, :, k]
    return acc


def error_units(C, a, b):
    """e = |C - ref64| / (2^-24 sum_k |a_k b_k|) per output; C, a, b restricted to the same sample."""
    ref = b @ a.T
    scale = 2.0 ** -24 * (np.abs(b) @ np.abs(a).T)
    return np.abs(C.astype(np.float64) - ref) / scale


def accuracy_figures(job, C=None, C_sample=None):
    """dict(kernel_rms, kernel_max, yard_rms, yard_max, outputs) of one accuracy job's C [Nn][M] (or of its sample alone)."""
    p = job.p
    rows, cols = sample_of(p["M"], p["Nn"], p["K"])
    a, b = job.a[rows], job.B_logical[cols]
    ek = error_units(C[np.ix_(cols, rows)] if C_sample is None else C_sample, a, b)
    ey = error_units(ascending_f32(a, b), a, b)
    rms = lambda e: float(np.sqrt(np.mean(e * e)))
    return dict(kernel_rms=rms(ek), kernel_max=float(ek.max()), yard_rms=rms(ey), yard_max=float(ey.max()), outputs=int(ek.size))


def assert_accuracy(job, fig):
    assert fig["kernel_rms"] <= RMS_MARGIN * fig["yard_rms"], f"{job.id} ({job.what}): RMS {fig}"
    assert fig["kernel_max"] <= MAX_MARGIN * fig["yard_max"], f"{job.id} ({job.what}): max {fig}"
