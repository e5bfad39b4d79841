"""The numpy control of tests/test_products.py: no GPU.

An emulation of the kernels' index work, written from csrc/gemm.hip and csrc/kernels.hip -- tile order, fragment rows and
their clamps, the k-groups of each wave, the tail wave, slabs, store predicates, the grid-stride loops, the staging of
k_gemm_bf16 and the tiles of the packers -- runs every case of tests/product_cases.py through the very checks the GPU file
applies to the driver's dumps.  Then mutants of the emulation, one per way these kernels can be subtly wrong, must each fail
the exact case named beside it: the table can see them.  Also here: the contract of csrc/kernels.h against every product the
library issues, and the claim that the table reaches all five instantiations of k_gemm_regs and both bf16 tiles.

The emulation computes a wave's partial tile with one float64 matrix product (exact on the integer operands, whatever the
order) and adds partial tiles and slabs in float32 in the kernels' order.  Summation ORDER in float32 (waves, groups, the two
k-slots of an instruction, slabs) is emulated separately (kernel_order) for the accuracy figures.  The emulation is
deterministic, so the second run of a job is a copy of the first: the two-runs check is the GPU's.
"""
import numpy as np
import pytest

import product_cases as pc
from product_cases import GUARD, NW, ceil_div

N_CUS = 256


class Alloc:
    """An output allocation as the driver makes it: [guard | payload | guard], filled with the sentinel.  Stores outside
    the allocation are counted, not made."""

    def __init__(self, n, dtype, sent):
        item = np.dtype(dtype).itemsize
        total = GUARD + ceil_div(n * item, 4) * 4 + GUARD
        self.raw = np.frombuffer(np.uint32(sent).tobytes() * (total // 4), np.uint8).copy()
        self.view, self.base, self.n, self.outside = self.raw.view(dtype), GUARD // item, n, 0

    def store(self, idx, vals):
        idx = np.asarray(idx).reshape(-1) + self.base
        vals = np.asarray(vals).reshape(-1)
        ok = (idx >= 0) & (idx < len(self.view))
        self.outside += int((~ok).sum())
        self.view[idx[ok]] = vals[ok]

    def payload(self):
        return self.view[self.base:self.base + self.n]


def frag_rows(kfast, V, r0, R):
    """(row of the product, row loaded) of fragment position p = i * V + s (Rows<KFAST, V>::row / ::offsets)."""
    i, s = np.arange(32)[:, None], np.arange(V)[None, :]
    if kfast:
        prod = r0 + 32 * s + i
        load = np.minimum(prod, R - 1)
    else:
        prod = r0 + V * i + s
        r = r0 + V * i
        load = np.where(r + V <= R, r, R - V) + s
    assert load.min() >= 0
    return prod.reshape(-1), load.reshape(-1)


def gather(X, kfast, ld, rows, ks):
    return X[rows[:, None] * ld + ks[None, :]] if kfast else X[ks[None, :] * ld + rows[:, None]]


def wave_ks(w, kbeg, kend, tail_ok, mutant=None):
    """The k indices wave w of a workgroup multiplies, in its order: groups w, w + NW, ... and, on one wave, the tail."""
    nfull = (kend - kbeg) >> 3
    groups = list(range(w, nfull, NW))
    if mutant == "wave_group" and w == 0 and groups:
        groups.pop()
    ks = [kbeg + 8 * g + np.arange(8) for g in groups]
    if tail_ok and mutant != "tail" and (kend - kbeg) & 7 and w == nfull % NW:
        ks.append(np.arange(kbeg + 8 * nfull, kend))
    return np.concatenate(ks) if ks else np.zeros(0, np.int64)


def emu_gemm_regs(akf, bkf, M, Nn, K, A, lda, B, ldb, out, ldo, splits, small_ok, mutant=None):
    used, kchunk, (_, _, VA, VB) = pc.regs_plan(akf, bkf, M, Nn, K, splits, small_ok)
    stride = M * Nn if used > 1 else 0
    TM, TN = 32 * VA, 32 * VB
    tiles_m, tiles_n = ceil_div(M, TM), ceil_div(Nn, TN)
    ntile = tiles_m * tiles_n
    for z in range(used):
        kbeg, kend = z * kchunk, min((z + 1) * kchunk, K)
        for blk in range(ntile):
            q, r, x = ntile >> 3, ntile & 7, blk & 7
            lin = (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + (blk >> 3)
            tn, tm = (lin % tiles_n, lin // tiles_n) if tiles_n <= tiles_m else (lin // tiles_m, lin % tiles_m)
            m0, n0 = tm * TM, tn * TN
            mprod, mload = frag_rows(akf, VA, m0, M)
            nprod, nload = frag_rows(bkf, VB, n0, Nn)
            acc = None
            for w in range(NW):
                ks = wave_ks(w, kbeg, kend, not akf and not bkf, mutant)
                part = (gather(A, akf, lda, mload, ks).astype(np.float64) @ gather(B, bkf, ldb, nload, ks).astype(np.float64).T
                        ).astype(np.float32)
                acc = part if acc is None else acc + part           # the LDS sum, in wave order
            if not akf and VA > 1:                                  # one VA-wide store per lane, all or nothing
                m_ok = np.repeat((m0 + VA * np.arange(32) + VA) <= M, VA)
            else:
                m_ok = mprod < M
            n_ok = nprod < Nn
            if mutant == "store_clamped":
                m_ok, n_ok = np.ones_like(m_ok), np.ones_like(n_ok)
            if mutant == "cols_last_tile" and tn == tiles_n - 1 and Nn % TN:
                continue
            mask = m_ok[:, None] & n_ok[None, :]
            idx = z * stride + nprod[None, :] * ldo + mprod[:, None]
            out.store(idx[mask], acc[mask])
    return used


def emu_fold(src, splits, M, Nn, out, ldc, stride, mutant=None):
    total = M * Nn
    step = total if (mutant == "fold_stride" or not stride) else stride
    nth = min(ceil_div(total, 256), pc.BLOCK_CAP) * 256
    for it in range(ceil_div(total, nth)):                          # the grid-stride loop
        e = it * nth + np.arange(nth)
        e = e[e < total]
        s = src[e].astype(np.float32)
        for z in range(1, splits - 1 if (mutant == "fold_skip_slab" and splits > 1) else splits):
            s = s + src[z * step + e]
        out.store((e // M) * ldc + e % M, s)


def emu_gemm_bf16(M, Nn, K, A, lda, B, ldb, out, ldo, splits, force_tile, mutant=None):
    used, kchunk, T = pc.bf16_plan(M, Nn, K, splits, force_tile)
    stride = M * Nn if used > 1 else 0
    for z in range(used):
        kbeg, kend = z * kchunk, min((z + 1) * kchunk, K)
        ks = kbeg + np.arange((kend - kbeg) // pc.BF16_KTILE * pc.BF16_KTILE)
        if ks.size == 0:
            continue
        for bx in range(ceil_div(M, T)):
            for by in range(ceil_div(Nn, T)):
                m, n = bx * T + np.arange(T), by * T + np.arange(T)
                At, Bt = np.zeros((T, ks.size)), np.zeros((T, ks.size))     # staged rows past the end are zeros
                At[m < M] = pc.bf16_to_f32(A[m[m < M, None] * lda + ks[None, :]])
                Bt[n < Nn] = pc.bf16_to_f32(B[n[n < Nn, None] * ldb + ks[None, :]])
                if mutant == "cols_last_tile" and by == ceil_div(Nn, T) - 1 and Nn % T:
                    continue
                acc = (At @ Bt.T).astype(np.float32)
                mask = (m < M)[:, None] & (n < Nn)[None, :]
                out.store((z * stride + n[None, :] * ldo + m[:, None])[mask], acc[mask])
    return used


def emu_transpose_pack(src, K, R, ld, out, Kpad, mutant=None):
    conv = pc.bf16_truncate if mutant == "truncate" else pc.bf16_rne
    for bx in range(ceil_div(R, 64)):
        for by in range(ceil_div(Kpad, 64)):
            r, k = np.meshgrid(bx * 64 + np.arange(64), by * 64 + np.arange(64), indexing="ij")
            tile = np.zeros((64, 64), np.float32)
            ok = (k < K) & (r < R)
            tile[ok] = src[k[ok] * ld + r[ok]]
            st = (r < R) & (k < (K if mutant == "kpad_unwritten" else Kpad))
            out.store((r * Kpad + k)[st], conv(tile)[st])


def emu_pack(src, n, out, mutant=None):
    conv = pc.bf16_truncate if mutant == "truncate" else pc.bf16_rne
    nth = min(ceil_div(n, 256), pc.BLOCK_CAP) * 256
    for it in range(ceil_div(n, nth)):
        i = it * nth + np.arange(nth)
        i = i[i < n]
        out.store(i, conv(src[i]))


def emulate(jobs, small_ok=True, bf16_tile=0, mutant=None, reps=2):
    """What one driver process leaves for `jobs` (tests/product_check.hip), with the emulated kernels in place of the library."""
    run = dict(out={}, results={"n_cus": N_CUS})
    for job in jobs:
        p = job.p
        outs = {}
        if job.kind in ("gemm", "gemm_slabs", "gemm_bf16"):
            M, Nn, K, ldc, splits = p["M"], p["Nn"], p["K"], p["ldc"], p["splits"]
            bf16 = job.kind == "gemm_bf16"
            akf, bkf = (True, True) if bf16 else (bool(p["TA"]), not p["TB"])
            if splits < 0:
                splits = pc.bf16_pick_splits(M, Nn, K) if bf16 else pc.regs_pick_splits(akf, bkf, M, Nn, K, N_CUS)
                run["results"][(job.id, 0, "picked")] = run["results"][(job.id, 1, "picked")] = splits
            C = Alloc(ldc * Nn, np.float32, p["sent"]) if (job.kind != "gemm_slabs" or p.get("fold")) else None
            S = Alloc(p["slab_n"], np.float32, p["sent"]) if p["slab_n"] else None
            B = job.B[(0 if mutant == "b_off" else p["b_off"]):]
            want = (pc.bf16_plan(M, Nn, K, splits) if bf16 else pc.regs_plan(akf, bkf, M, Nn, K, splits))[0]
            direct = want == 1 and job.kind != "gemm_slabs"
            tgt, ldo = (C, ldc) if direct else (S, M)
            if bf16:
                used = emu_gemm_bf16(M, Nn, K, job.A, p["lda"], B, p["ldb"], tgt, ldo, splits, bf16_tile, mutant)
            else:
                used = emu_gemm_regs(akf, bkf, M, Nn, K, job.A, p["lda"], B, p["ldb"], tgt, ldo, splits, small_ok, mutant)
            if job.kind == "gemm_slabs":
                run["results"][(job.id, 0, "ret")] = run["results"][(job.id, 1, "ret")] = used
            if C is not None and not direct:
                emu_fold(S.payload(), used, M, Nn, C, ldc, 0, mutant)
            outs = dict(C=C, S=S)
        elif job.kind == "gemm_fold":
            C = Alloc(p["ldc"] * p["Nn"], np.float32, p["sent"])
            emu_fold(job.A, p["splits"], p["M"], p["Nn"], C, p["ldc"], p["stride"], mutant)
            outs = dict(C=C)
        elif job.kind == "transpose_pack_bf16":
            C = Alloc(p["R"] * p["Kpad"], np.uint16, p["sent"])
            emu_transpose_pack(job.A, p["K"], p["R"], p["ld"], C, p["Kpad"], mutant)
            outs = dict(C=C)
        elif job.kind == "pack_bf16":
            C = Alloc(p["n"], np.uint16, p["sent"])
            emu_pack(job.A, p["n"], C, mutant)
            outs = dict(C=C)
        for name, al in outs.items():
            if al is not None:
                assert mutant or al.outside == 0, f"{job.id}: {al.outside} stores outside the allocation of {name}"
                run.setdefault("outside", {})[job.id] = run.get("outside", {}).get(job.id, 0) + al.outside
                for rep in range(reps):
                    run["out"][(job.id, name, rep)] = al.raw.tobytes()
    return run


# ---- the table through the emulation -----------------------------------------------------------------------------------------
SMALL_FAMILIES = ("kss", "ksf", "kff", "fold", "bf16", "tpack", "pack")


TILE_RULES = [(f, v) for f in SMALL_FAMILIES for v in (0, 1) if not v or f in ("kss", "ksf", "kff", "bf16")]


@pytest.mark.parametrize("family,variant", TILE_RULES, ids=[f"{f}-{'large' if v else 'small'}-tiles" for f, v in TILE_RULES])
def test_emulation_passes_every_exact_check(family, variant):
    jobs = [pc.make_job(c) for c in pc.FAMILIES[family]]
    run = emulate(jobs, small_ok=not variant, bf16_tile=128 if variant else 64)
    for job in jobs:
        pc.check_exact(job, run)


@pytest.mark.parametrize("family", ("real_fp32", "real_bf16"))
def test_emulation_passes_the_headline_shapes(family):
    for case in pc.FAMILIES[family]:      # one at a time: the operands of a headline case are tens of megabytes
        job = pc.make_job(case)
        pc.check_exact(job, emulate([job], reps=1), reps=1)


def test_ids_are_unique_and_every_case_says_what_it_reaches():
    ids = [c.id for c in pc.ALL_CASES]
    assert len(ids) == len(set(ids))
    assert all(len(c.what) > 8 for c in pc.ALL_CASES)
    for fam in pc.FAMILIES.values():
        whats = [c.what for c in fam]
        assert len(whats) == len(set(whats)), "two cases of a family claim the same thing"


# ---- mutants -----------------------------------------------------------------------------------------------------------------
BY_ID = {c.id: c for c in pc.ALL_CASES}
MUTANTS = [
    # (mutant, the exact case that must fail, tile rule it runs under, words the failure must carry)
    ("tail", "gemm-ksks-192x80x7-s1", True, "differ from the integer product"),
    ("tail", "gemm-ksks-64x16x17-s2", True, "differ from the integer product"),
    ("wave_group", "gemm-ksks-192x80x64-s1", True, "differ from the integer product"),
    ("fold_skip_slab", "gemm-ksks-192x80x65-s3", True, "C: "),
    ("fold_stride", "fold-192x80-z3-st15396", True, "differ from the integer product"),
    ("store_clamped", "gemm-ksks-192x80x72-s1-ldc196", False, "sentinel words overwritten"),
    ("store_clamped", "gemm-kfkf-80x65x256-s1", True, "sentinel words overwritten"),
    ("cols_last_tile", "gemm-kskf-256x65x48-s1", True, "never written"),
    ("cols_last_tile", "bf16-Y-256x72x64-s1", True, "never written"),
    ("b_off", "bf16-dWhy-256x256x128-s2-off24", True, "differ from the integer product"),
    ("kpad_unwritten", "tpack-K63-R100-ld104-Kpad64", True, "differ from round-to-nearest-even"),
    ("kpad_unwritten", "tpack-K64-R16-ld16-Kpad128", True, "differ from round-to-nearest-even"),
    ("truncate", "pack-257", True, "differ from round-to-nearest-even"),
    ("truncate", "tpack-K100-R256-ld260-Kpad128", True, "differ from round-to-nearest-even"),
]


@pytest.mark.parametrize("mutant,case_id,small_ok,words", MUTANTS, ids=[f"{m[0]}@{m[1]}" for m in MUTANTS])
def test_mutant_fails_the_named_case(mutant, case_id, small_ok, words):
    job = pc.make_job(BY_ID[case_id])
    pc.check_exact(job, emulate([job], small_ok=small_ok))                      # the case passes unmutated ...
    with pytest.raises(AssertionError) as err:                                   # ... and sees the mutant
        pc.check_exact(job, emulate([job], small_ok=small_ok, mutant=mutant))
    assert words in str(err.value), str(err.value)


def test_every_listed_mutant_is_covered():
    assert {m[0] for m in MUTANTS} == {"tail", "wave_group", "fold_skip_slab", "fold_stride", "store_clamped", "cols_last_tile",
                                       "b_off", "kpad_unwritten", "truncate"}


# ---- accuracy ------------------------------------------------------------------------------------------------------------------
def kernel_order(job, rows, cols, small_ok=True):
    """C[cols][rows] in float32 in the kernels' summation order: per slab and wave the k-groups in turn, within a group the
    instructions j = 0..3 each adding k = j and k = 4 + j (the two k-slots of a 32x32x2 instruction); then the waves in order,
    then the slabs in order.  The bf16 product: ascending within a slab (one accumulator per output), then the slabs."""
    p = job.p
    a, b = job.a[rows].astype(np.float32), job.B_logical[cols].astype(np.float32)
    bf16 = job.kind == "gemm_bf16"
    splits = p["splits"]
    if splits < 0:
        splits = pc.bf16_pick_splits(p["M"], p["Nn"], p["K"]) if bf16 else \
            pc.regs_pick_splits(bool(p["TA"]), not p["TB"], p["M"], p["Nn"], p["K"], N_CUS)
    used, kchunk = (pc.bf16_plan(p["M"], p["Nn"], p["K"], splits) if bf16 else
                    pc.regs_plan(bool(p["TA"]), not p["TB"], p["M"], p["Nn"], p["K"], splits, small_ok))[:2]
    total = None
    for z in range(used):
        kbeg, kend = z * kchunk, min((z + 1) * kchunk, p["K"])
        slab = None
        for w in range(1 if bf16 else NW):
            ks = np.arange(kbeg, kend) if bf16 else wave_ks(w, kbeg, kend, True)
            if not bf16:                                    # k = 4h + j: j outer, the k-slot h inner
                full = ks[:len(ks) // 8 * 8].reshape(-1, 2, 4).transpose(0, 2, 1).reshape(-1)
                ks = np.concatenate([full, ks[len(ks) // 8 * 8:]])
            acc = np.zeros((len(cols), len(rows)), np.float32)
            for k in ks:
                acc = acc + b[:, k, None] * a[None, :, k]
            slab = acc if slab is None else slab + acc
        total = slab if total is None else total + slab
    return total


@pytest.mark.parametrize("case", pc.ACC_FP32 + pc.ACC_BF16 + pc.REAL_FP32[:1] + pc.REAL_BF16[1:2], ids=lambda c: c.id)
def test_kernel_order_is_within_the_accuracy_conditions(case):
    job = pc.make_job(case, "accuracy")
    rows, cols = pc.sample_of(job.p["M"], job.p["Nn"], job.p["K"])
    fig = pc.accuracy_figures(job, C_sample=kernel_order(job, rows, cols))
    print(case.id, fig)
    pc.assert_accuracy(job, fig)


def test_a_lost_term_at_k_6336_is_far_outside_the_accuracy_conditions():
    """The accuracy check is not vacuous at large K: the yardstick's own sum with ONE of 6336 terms left out moves both figures
    by more than 100 times their bounds."""
    rng = np.random.default_rng(6336)
    a = rng.standard_normal((64, 6336)).astype(np.float32).astype(np.float64)
    b = rng.standard_normal((64, 6336)).astype(np.float32).astype(np.float64)
    yard = pc.ascending_f32(a, b)
    lost = (yard - (b[:, 4000, None] * a[None, :, 4000]).astype(np.float32)).astype(np.float32)
    ey, el = pc.error_units(yard, a, b), pc.error_units(lost, a, b)
    rms = lambda e: np.sqrt(np.mean(e * e))
    assert rms(el) > 100 * pc.RMS_MARGIN * rms(ey), (rms(el), rms(ey))
    assert el.max() > 100 * pc.MAX_MARGIN * ey.max(), (el.max(), ey.max())


# ---- the contract --------------------------------------------------------------------------------------------------------------
def test_every_case_lies_inside_the_contract():
    for case in pc.ALL_CASES:
        c = pc.case_contract(case)
        if c is not None:
            assert pc.contract_violations(c) == [], case.id


def test_the_contract_refuses_what_the_kernels_cannot_do():
    ok = dict(kind="gemm", TA=0, TB=1, M=64, Nn=16, K=9, lda=64, ldb=16, ldc=64)
    assert pc.contract_violations(ok) == []
    for change in (dict(M=66, lda=66, ldc=66), dict(Nn=15), dict(ldb=17), dict(lda=66), dict(ldc=66), dict(c_off=2), dict(b_off=1),
                   dict(TA=1), dict(TB=0, ldb=16, K=9), dict(K=0), dict(ldc=60)):
        assert pc.contract_violations(dict(ok, **change)), change
    okb = dict(kind="gemm_bf16", TA=0, TB=0, M=5, Nn=3, K=64, lda=64, ldb=72, ldc=5)
    assert pc.contract_violations(okb) == []
    for change in (dict(K=32), dict(lda=68), dict(b_off=4), dict(ldb=56)):
        assert pc.contract_violations(dict(okb, **change)), change


def test_every_product_the_library_issues_lies_inside_the_contract():
    """Over the widths and batches include/lstm_hip.h admits: fp32 at every multiple of 16 (LSTM_HIP_PAD_HIDDEN widths are among
    them), any B >= 1, S >= 2 (T = 1 at S = 2, B = 1); bf16 at multiples of 128 up to 1024 with B a multiple of 8, whose dWhy
    product reads the h image from Ht_b + B."""
    fp32_widths = sorted(set(range(16, 2049, 16)) | {pc.padded_hidden(n) for n in range(1, 1101)} |
                         {pc.padded_hidden(n, step=True) for n in range(1, 200)})
    assert all(w % 16 == 0 for w in fp32_widths)
    n = 0
    for Np in fp32_widths:
        for B in (1, 2, 3, 5, 7, 8, 9, 17, 59, 64, 1024):
            for S in (2, 3, 10, 100):
                for fused in (False, True):
                    for prod in pc.library_products(Np, S, B, fused=fused, du_split=not fused):
                        assert pc.contract_violations(prod) == [], (Np, S, B, prod)
                        n += 1
    for Np in sorted({pc.padded_hidden(n, bf16=True) for n in range(1, 1025)}):
        assert Np % 128 == 0 and 0 < Np <= 1024
        for B in (8, 16, 24, 64, 128, 1000):
            for S in (2, 3, 100):
                for prod in pc.library_products(Np, S, B, bf16=True):
                    assert pc.contract_violations(prod) == [], (Np, S, B, prod)
                    n += 1
    assert pc.padded_hidden(1025, bf16=True) == 0
    assert n > 10000
    # T = 1 is there, and the bf16 base offset is what makes B % 8 a requirement
    assert pc.library_products(16, 2, 1)[0]["Nn"] == 1
    assert pc.contract_violations(pc.library_products(128, 3, 4, bf16=True)[2]) == ["bf16: A, B 16-byte aligned"]


# ---- coverage of the instantiations ------------------------------------------------------------------------------------------
def test_the_table_reaches_every_instantiation_under_the_two_tile_rules():
    seen = {True: set(), False: set()}
    for case in pc.KSS + pc.KSF + pc.KFF:
        p = case.p
        for small_ok in (True, False):
            seen[small_ok].add(pc.regs_plan(bool(p["TA"]), not p["TB"], p["M"], p["Nn"], p["K"], p["splits"], small_ok)[2])
    # every case of the table is small, so the rule alone decides: 64-wide tiles by default, 128-wide with the switch off
    assert seen[True] == {(False, False, 2, 2), (False, True, 2, 2), (True, True, 2, 2)}
    assert seen[False] == {(False, False, 4, 2), (False, True, 4, 2), (True, True, 2, 2)}
    assert seen[True] | seen[False] == pc.INSTANTIATIONS
    # the headline dU takes the 128-wide tile by the rule itself (16 x 8 tiles x 2 slabs), the headline dWhy the 64-wide one
    assert pc.regs_plan(False, False, 2048, 512, 6336, 2)[2] == (False, False, 4, 2)
    assert pc.regs_plan(False, False, 256, 512, 6336, 16)[2] == (False, False, 4, 2)
    assert pc.regs_plan(False, True, 256, 6336, 512, 1)[2] == (False, True, 4, 2)
    for tile in (64, 128):
        assert {pc.bf16_plan(c.p["M"], c.p["Nn"], c.p["K"], c.p["splits"], tile)[2] for c in pc.BF16} == {tile}
    assert {pc.bf16_plan(c.p["M"], c.p["Nn"], c.p["K"], c.p["splits"])[2] for c in pc.BF16} == {64}   # why the switch is needed


def test_split_rules():
    assert pc.regs_plan(False, False, 64, 16, 17, 2)[:2] == (2, 16)      # second slab: one term
    assert pc.regs_plan(False, False, 192, 80, 9, 8)[:2] == (2, 8)       # a request larger than K / 8
    assert pc.regs_plan(False, False, 64, 16, 72, 8)[:2] == (5, 16)
    assert pc.bf16_plan(256, 128, 320, 2)[:2] == (2, 192)                # slabs of 192 and 128
    assert pc.bf16_plan(256, 56, 128, 3)[:2] == (2, 64)
    assert pc.regs_pick_splits(False, False, 2048, 512, 6336, 256) == 2
    assert pc.regs_pick_splits(False, False, 256, 512, 6336, 256) == 16
    assert pc.bf16_pick_splits(2048, 512, 6336) == 4 and pc.bf16_pick_splits(256, 512, 6336) == 16
    assert pc.bf16_plan(256, 512, 6336, 16)[:2] == (15, 448)             # the bf16 rule is an upper bound: whole k-tiles per slab
