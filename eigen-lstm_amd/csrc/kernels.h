// kernels.h -- launch wrappers of the gfx950 kernels (kernels.hip), used by lstm_hip_api.cpp.
// Every wrapper enqueues on `st` and returns; no host synchronisation, no allocation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "heads/head_args.h"

namespace lstmk {

// flat parameter block offsets [W | U | b | Why | by], floats
struct ParamLayout {
    size_t W, U, b, Why, by, total;
    __host__ __device__ static ParamLayout make(int N, int M) {
        ParamLayout p;
        p.W = 0;
        p.U = p.W + (size_t)4 * N * M;
        p.b = p.U + (size_t)4 * N * N;
        p.Why = p.b + (size_t)4 * N;
        p.by = p.Why + (size_t)M * N;
        p.total = p.by + (size_t)M;
        return p;
    }
};

// ---- the request for dynamic LDS: the one place a kernel is granted more than a launch gets unasked ----------------------
// A refused request is returned.  A launcher that returns hipError_t passes it on and launches nothing; a void launcher may
// drop it: the launch it then makes is refused too, and the caller's launch check reports that.
template <class K> inline hipError_t request_lds(K kernel, size_t bytes) {
    return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
// The same behind a cache: above FLOOR (what needs no request) the size is requested of the kernel first, and the largest
// request that went through is remembered per kernel instantiation and per device.  The device is the calling thread's
// current one, which every entry point of lstm_hip_api.cpp notes here as it sets it (so a cached launch asks the runtime
// nothing, as before the table had a device); a device the table has no row for is asked every time.
extern thread_local int lds_device; // (kernels.hip; 0 until an entry point says otherwise)
template <auto KERNEL, size_t FLOOR> inline hipError_t grant_lds(size_t lds) {
    constexpr int kDevices = 128;
    static size_t granted[kDevices] = {};
    if (lds <= FLOOR) return hipSuccess;
    const int dev = lds_device;
    if (dev < 0 || dev >= kDevices) return request_lds(KERNEL, lds);
    if (lds > granted[dev]) {
        if (const hipError_t e = request_lds(KERNEL, lds)) return e;
        granted[dev] = lds;
    }
    return hipSuccess;
}

// ---- which form of each recurrence a handle runs (plan_engine, persistent.hip) ------------------------------------------
// Decided once per handle at create from the shape, the create flags and the CU count; every launch of the window follows it.
enum class FwdForm {
    Step,       // one fwd_step launch per timestep (LSTM_HIP_STEP_KERNELS, or no co-resident persistent grid)
    Small,      // k_small_fwd: one stream at hidden 64 / 128, the whole recurrence on one CU
    Persistent, // fwd_persistent: one recurrence on 16x16x4 tiles (k_fwd_persistent / k_fwd_persistent2), image Ufwd
    Cols8,      // fwd_persistent4: 8-column groups on 4x4x1, image Ufwd4, ring Hx
    TwoHalf,    // fwd_persistent6: two alternating 4-column halves per group, Ufwd4 in the Ufwd5 layout, ring Hx; column launches
    Bf16,       // fwd_persistent_bf16: the bf16 one-recurrence forms, image Ufwd16
    Bf16Halves, // fwd_halves_bf16: the bf16 two-half form, image Ufwd6b, ring Hxb; column launches
};
enum class BwdForm {
    Step,        // one bwd_step launch per timestep
    Small,       // k_small_bwd (reads the tile image Ubwd)
    Persistent,  // bwd_persistent on 16-column groups, 16x16x4 tiles, image Ubwd
    Cols8,       // bwd_persistent on 8-column groups, 4x4x1, image Ubwd4
    Scatter,     // bwd_scatter: two-half scatter form, Ubwd4 in the Ubwd6 layout, partial-sum ring DGx; column launches
    Bf16,        // bwd_persistent on the bf16 image Ubwd16 (4-, 8- or 16-column groups)
    Bf16Scatter, // bwd_scatter_bf16: image Ubwd6b, ring DGx; column launches
};
struct EnginePlan {
    FwdForm fwd = FwdForm::Step;
    BwdForm bwd = BwdForm::Step;
    int n_cus = 0;
    bool fused = false;     // dW / db / dWhy (and Why^T dy) inside the backward recurrence, as per-group partial blocks (gpart)
    int bwd_cols = 16;      // batch columns per workgroup of bwd_persistent (Persistent, Cols8, Bf16)
    int gpart_cols = 8;     // batch columns per fused partial block
    int fwd_cols = 16;      // Bf16 forward: 8- or 16-column groups
    // the multi-launch forms (TwoHalf, Scatter, Bf16Halves, Bf16Scatter): one launch per `launch_cols` columns of the batch,
    // `group_cols` (4 or 8) columns per group; a launch of fewer than 8 groups is pinned one group per XCD where *_pin
    int launch_cols = 0, group_cols = 8;
    bool fwd_pin = false, bwd_pin = false;
    int poll_cfg = 0;         // Cols8 / TwoHalf: bits 0-7 s_sleep between polls, 8-15 first delay of the non-gating waves
    int bwd_cfg = 0;          // Scatter: the kernel's tuning / test bits (LSTM_HIP_BWD_HALVES >> 1)
    bool bwd_spread = false;  // LSTM_HIP_BWD_SPREAD: keep the dispatch-order workgroup mapping of the backward recurrence
    bool side_stream = false; // unfused Scatter: the sums that do not feed the recurrence run on the second stream beside it
    bool direct_dgt = false;  // Bf16Scatter: the recurrence writes the k-contiguous bf16 image of dg for the dU product
    bool adagrad_quad = false; // Adagrad refreshes the two-half images (Ufwd5 + Ubwd6, or Ufwd6b) with quad transposes
    bool du_split = false;    // LSTM_HIP_DU_SPLIT (fp32, communicator loop): dU as two column halves, the first reduced early
    bool stamps = false;      // LSTM_HIP_DEBUG_STAMPS on a shape whose forms carry stamps
    unsigned epoch_limit = 1u << 26; // LSTM_HIP_EPOCH_LIMIT: a recurrence that has made this many launches on the cumulative
                                     // hand-off counters clears them and restarts its epoch (do_forward / do_backward)
    // live images and rings (sizes in elements; 0: none)
    size_t hx_floats = 0;        // Hx
    size_t hxb_halfwords = 0;    // Hxb
    size_t dgx_floats = 0;       // DGx
    bool u16 = false;            // Ufwd16 / Ubwd16 (a bf16 one-recurrence form runs)
    char refusal[192] = "";      // non-empty: the shape cannot run; the reason
    bool bf16() const { return fwd == FwdForm::Bf16 || fwd == FwdForm::Bf16Halves; }
    bool persistent() const { return fwd != FwdForm::Step; }
    bool ufwd4() const { return fwd == FwdForm::Cols8 || fwd == FwdForm::TwoHalf; }
    bool ubwd4() const { return bwd == BwdForm::Cols8 || bwd == BwdForm::Scatter; }
    int half_forms() const { return (fwd == FwdForm::TwoHalf ? 1 : 0) | (bwd == BwdForm::Scatter ? 4 : 0); } // layouts of Ufwd4 / Ubwd4
};
EnginePlan plan_engine(int N, int B, unsigned flags, int n_cus);

// ---- recurrent weight repack (once per window, after Adagrad) -------------------------------
// Ufwd[N/4][N/16][64] float4 : MFMA 16x16x4 A-fragments of U for the forward product
// Ubwd[N/16][N/4][64] float4 : A-fragments of U^T for the backward product
// Ubwd4 / Ufwd4 (optional): the 4x4x1 images of the 8-column backward / forward forms; half_forms: Ufwd4 receives the
// image of the two-half forward form (k_fwd_persistent6) instead
void pack_U(const float *U, float4 *Ufwd, float4 *Ubwd, int N, hipStream_t st, float4 *Ubwd4 = nullptr,
            float4 *Ufwd4 = nullptr, int half_forms = 0);

// ---- baseline engine: one launch per timestep -----------------------------------------------
// g = U*h_prev + W[:,x] + b ; gates ; c = tanh(i*u + f*c_prev) ; h = o*c      (R/lstm.cc:176-192)
void fwd_step(const float4 *Ufwd, const float *W, const float *bias, const float *Hprev, const float *Cprev,
              float *Hout, float *Cout, float *Gout, const int32_t *xi_t, int N, int B, bool fast, hipStream_t st);
// dh = DHy[t] + U^T*dg[t+1] ; dc ; dg[t] ; dcnext                              (R/lstm.cc:228-256)
void bwd_step(const float4 *Ubwd, const float *DGnext /*null at t=S-1*/, const float *DHy_t, const float *G_t,
              const float *C_t, const float *Cprev, float *dcnext, float *DG_t, int N, int B, hipStream_t st);

// ---- default engine: each recurrence of a window as ONE persistent launch (persistent.hip) ----
// Weights stay in VGPRs; the steps are chained inside the launch.  Hand-off, by form:
//   8-column forward form and (optionally) the fp32 4x4x1 backward form: data-as-flag through a ring of sentinel-filled
//     step slots (Hx / DGx; EnginePlan sizes, filled with 0xFF bytes once and after an abort; ring_base starts at 0
//     and moves by *_ring_advance() after every launch);
//   every other form: sc1 stores + sharded device-scope counters.  `cnt` must hold persistent_counter_bytes() bytes
//     (separate regions for fwd and bwd), zeroed once; `epoch` = 1, 2, ... counts the launches that used that region
//     (counters are cumulative).  The ring forms use the step-0 slots of `cnt` for their XCD placement check.
// `abortp` is one zeroed word that a timed-out spin sets.  `stamps` (diagnostic builds, N = 512 only): [2][S][16] u64.
// The multi-launch forms take columns [col0, col0 + cols) of the batch per launch, in groups of `gc` columns; `pin`: a launch
// of fewer than 8 groups runs pinned, one group per XCD (EnginePlan).
size_t persistent_counter_bytes(int S, int B);
void fwd_persistent(const float4 *Ufwd, const float *W, const float *bias, float *H, float *C, float *G,
                    const int32_t *xi, unsigned *cnt, unsigned *abortp, unsigned epoch, int N, int S, int B, bool fast,
                    hipStream_t st);
int fwd_ring_advance(int ring_base, int S);
void fwd_persistent4(const float4 *Ufwd4, const float *W, const float *bias, float *H, float *C, float *G, const int32_t *xi,
                     float *Hx, unsigned *cnt, unsigned *abortp, unsigned epoch, int ring_base, int N, int S, int B, bool fast,
                     int poll_cfg, hipStream_t st, unsigned long long *stamps = nullptr);
// two-half form (N = 512 / 256): the same ring, each group's eight columns advanced as two alternating 4-column recurrences
// (or one, gc = 4); weights in the Ufwd5 image (pack_U / adagrad with half_forms)
void fwd_persistent6(const float4 *Ufwd5, const float *W, const float *bias, float *H, float *C, float *G, const int32_t *xi,
                     float *Hx, unsigned *cnt, unsigned *abortp, unsigned epoch, int ring_base, int N, int S, int B, bool fast,
                     int poll_cfg, int col0, int cols, int gc, bool pin, hipStream_t st, unsigned long long *stamps);
// two-half (scatter) form of the backward recurrence (N = 512 / 256, 8-column groups): every workgroup advances its eight
// columns as two alternating 4-column recurrences, multiplies its OWN dg_t into partial sums for all N outputs and scatters
// them to the owners of the outputs.  Ubwd6 image (pack_U / adagrad with bit 2 of half_forms), partial-sum ring Qx
// (sentinel-filled like the other rings; ring_base moves by bwds_ring_advance); computes Why^T dy itself; gpart != null:
// fused mode as below.  cfg: tuning / test bits (16: keep the dispatch-order workgroup mapping).
int bwds_ring_advance(int ring_base, int S);
void bwd_scatter(const float4 *Ubwd6, float *DG, const float *Why, const float *dY, const float *G, const float *C, const float *H,
                 const int32_t *xi, float *gpart, float *Qx, unsigned *cnt, unsigned *abortp, unsigned epoch, int ring_base, int N,
                 int S, int B, int cfg, int col0, int cols, int gc, bool pin, hipStream_t st, unsigned long long *stamps);
// gpart != null (8-column groups only): fused mode.  The recurrence then also produces DHy on the fly from
// Why and dY (DHy is not read), and leaves per-column-group partial blocks [dW | - | db | dWhy]
// (bwd_partial_floats(N) floats each) to be folded in group order; H and xi are read as well.  spread: keep the
// dispatch-order workgroup mapping (column groups over all XCDs).
void bwd_persistent(const float4 *Ubwd, float *DG, const float *DHy, const float *G, const float *C, const float *H,
                    const int32_t *xi, float *gpart, const float *Why, const float *dY, unsigned *cnt, unsigned *abortp,
                    unsigned epoch, int N, int S, int B, int cols, bool spread, hipStream_t st, unsigned long long *stamps = nullptr,
                    unsigned short *DGb = nullptr);
// bf16 recurrence (N % 128 == 0): bf16 fragment images of U (N*N*8 bytes each), h and dg also kept as bf16
// hand-off copies Hb [S][B][N], DGb [S][B][4N]; bwd_persistent takes the Ubwd16 image as `Ubwd` and DGb != null
void pack_U_bf16(const float *U, void *Ufwd16, void *Ubwd16, int N, hipStream_t st);
void fwd_persistent_bf16(const void *Ufwd16, const float *W, const float *bias, float *H, unsigned short *Hb, float *C,
                         float *G, const int32_t *xi, unsigned *cnt, unsigned *abortp, unsigned epoch, int N, int S, int B,
                         bool fast, int cols, hipStream_t st);
// scatter form of the bf16 backward recurrence (N = 256 / 512 / 1024): Ubwd6b image (pack_U6_bf16, N*N*8 bytes), partial-sum
// ring Qx as in bwd_scatter; reads DHy (a launch of its own in the bf16 path), writes the fp32 DG
void pack_U6_bf16(const float *U, void *Ubwd6b, int N, hipStream_t st);
// two-half form of the bf16 forward recurrence (k_fwd_halves_bf16): weights image Ufwd6b (N*N*8 bytes), bf16 sentinel ring Hxb
// (all ones at rest; slots advance with fwd_ring_advance)
void pack_Ufwd6_bf16(const float *U, void *img, int N, hipStream_t st);
void fwd_halves_bf16(const void *Ufwd6b, const float *W, const float *bias, float *H, unsigned short *Hb, float *C, float *G,
                     const int32_t *xi, void *Hxb, unsigned *cnt, unsigned *abortp, unsigned epoch, int ring_base, int N, int S,
                     int B, int col0, int cols, int gc, bool pin, bool fast, hipStream_t st, unsigned long long *stamps);
int bwd_scatter_bf16_units(int N);
int bwd_scatter_bf16_ring_advance(int base, int S);
void bwd_scatter_bf16(const void *Ubwd6b, float *DG, const float *DHy, const float *G, const float *C, float *Qx, unsigned *cnt,
                      unsigned *abortp, unsigned epoch, int ring_base, int N, int S, int B, int col0, int cols, int gc, bool pin,
                      hipStream_t st, unsigned long long *stamps, unsigned short *DGt_b = nullptr, int Tpad = 0);
// one stream, hidden 64 / 128: both recurrences on one CU (k_small_fwd, k_small_bwd); they read U and Why as stored, write H, C,
// G and DG (the backward one reads U from the Ubwd tile image); the backward one computes Why^T dy itself (no DHy), dW / db / dWhy / dU are the unfused path's launches
void small_fwd(const float *U, const float *W, const float *bias, float *H, float *C, float *G, const int32_t *xi, int N, int S, bool fast,
               hipStream_t st);
void small_bwd(const float4 *Ubwd, const float *Why, const float *dY, const float *G, const float *C, float *DG, int N, int S, hipStream_t st);
size_t bwd_partial_floats(int N);

// ---- time-batched dense products (gemm.hip: fp32 MFMA 32x32x2, operands streamed into registers, K split over the waves
//      of a workgroup) --------------------------------------------------------------------------
// C[M x Nn] = op(A)[M x K] * op(B)[K x Nn], column-major; TA: A is stored K x M; TB: B is stored Nn x K.  (TA && TB is
// not a product of the window and is refused.)  splits > 1 writes partial slabs into `slabs` (each M*Nn floats, ld = M)
// and gemm_fold sums them into C in slab order (deterministic).  `slabs` must hold splits*M*Nn floats.
//
// Contract (nothing below is checked at run time; tests/product_cases.py contract_violations() is this list as code, and
// tests/test_products_cpu.py holds every product do_forward / do_backward issue against it).  An operand is "k fast" when the
// contraction index is its contiguous one -- A when TA, B when !TB -- and "k slow" otherwise.
//   forms     (TA, TB) = (0, 1) k slow x k slow (dU, dWhy), (0, 0) k slow x k fast (Y), (1, 0) k fast x k fast (DHy).
//             (1, 1) does not exist: gemm launches nothing, gemm_slabs / gemm_regs return -1.
//   K         any K >= 1 when both operands are k slow (the K % 8 tail is a predicated group); K % 8 == 0 as soon as one
//             operand is k fast (a tail would be dropped silently).  splits: any value; fewer slabs may be used, K is cut in
//             multiples of 8 (the count is gemm_slabs' return value, and gemm_pick_splits' values are returned unchanged).
//   k-slow A  a lane loads and STORES four consecutive rows (two with the small tile) as one vector and clamps the last
//             vector to row M - 4: M % 4 == 0, M >= 4, lda % 4 == 0, lda >= M, A 16-byte aligned; and for C: ldc % 4 == 0,
//             C 16-byte aligned.  (Rows M - M % 4 .. M - 1 of another M would never be stored.)
//   k-slow B  two consecutive rows per lane, the last pair clamped to row Nn - 2: Nn % 2 == 0, Nn >= 2, ldb % 2 == 0,
//             ldb >= Nn, B 8-byte aligned.
//   k-fast    16-byte loads of four consecutive k, rows clamped to the last one: any row count >= 1 (M for A, Nn for B),
//             ld % 4 == 0, ld >= K, base 16-byte aligned.  A k-fast A stores C one float at a time: any ldc >= M, any C.
//   C         ldc >= M; rows M .. ldc-1 of a column are never written.  slabs: 16-byte aligned, M*Nn floats each, ld = M.
//   sizes     lane and k-group offsets are 32-bit: (K - 1) * ld + rows (k slow) or (rows - 1) * ld + K (k fast) < 2^32.
//   reads     only the elements the layout spans: k < K and rows < M / Nn of every line, never the rest of a line of ld.
void gemm(bool TA, bool TB, int M, int Nn, int K, const float *A, int lda, const float *B, int ldb, float *C, int ldc,
          int splits, float *slabs, hipStream_t st);
// how many slabs the shape rule wants (1: no slabs); a static function of the shape and the device's compute-unit count
int gemm_pick_splits(bool TA, bool TB, int M, int Nn, int K, int n_cus);
// the ordered fold of `splits` slabs
// slab_stride: floats between consecutive slabs (0 = M*Nn, i.e. densely packed)
void gemm_fold(const float *slabs, int splits, int M, int Nn, float *C, int ldc, hipStream_t st, size_t slab_stride = 0);
// the split-K product without its fold (slabs densely packed, M*Nn floats each); returns the number of slabs written
int gemm_slabs(bool TA, bool TB, int M, int Nn, int K, const float *A, int lda, const float *B, int ldb, float *slabs, int splits,
               hipStream_t st);
// the same by operand layout ("k fast": the contraction index is the contiguous one); gemm / gemm_slabs map onto these
int gemm_regs_splits(bool a_kfast, bool b_kfast, int M, int Nn, int K, int n_cus);
int gemm_regs(bool a_kfast, bool b_kfast, int M, int Nn, int K, const float *A, int lda, const float *B, int ldb, float *C, int ldc,
              int splits, float *slabs, hipStream_t st);

// ---- bf16 time-batched products (LSTM_HIP_BF16_RECURRENCE): C[m + ldc*n] = sum_k A[m][k] * B[n][k], fp32 accumulate on
//      v_mfma_f32_32x32x16_bf16.  A, B: bfloat16, k contiguous (lda, ldb in elements, multiples of 8; 16-byte aligned
//      bases), K a multiple of 64 (zero-padded images).  transpose_pack_bf16 builds such an image from a column-major fp32
//      matrix whose COLUMNS are the contraction index: dst[r][k] = bf16(src[k*ld + r]), zero for K <= k < Kpad.
void gemm_bf16(int M, int Nn, int K, const unsigned short *A, int lda, const unsigned short *B, int ldb, float *C, int ldc,
               int splits, float *slabs, hipStream_t st);
int gemm_bf16_pick_splits(int M, int Nn, int K);
void transpose_pack_bf16(const float *src, int K, int R, int ld, unsigned short *dst, int Kpad, hipStream_t st);
void pack_bf16(const float *src, size_t n, unsigned short *dst, hipStream_t st);

// ---- output layer elementwise: probs = exp(y+by)/sum ; loss ; dy = probs - onehot  (R/lstm.cc:195-207,225)
// Y is [T cols][256] (column-major 256 x T) and is overwritten by dY; probs written to P.
// colloss[col] = -log2 p[target] (0 for an empty target); dby_part[wave][256] partial row sums of dY.
// stable: the max-shifted form of LSTM_HIP_STABLE_SOFTMAX (probs = exp(z - max z)/sum, log-sum-exp surprisal).
// Processes columns [col0, col1) (col0 a multiple of 8) with global indexing, so a window can be done in time chunks.
// P null: the probabilities are not stored (dy, the losses and the dby partials are unchanged).
int softmax_parts(int T);
void softmax_loss_dy(float *Y, float *P, const float *by, const int32_t *ti, float *colloss, float *dby_part, int col0,
                     int col1, bool stable, hipStream_t st); // stable: LSTM_HIP_STABLE_SOFTMAX (kernels.hip)
// the variant of the text windows (lstm_hip_train_text_windows): a column with an empty target gets
// dy = 0 (and colloss = 0) instead of dy = probs, so a row without a target adds nothing to any gradient.  Everything else,
// the order of every sum included, is softmax_loss_dy's.
void softmax_loss_dy_text(float *Y, float *P, const float *by, const int32_t *ti, float *colloss, float *dby_part, int col0,
                          int col1, bool stable, hipStream_t st);
// the text variant with a weight per column (lstm_hip_set_train_texts_weighted): wt[col] is the weight
// of the column's target, laid out like ti.  A column with a target gets dy = wt * (probs - target) and colloss = wt *
// surprisal (one fp32 multiply each behind the text variant's value); wt == 0 selects dy = +0 and colloss = 0 whatever probs
// holds; a column without a target is the text variant's.  wt == 1 everywhere gives the text variant's bytes.
void softmax_loss_dy_weighted(float *Y, float *P, const float *by, const int32_t *ti, const float *wt, float *colloss,
                              float *dby_part, int col0, int col1, bool stable, hipStream_t st);
// the launch with soft targets (lstm_hip_set_soft_targets): probs, colloss, the dby_part rows and the
// column ranges are softmax_loss_dy's; dy = alpha * (probs - r) + oma_tau * (softmax(z / tau) - softmax(zT / tau)) with
// r = ome * onehot + eps256 (0 in a column without a target) and zT = Yt + by_t the teacher's logits of the same column.
// Yt null: no teacher, dy = probs - r (alpha is 1 then).  colkl[col] = KL(q || p_tau) of the column in bits (teacher only).
struct SoftTargetArgs {
    const float *Yt;   // the teacher's logit block at the window's first column, [T][256]; null: no teacher
    const float *by_t; // the teacher's by
    float *colkl;      // [T]
    float alpha, oma_tau, inv_tau; // alpha, (1 - alpha) * tau, 1 / tau
    float ome, eps256;             // 1 - eps, eps / 256
    bool tempered;                 // tau != 1: p_tau is a second, max-shifted softmax of z / tau
};
void softmax_soft(float *Y, float *P, const float *by, const int32_t *ti, float *colloss, float *dby_part, int col0, int col1,
                  bool stable, const SoftTargetArgs &a, hipStream_t st);
// window loss as the reference sums it: for each t a float sum over b, / B_global, accumulated in double;
// when dby != null a second workgroup folds the per-wave partials into dby = rowsum(dY) (R/lstm.cc:227)
void loss_reduce(const float *colloss, int steps, int B, int B_global, double *out, const float *dby_part, int n_parts,
                 float *dby, hipStream_t st, float scale = 1.0f);

// ---- dW = DG * X^T and db = rowsum(DG)                                        (R/lstm.cc:251-252)
// X is one-hot, so dW[:,v] is the sum of the DG columns whose input byte is v (bucket 256 = empty
// input column); db[r] = sum over the 257 buckets.  Stable counting sort of the column ids, ordered
// chunk sums, ordered folds: deterministic.  `scratch` must hold dW_scratch_bytes(T, G4).
constexpr int DW_CHUNK = 32;
size_t dW_scratch_bytes(int T, int G4);
void dW_db(const float *DG /*[T][G4]*/, const int32_t *xi /*[T]*/, int T, int G4, float *dW /*[256][G4]*/, float *db,
           void *scratch, hipStream_t st);
// the same in two parts: the sort needs only the input bytes, the sums need the complete DG
void dW_sort(const int32_t *xi, int T, int G4, void *scratch, hipStream_t st);
void dW_sums(const float *DG, int T, int G4, float *dW, float *db, void *scratch, hipStream_t st);

// ---- Adagrad over the flat block (R/lstm.cc:261-272; eps added in double, :25,46-48)
// the NEXT window's slide (slide_window's arguments), carried by an Adagrad launch in extra workgroups: inside the window loop
// the slide of window i+1 needs nothing Adagrad of window i produces and touches nothing it reads.  Several workgroups share
// it without waiting for each other, so the cursors and the ring head are read from pos / headp and the new ones written to
// pos_out / head_out (other memory: the caller flips its live copies after the launch); the result is slide_window's.
struct SlideJob {
    const uint8_t *text;
    uint64_t len;
    const uint64_t *pos;
    int32_t *Xr, *Tr;
    const int32_t *headp;
    int32_t *xi, *ti;
    float *H, *C;
    int S, B, N, stride, carry_col;
    uint64_t *pos_out;
    int32_t *head_out;
};
// the window's loss sum and dby fold (loss_reduce's arguments), carried by the update launch of the same window in extra
// workgroups: same sums in the same order; dby goes to dP and the carrying workgroups update by themselves
struct TailJob {
    const float *colloss;
    int steps, B, B_global;
    float scale;
    double *loss_out;
    const float *dby_part;
    int n_parts;
};
// One Adagrad launch: the update of the flat block P / dP / mem (n floats, U at float offset u_off) and what it carries:
//  - the live images of U, refreshed from the updated block: fp32 Ufwd / Ubwd (16x16x4 tiles) and Ufwd4 / Ubwd4 in the
//    layouts half_forms names (pack_U); bf16 u6b (scatter-form backward image, u6_uw units per workgroup) and uf6b (two-half
//    forward image, quad launches only); Why as bf16 in place order and transposed (why_off: float offset of Why); null: none
//  - gpart != null: the gradient still in pieces -- n_groups partial blocks [dW | - | db | dWhy] group_stride floats apart and,
//    when slabs != null, n_slabs split-K slabs of dU slab_stride floats apart; they are summed here in the order the separate
//    folds use and the sums are also stored to dP (by_off: float offset of dby, final in dP)
//  - skip_dP_store: the sums of the pieces are used but not stored (nobody reads dP before the next window overwrites it)
//  - tail: this window's loss sum and dby fold (or null; needs by_off); slide: the next window's slide (or null); quad: the two-half images (Ufwd4 + Ubwd4 with half_forms 5, or uf6b) are
//    written through quad transposes
//  - v != null: the update is Adam with decoupled weight decay (lstm_hip_set_optimizer) instead of Adagrad: mem holds the
//    first moment m, v the second moment, and `adam` the step's scalars, computed in double on the host and narrowed:
//      p = p * decay; m = m + omb1 * (d - m); v = b2 * v + omb2 * d^2; p = p - step * m / (sqrt(v) / bc2s + eps)
struct AdamScalars {
    float decay;     // 1 - lr * weight_decay (1 when weight_decay is 0)
    float omb1;      // 1 - beta1
    float b2, omb2;  // beta2, 1 - beta2
    float step;      // lr / (1 - beta1^t)
    float bc2s;      // sqrt(1 - beta2^t)
    float eps;
};
struct AdagradJob {
    float *P, *dP, *mem;
    size_t n, u_off;
    int N;
    float lr;
    float4 *Ufwd, *Ubwd, *Ubwd4, *Ufwd4;
    int half_forms;
    void *u6b, *uf6b;
    int u6_uw, uf6_uw;
    unsigned short *why_b, *whyT_b;
    size_t why_off;
    const float *gpart, *slabs;
    int n_groups, n_slabs;
    size_t group_stride, slab_stride, by_off;
    const SlideJob *slide;
    const TailJob *tail;
    bool skip_dP_store;
    bool quad;
    const float *clip; // global-norm clipping: the coefficient grad_norm wrote (the step uses d * coef where coef < 1); null: off
    float *v;          // Adam's second moment (n floats); null: Adagrad
    AdamScalars adam;
};
void adagrad(const AdagradJob &job, hipStream_t st);
// ---- global gradient norm (lstm_hip_set_grad_clip), before the clipped Adagrad launch: grad_sumsq takes the block of `job`
// (dP, or the fold pieces job.gpart / job.slabs, which it sums into dP in the order adagrad uses) and writes
// grad_norm_parts(job.n) double partials of sum d^2 in a fixed order; grad_norm adds them, writes the norm to *norm_out and
// the float coefficient max_norm / (norm + 1e-6) (1 where it is not below 1) to *coef_out.  Deterministic: no atomics.
int grad_norm_parts(size_t n);
void grad_sumsq(const AdagradJob &job, double *part, hipStream_t st);
void grad_norm(const double *part, int n_parts, double max_norm, double *norm_out, float *coef_out, hipStream_t st);
// ---- gradient accumulation (lstm_hip_set_grad_accumulation), one launch per window in place of (all but the last window of a
// cycle) or in front of (the last) the update: g is the window's gradient of `job` as grad_sumsq forms it -- job.dP, or the
// fold pieces job.gpart / job.slabs summed in the same order -- and acc the handle's accumulator of job.n floats.
//   GRAD_ACC_FIRST  acc = g            and g is left in dP
//   GRAD_ACC_ADD    acc = acc + g      and g is left in dP
//   GRAD_ACC_LAST   dP = acc + g, then (scale) dP = dP * w: fp32, separately rounded, no FMA; acc is only read
// The update's grid of 256-thread workgroups over float4; plain vector loads and stores, no LDS, no atomics.
enum { GRAD_ACC_FIRST = 0, GRAD_ACC_ADD = 1, GRAD_ACC_LAST = 2 };
void grad_accumulate(const AdagradJob &job, float *acc, int mode, bool scale, float w, hipStream_t st);
int fwd_halves_bf16_units(int N);

// ---- window builder on the device (OV/lstm_eigen_opt/lstm.cc:190-213): x/target rings + flat copies,
//      cursor advance, and the h/c carry (column 1 -> column 0).  Single workgroup.
void slide_window(const uint8_t *text, uint64_t len, uint64_t *pos, int32_t *Xr, int32_t *Tr, int32_t *headp,
                  int32_t *xi, int32_t *ti, float *H, float *C, int S, int B, int N, int stride, int carry_col,
                  hipStream_t st);

// ---- logical <-> padded hidden width (LSTM_HIP_PAD_HIDDEN), at the ABI boundary only.  A buffer is a list of pieces, each a
//      column-major matrix whose columns are `blocks` row blocks of rows_l (logical) / rows_p (padded) rows: W, U and b have
//      the four gate blocks, Why and by one block of 256 rows.  Padded: cols_p >= cols_l columns of blocks * rows_p rows.
//      to_padded: every float of the padded buffer is written, the padding entries as 0; else the logical buffer is gathered
//      from the padded one.  One launch.
constexpr int PAD_MAX_PIECES = 5;
struct PadPiece {
    size_t off_l, off_p; // float offsets of the piece in the logical / padded buffer
    int blocks, rows_l, rows_p, cols_l, cols_p;
};
struct PadMap {
    PadPiece piece[PAD_MAX_PIECES]; // in buffer order
    int n;
    size_t total_l, total_p;
};
PadMap pad_map_params(int N, int Np, int M);              // the flat block [W | U | b | Why | by]
PadMap pad_map_rows(int blocks, int N, int Np, int cols); // `cols` columns of `blocks` x N rows (h, c: 1; g: 4)
void pad_copy(const float *src, float *dst, const PadMap &map, bool to_padded, hipStream_t st);

// ---- running weight average (lstm_hip_set_averaging): one launch of its own after the update launch, on due updates only.
//      copy: a <- p, no arithmetic (the first due update); else a <- a + w * (p - a) in fp32, three separately rounded
//      operations, no FMA.  p and a are 16-byte aligned blocks of n floats that do not overlap; at most 8 * cus workgroups
//      of 256 threads stride over them in float4.  Plain vector loads and stores only.
void average(const float *p, float *a, size_t n, float w, bool copy, int cus, hipStream_t st);

// ---- weight drop (lstm_hip_set_weight_drop; the rule is weight_drop.h): dst <- keep ? src * scale : +0.0f over the internal
//      4Np x Np matrix U, whose logical part is 4Nl x Nl (Nl <= Np, Np % 16 == 0); padding entries are written as 0.  src
//      and dst are 16-byte aligned and either equal or disjoint.  One launch of at most 8 * cus workgroups of 256 threads,
//      plain vector loads and stores only.  Used on P.U -> Ue before the packers and on dP.U in place behind the dU product.
void weight_drop_mask(const float *src, float *dst, int Np, int Nl, uint64_t seed, uint64_t t, uint32_t thr, float scale, int cus,
                      hipStream_t st);

// ---- many texts on the lanes of the forward path (lstm_hip_eval_texts, lstm_hip_embed_texts; DESIGN.md sections 3.17 and
//      3.23; the kernels are text_lanes.hip), around the unchanged forward path of an internal handle with S = EVAL_STEPS + 1
//      and B = lanes.  slot[w * lanes + l] is the stream lane l holds in window w (-1: idle); that window holds steps
//      j0 .. j0 + EVAL_STEPS - 1 of stream s, j0 = EVAL_STEPS * (w - first[s]), in rows 1 .. EVAL_STEPS.  Stream s has
//      L = off[s + 1] - off[s] bytes.  The rule: step j feeds byte j; it exists iff j + 1 < L + feed_last, and it has a target,
//      byte j + 1, iff j + 1 < L && j + 1 >= skip[s].  feed_last = 0 (eval_texts): L - 1 steps, the last byte is a target
//      only.  feed_last = 1 (embed_texts): L steps, the last byte is fed too, row r + 1 holds position j0 + r, the state
//      after inputs 0 .. j0 + r, and the plan tables come from offsets that count every stream one byte longer; off / skip
//      are the caller's.
//      lane_window writes rows 1 .. of xi / ti (input byte j, target byte j + 1, each -1 where the rule gives none or on an
//      idle lane) and column 0 of H / C of every busy lane: the stream's column of H0 / C0 in its first window, else column
//      EVAL_STEPS of the same lane.  One launch of at most `cus` workgroups of 256 threads striding over lanes x rows and
//      lanes x N, plain vector loads and stores only.
constexpr int EVAL_STEPS = 128;
struct LaneArgs {
    const uint8_t *text;
    const uint64_t *off;    // [streams + 1]
    const uint64_t *skip;   // [streams]
    const int32_t *slot;    // [windows][lanes]
    const int64_t *first;   // [streams]
    const float *H0, *C0;   // [streams][N]
    int32_t *xi, *ti;       // [EVAL_STEPS + 1][lanes]
    float *H, *C;           // [EVAL_STEPS + 1][lanes][N]
    const float *colloss;   // [EVAL_STEPS][lanes]
    double *bits;           // [streams]
    int lanes, N;
    int feed_last;          // 0: a stream of L bytes has L - 1 steps; 1: L steps
};
void lane_window(const LaneArgs &a, int64_t w, int cus, hipStream_t st);

// ---- the folds, behind the softmax launch.  Both: one thread per lane adds (double)colloss of the lane's rows that have a
//      target, in row order, into bits[s].
//      eval_fold also scatters those floats to sur (may be null) at the scored byte's place, off[s] + j + 1; the stream's last
//      column goes to column s of Hout / Cout (may be null) in the window where it ends.  One launch of at most `cus`
//      workgroups of 256 threads, plain vector loads and stores only.
struct EvalArgs : LaneArgs {
    float *sur;             // [off[streams]] or null
    float *Hout, *Cout;     // [streams][N] or null
};
void eval_fold(const EvalArgs &a, int64_t w, int cus, hipStream_t st);

//      embed_fold also pools and picks.  Per wanted source x (0: H, 1: C; a source is wanted when last[x] is not null, and
//      then sum, mean, maxv and last of it are all there): a
//      workgroup per (lane, 32 float4s of N) loads the lane's live rows at or above skip[s] at once, as 8 chunks of 16 rows,
//      and adds (double)v into four doubles per float4 chunk after chunk, in row order, keeping four float maxima; both are
//      carried in sum[x] / maxv[x] [streams][N] from the stream's window before (fresh in its first); in the window where the
//      stream ends it writes last[x] = the row of position L - 1,
//      mean[x] = (float)(sum / (double)count) and, for an empty pool, mean[x] = maxv[x] = +0.0f.  Rows past the stream's end are
//      never read.  picks [pick_lo, pick_hi) of the table (lane, row, k) are the window's: row `row` of lane `lane` goes to
//      column k of picked[x] ([npick][N], null: not wanted).  One launch of at most 8 * cus workgroups of 256 threads, plain
//      vector loads and stores only.
struct EmbedArgs : LaneArgs {
    double *sum[2];         // [streams][N] each
    float *mean[2], *maxv[2], *last[2];
    const int32_t *picks;   // [npick][3], sorted by window
    float *picked[2];       // [npick][N]
};
void embed_fold(const EmbedArgs &a, int64_t w, int64_t pick_lo, int64_t pick_hi, int cus, hipStream_t st);

// ---- B = 1 recurrence for the evaluator / sampler (OV/lstm_eigen_class_CUDA/lstm.cc:578-720)
// One workgroup with b1_lds_bytes(N) of dynamic LDS, which the caller checks against the device's opt-in limit first; both
// return the status of the grant and of the launch.
size_t b1_lds_bytes(int N);
hipError_t eval_bits(const float *P, int N, const uint8_t *text, uint64_t len, double *out_bits_sum, float *scratch, bool stable,
                     hipStream_t st);
hipError_t sample(const float *P, int N, float *hc /*2N*/, const double *u, int count, uint8_t *out, float *scratch, bool stable,
                  hipStream_t st);

// ---- the inference heads: one launch per step on the state after t inputs, then fwd_step over all columns with x_next as
// inputs.  Their argument blocks (GenHeadArgs, GuideLogitsArgs, BeamHeadArgs, CoderState and CodeHeadArgs, ScoreHeadArgs) are described in
// heads/head_args.h, included above; the kernels are heads/*.inc, included by kernels.hip.
// stable: LSTM_HIP_STABLE_SOFTMAX.  hipSuccess, or the HIP error of a refused LDS request with nothing launched (the FILTER
// instantiations only; beam_head and score_head likewise)
hipError_t gen_head(const GenHeadArgs &a, long long t, bool stable, hipStream_t st);
int gen_head_group(int N, int streams); // streams per workgroup of gen_head
// the guides of a guided call (GuideLogitsArgs, heads/guide_logits.inc): one launch per step ahead of the head, for all guides;
// the group size is gen_head_group(the widest guide, streams).  hipSuccess, or the HIP error of a refused LDS request
hipError_t guide_logits(const GuideLogitsArgs &a, long long t, hipStream_t st);
hipError_t beam_head(const BeamHeadArgs &a, long long t, hipStream_t st);
// out[(s * W + r) * count + i]: byte i of final slot r of stream s, walked back through the tables; 0 from len on
void beam_backtrack(const uint8_t *trace_parent, const uint8_t *trace_byte, const int32_t *len, uint8_t *out, int streams,
                    int W, int count, hipStream_t st);
void code_head(const CodeHeadArgs &a, long long t, hipStream_t st);
// the MIX instantiation (a.zk, a.v, a.nguides, a.rate set), behind guide_logits in coder mode: the table on
// the mixed logits, the coder step, the weights' update.  hipSuccess, or the HIP error of a refused LDS request
hipError_t code_head_mixed(const CodeHeadArgs &a, long long t, hipStream_t st);
hipError_t score_head(const ScoreHeadArgs &a, long long t, bool stable, hipStream_t st); // stable: LSTM_HIP_STABLE_SOFTMAX

// ---- adaptive coding (lstm_hip_encode_adaptive / lstm_hip_decode_adaptive): the training window of
// block k, built from the coder's device text buffer.  With L = S - 1 and e_j = byte j of a stream (empty for j < 0), row t of
// the window holds target e_{kL+t-1} and input e_{kL+t-2}: what slide_window leaves after k + 1 slides of stride L from an
// empty window with the stream's cursor at its first byte.  Flat xi / ti and the rings (head = 0) are both written; column
// S-1 of H and C moves to column 0 (16-byte accesses).  Workgroup 0 also folds the ideal bits coded since the last fold into
// *block_bits (per-stream differences against bits_prev, summed in one fixed tree order; bits null: nothing kept).
// build = 0: the fold only (the tail).  Every stream must hold at least (k + 1) * L bytes.  `cus`: the handle's CU count
// (the grid never exceeds it).
struct BlockWindowArgs {
    const uint8_t *text;        // the coder's text buffer
    const uint64_t *text_off;   // B + 1
    int32_t *xi, *ti, *Xr, *Tr, *head;
    float *H, *C;
    const double *bits;         // per stream, accumulated by code_head (null: decoder)
    double *bits_prev;          // per stream: the value at the last fold
    double *block_bits;         // where this fold goes
    long long k;
    int S, B, NB4, build;
};
void block_window(const BlockWindowArgs &a, int cus, hipStream_t st);

// ---- training on separate texts (lstm_hip_train_text_windows): window w of the plan
// lstm_hip_text_plan(S - 1, B, ...) on the training handle.  slot[w * B + l] is the stream lane l holds in window w (-1: idle);
// with L = S - 1 and j0 = L * (w - first[s]), row t of the lane holds step j0 + t - 1 of stream s: input byte j0 + t - 1,
// target byte j0 + t (row 0: the step before the window's first, as a slid window has it; it is never read).  A row without a
// step -- before the text's start, past its last step, an idle lane -- is xi = ti = -1.
// text_window: flat xi / ti and the rings (head = 0) are both written, as block_window writes them; column 0 of H and C of a
// lane that continues its text (w > first[s]) is column S - 1 of the same lane, of every other lane zero (16-byte accesses;
// S >= 2, so the column read is never the column written).  One launch of at most `cus` workgroups of 256 threads striding
// over S x B entries and B x N / 4 float4s.
// text_fold, behind the softmax launch: one thread per lane adds (double)colloss of the lane's rows that hold a step, in row
// order, into bits[s]: per stream the additions are sequential in text order, one window after the other.
struct TextWindowArgs {
    const uint8_t *text;
    const uint64_t *off;        // [streams + 1]
    const int32_t *slot;        // [windows][B]
    const int64_t *first;       // [streams]
    int32_t *xi, *ti, *Xr, *Tr, *head;
    float *H, *C;
    const float *colloss;       // [S - 1][B]
    double *bits;               // [streams]
    int S, B, N;
    // weighted texts (lstm_hip_set_train_texts_weighted), both null otherwise: weight is indexed like text, and text_window
    // writes wt [S][B] beside ti: the weight of the row's target byte (entry j + 1 for step j), 0 for a row without a step
    const float *weight;
    float *wt;
};
void text_window(const TextWindowArgs &a, int64_t w, int cus, hipStream_t st);
void text_fold(const TextWindowArgs &a, int64_t w, int cus, hipStream_t st);

} // namespace lstmk
