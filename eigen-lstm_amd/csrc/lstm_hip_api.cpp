// lstm_hip_api.cpp -- the C ABI of include/lstm_hip.h over the gfx950 kernels.
//
// One lstm_hip_ctx = what the reference keeps in cuParameters p, d, m and cuLSTM<S>
// (OV/lstm_eigen_class_CUDA/cu_lstm.h:20-304), laid out for one MI355X:
//   P, dP, mem : flat [W|U|b|Why|by] blocks (dP is also the RCCL all-reduce payload)
//   H, C       : [S][B][N]   (= N x (S*B) column-major; columns t*B.. are step t)
//   G, DG      : [S][B][4N]  post-activation gates / their gradients
//   Y          : [S][B][256] logits, overwritten in place by dY;  Pr: probs
//   DHy        : [S][B][N]   Why^T * dY for every step at once
// so the time-batched products see plain column-major matrices with T = (S-1)*B columns.
#include "../../include/lstm_hip.h"
#include "kernels.h"
#include "weight_drop.h"
#include "dfa_regex.h"

#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <tuple>
#include <type_traits>
#include <string>
#include <vector>

using namespace lstmk;

namespace {

thread_local char g_err[512] = "";
int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return fail(LSTM_HIP_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define TRY(expr)                         \
    do {                                  \
        if (int rc_ = (expr)) return rc_; \
    } while (0)

// ---- the owner of a handle's memory -------------------------------------------------------------------------------------
// Every device allocation of a handle goes through its DeviceMem, and so does its one pinned host array (h_losses, the
// second kind): what was allocated is what lstm_hip_destroy frees, on a half-built handle too, and no buffer has to be named
// twice.  The handle's members stay plain pointers; the owner keeps the list.
class DeviceMem {
    struct Held {
        void *p;
        bool pinned;
    };
    std::vector<Held> held;

  public:
    static constexpr int kNoFill = -1; // for a buffer that is written whole before it is read
    // p = `count` elements (bytes, for a void pointer), every byte set to fill_byte
    template <class T> int alloc(T *&p, size_t count, int fill_byte = 0) {
        const size_t bytes = count * sizeof(std::conditional_t<std::is_void_v<T>, char, T>);
        void *q = nullptr;
        HIP_TRY(hipMalloc(&q, bytes));
        held.push_back({q, false});
        p = static_cast<T *>(q);
        if (fill_byte != kNoFill) HIP_TRY(hipMemset(q, fill_byte, bytes));
        return 0;
    }
    template <class T> int alloc_pinned(T *&p, size_t count) {
        void *q = nullptr;
        HIP_TRY(hipHostMalloc(&q, count * sizeof(T), hipHostMallocDefault));
        held.push_back({q, true});
        p = static_cast<T *>(q);
        return 0;
    }
    // frees p, which alloc or alloc_pinned gave, and nulls it; a null p is nothing to do
    template <class T> int release(T *&p) {
        if (!p) return 0;
        const auto it = std::find_if(held.begin(), held.end(), [&](const Held &e) { return e.p == p; });
        const bool pinned = it != held.end() && it->pinned;
        if (it != held.end()) held.erase(it);
        void *q = p;
        p = nullptr;
        HIP_TRY(pinned ? hipHostFree(q) : hipFree(q));
        return 0;
    }
    // Room for `count` elements in a buffer that grows to its largest call and is kept: nothing to do while it fits (hipFree
    // waits for the whole device); otherwise `st` is drained, the buffer released and max(count, floor) elements allocated,
    // unfilled.  cap is 0 while there is no buffer.
    template <class T, class C> int grow(hipStream_t st, T *&p, C &cap, C count, C floor = 0) {
        if (count <= cap) return 0;
        HIP_TRY(hipStreamSynchronize(st));
        TRY(release(p));
        cap = 0;
        const C n = std::max(count, floor);
        TRY(alloc(p, (size_t)n, kNoFill));
        cap = n;
        return 0;
    }
    void free_all() {
        for (const Held &e : held) (void)(e.pinned ? hipHostFree(e.p) : hipFree(e.p));
        held.clear();
    }
};
// A device temporary of one call: allocated where the call can still refuse, freed on every return path.  (Not a piece of
// the handle's generator scratch: that is kept, and an evaluator's text can be large.)
template <class T> struct DeviceTemp {
    T *p = nullptr;
    DeviceTemp() = default;
    DeviceTemp(const DeviceTemp &) = delete;
    DeviceTemp &operator=(const DeviceTemp &) = delete;
    ~DeviceTemp() {
        if (p) (void)hipFree(p);
    }
    int alloc(size_t count) {
        HIP_TRY(hipMalloc((void **)&p, count * sizeof(T)));
        return 0;
    }
    operator T *() const { return p; }
};

// ---- the freshness of a handle's weight images --------------------------------------------------------------------------
// Which images of U and Why hold the current parameters.  Under weight drop the U flags say more: that the images AND the
// masked copy Ue are those of the current (rate, seed, t).  Three events make images stale or fresh, named here; the fourth,
// a training window that needs them, is the window_images_* functions below.  Nothing else writes a flag.
struct WeightImages {
    bool packed = false;     // the fp32 images of the plan's forms (Ufwd / Ubwd / Ufwd4 / Ubwd4)
    bool packed16 = false;   // the bf16 images as a set (what the one-recurrence forms read: Ufwd16 / Ubwd16)
    bool packed6b = false;   // Ubwd6b alone is current (written by the update launch)
    bool packedf6b = false;  // ... and Ufwd6b
    bool why_packed = false; // both bf16 copies of Why

    bool u_current(const EnginePlan &p) const { return p.bf16() ? packed16 : packed; }
    // the parameter block was written from outside (lstm_hip_set_params, the internal handles' copy of the parent's block)
    void params_written() { *this = WeightImages{}; }
    // weight drop got another (rate, seed, t) or went off: every image of U is of another source; Why is not masked
    void mask_changed() { packed = packed16 = packed6b = packedf6b = false; }
    // An update launch ran.  It refreshed the fp32 images of U (the bf16 path has none) and, on the bf16 path, the two-half
    // images (Ufwd6b in its quad form only) and both bf16 copies of Why; pack_U_bf16 repacks the one-recurrence images.
    // Under weight drop the launch's images are of the unmasked U and the next window has the next mask.
    void update_ran(const EnginePlan &p, bool weight_drop) {
        packed = true;
        packed16 = false;
        packed6b = p.bwd == BwdForm::Bf16Scatter;
        packedf6b = p.fwd == FwdForm::Bf16Halves && p.adagrad_quad;
        why_packed = p.bf16();
        if (weight_drop) mask_changed();
    }
};

enum KernelId {
    K_PACK_U, K_FWD_STEP, K_GEMM_Y, K_SOFTMAX, K_LOSS, K_GEMM_DHY, K_BWD_STEP, K_GEMM_DWHY, K_GEMM_DU, K_DW_DB,
    K_DBY, K_ADAGRAD, K_SLIDE, K_ALLREDUCE, K_FWD_PERSIST, K_BWD_PERSIST, K_GEN_HEAD,
    K_SIDE_SUMS, // dW_sort, the dWhy product and dW_sums on the second stream (never timed: profiling keeps them on `st`)
    K_DU_HALVES, // the two column halves of the dU product (LSTM_HIP_DU_SPLIT; communicator loop only, never timed)
    K_GRAD_SUMSQ, K_GRAD_NORM, // global-norm clipping (lstm_hip_set_grad_clip): partial sums of d^2, then norm and coefficient
    K_ADAM,                    // the update launch on a handle set to LSTM_HIP_OPT_ADAM (K_ADAGRAD's launch with the Adam rule)
    K_CODE_HEAD,               // one step of the range coder (lstm_hip_encode / lstm_hip_decode)
    K_BLOCK_WINDOW,            // adaptive coding: a block's training window, carry and bit fold (one launch per block)
    K_TEXT_WINDOW,             // training on separate texts (lstm_hip_train_text_windows): a plan window's indices and carry ...
    K_TEXT_FOLD,               // ... the fold of its surprisals into the streams' bits ...
    K_SOFTMAX_TEXT,            // ... and K_SOFTMAX's launch in the form that gives a column without a target dy = 0
    K_BEAM_HEAD,              // one step of beam search (lstm_hip_beam_search): logits, selection, reordered states
    K_BEAM_BACKTRACK,          // ... and the walk through its tables, once per call
    K_SCORE_HEAD,              // one step of lstm_hip_score: logits, surprisal, entropy, rank and alternatives of every stream
    K_COUNT_BASE, // the ids above have their names in kKernelNames, the ids from here on in kKernelNamesMore (kernel_name)
    K_SOFTMAX_SOFT = K_COUNT_BASE, // K_SOFTMAX's launch with soft targets (lstm_hip_set_soft_targets): label smoothing, a teacher's term
    K_SOFTMAX_WEIGHTED,            // K_SOFTMAX_TEXT's launch with a weight per target byte (lstm_hip_set_train_texts_weighted)
    K_GRAD_ACCUMULATE,             // gradient accumulation (lstm_hip_set_grad_accumulation): a window's gradient into the accumulator
    K_COUNT_MORE, // ... and the ids from here on in kKernelNamesLast
    K_GUIDE_LOGITS = K_COUNT_MORE, // one step of the guides of a guided call (lstm_hip_generate_guided / lstm_hip_score_guided)
    K_COUNT_LAST, // ... and the ids from here on in kKernelNamesMixed
    K_CODE_HEAD_MIXED = K_COUNT_LAST, // one step of the mixed range coder (lstm_hip_encode_mixed / lstm_hip_decode_mixed)
    K_COUNT
};
const char *const kKernelNames[K_COUNT] = { // (K_COUNT_BASE names; the rows behind them stay null)
    "pack_U", "fwd_step", "gemm_Y", "softmax_loss_dy", "loss_reduce", "gemm_DHy", "bwd_step", "gemm_dWhy", "gemm_dU",
    "dW_db", "loss_dby", "adagrad", "slide", "allreduce", "fwd_persistent", "bwd_persistent", "gen_head", "side_sums",
    "gemm_dU_halves", "grad_sumsq", "grad_norm", "adam", "code_head", "block_window", "text_window", "text_fold",
    "softmax_loss_dy_text", "beam_head", "beam_backtrack", "score_head"};
const char *const kKernelNamesMore[K_COUNT_MORE - K_COUNT_BASE] = {"softmax_soft", "softmax_loss_dy_weighted", "grad_accumulate"};
const char *const kKernelNamesLast[K_COUNT - K_COUNT_MORE] = {"guide_logits"}; // (K_COUNT_LAST - K_COUNT_MORE names)
const char *const kKernelNamesMixed[K_COUNT - K_COUNT_LAST] = {"code_head_mixed"};
inline const char *kernel_name(int id) {
    return id < K_COUNT_BASE   ? kKernelNames[id]
           : id < K_COUNT_MORE ? kKernelNamesMore[id - K_COUNT_BASE]
           : id < K_COUNT_LAST ? kKernelNamesLast[id - K_COUNT_MORE]
                               : kKernelNamesMixed[id - K_COUNT_LAST];
}

// ---- RCCL, loaded on first use so single-GPU users never touch it --------------------------
struct UniqueId {
    char internal[LSTM_HIP_UNIQUE_ID_BYTES];
};
struct Rccl {
    void *lib = nullptr;
    int (*GetUniqueId)(void *) = nullptr;
    int (*CommInitRank)(void **, int, UniqueId, int) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*GroupStart)() = nullptr; // optional
    int (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
};
Rccl g_rccl;
int rccl_load() {
    if (g_rccl.lib) return 0;
    void *lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) return fail(LSTM_HIP_ERCCL, "cannot load librccl: %s", dlerror());
    g_rccl.GetUniqueId = (decltype(g_rccl.GetUniqueId))dlsym(lib, "ncclGetUniqueId");
    g_rccl.CommInitRank = (decltype(g_rccl.CommInitRank))dlsym(lib, "ncclCommInitRank");
    g_rccl.AllReduce = (decltype(g_rccl.AllReduce))dlsym(lib, "ncclAllReduce");
    g_rccl.CommDestroy = (decltype(g_rccl.CommDestroy))dlsym(lib, "ncclCommDestroy");
    g_rccl.GetErrorString = (decltype(g_rccl.GetErrorString))dlsym(lib, "ncclGetErrorString");
    g_rccl.GroupStart = (decltype(g_rccl.GroupStart))dlsym(lib, "ncclGroupStart");
    g_rccl.GroupEnd = (decltype(g_rccl.GroupEnd))dlsym(lib, "ncclGroupEnd");
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllReduce || !g_rccl.CommDestroy)
        return fail(LSTM_HIP_ERCCL, "librccl lacks a required symbol");
    g_rccl.lib = lib;
    return 0;
}

} // namespace

struct lstm_hip_ctx {
    lstm_hip_config cfg{}; // cfg.N is the internal (padded) width Np; every buffer and launcher uses it
    int N_log = 0;         // the caller's N (LSTM_HIP_PAD_HIDDEN: may be < cfg.N); the boundary calls convert to and from it
    float *stage = nullptr; // N_log != cfg.N: logical-width staging buffer of the boundary copies (pad_copy)
    bool padded() const { return N_log != cfg.N; }
    ParamLayout pl{};
    int T = 0; // (S-1)*B columns in the time-batched matrices
    hipStream_t st = nullptr;
    hipStream_t st2 = nullptr; // the early part of the gradient all-reduce runs here, beside the dU product on `st`
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_fork = nullptr, ev_join = nullptr, ev_mid = nullptr, evt0 = nullptr, evt1 = nullptr;
    bool fold_pending = false;  // the backward pass left the gradient in pieces for Adagrad to sum (single-GPU loop)
    int n_slabs_dU = 0;         // ... with this many dU slabs (0: dU is final in dP)
    bool in_loop = false;       // inside lstm_hip_train_windows: nobody reads the gradient block between backward and Adagrad
    size_t dU_reduced = 0;      // ... and so are this many leading floats of the dU range (its first column half)
    bool early_reduced = false; // [dW] and [db | dWhy | dby] are already being all-reduced on st2 (ev_join marks the end)
    float *slabs_dU = nullptr; // split-K slabs of dU
    EnginePlan plan;           // the form of each recurrence and everything derived from it (plan_engine)
    DeviceMem own;             // every device buffer below (and the pinned h_losses) is allocated and freed through it
    WeightImages img;          // which of the weight images below are current
    unsigned short *Hb = nullptr, *DGb = nullptr; // bf16 hand-off copies of h and dg
    void *Ufwd16 = nullptr, *Ubwd16 = nullptr;    // bf16 fragment images of U (the one-recurrence forms)
    void *Ubwd6b = nullptr;                       // ... of the scatter-form backward (BwdForm::Bf16Scatter)
    void *Ufwd6b = nullptr;                       // two-half bf16 forward form: weights image
    unsigned short *Hxb = nullptr;                // ... and bf16 hand-off ring
    bool carry_slide = false, pre_slid = false;   // window loop: this Adagrad launch carries the next window's slide / it has been done
    // window loops, single GPU, fused gradients, no clipping, not profiling (loop_window): the window's loss sum and dby fold ride
    // in its update launch instead of a launch of their own, and only the loop's last window stores what nothing inside the
    // loop reads -- the probabilities and the folded gradient
    bool tail = false;                            // this window's loss / dby go with its update launch ...
    double *tail_loss = nullptr;                  // ... the loss to here
    bool keep_outputs = true;                     // this window stores Pr and the folded dP
    bool pr_stale = false, dp_stale = false;      // Pr / dP do not hold the last window's values: get_activations / get_grads refuse
    bool dgt_written = false;                     // the backward recurrence wrote the transposed bf16 image of dg itself
    // bf16 operands of the four time-batched products, k contiguous (kernels.h, gemm_bf16): Why^T and Why; per window
    // h^T [N][SBpad], dy^T [256][Tpad], dg^T [4N][Tpad] and dy [T][256]
    unsigned short *WhyT_b = nullptr, *Why_b = nullptr, *Ht_b = nullptr, *dYt_b = nullptr, *DGt_b = nullptr, *dYb = nullptr;
    int Tpad = 0, SBpad = 0;
    float *gpart = nullptr;    // per-column-group partial [dW|dU|db|dWhy] blocks of the fused backward recurrence

    float *P = nullptr, *dP = nullptr, *mem = nullptr;
    float4 *Ufwd = nullptr, *Ubwd = nullptr; // 16x16x4 tile images of U (fp32)
    float4 *Ubwd4 = nullptr; // weight image of the 4x4x1 backward forms (kernels.hip, k_pack_U): BwdForm::Cols8 / Scatter
    float4 *Ufwd4 = nullptr; // ... of the 8-column forward forms: FwdForm::Cols8 / TwoHalf
    float *Hx = nullptr;     // 8-column forward forms: ring of hand-off slots (data-as-flag), sentinel-filled
    int ring_base = 0;       // slot of step 0 in the next launch
    float *DGx = nullptr;    // backward scatter forms: the same kind of ring for the partial sums
    int ring_base_b = 0;
    float *H = nullptr, *C = nullptr, *G = nullptr, *DG = nullptr, *Y = nullptr, *Pr = nullptr, *DHy = nullptr;
    float *dcnext = nullptr, *colloss = nullptr, *dby_part = nullptr, *slabs = nullptr;
    char *dw_scratch = nullptr;
    int n_dby_parts = 0;
    int splits_dWhy = 1, splits_dU = 1;
    int32_t *xi = nullptr, *ti = nullptr;            // flat [S][B] indices the kernels read
    int32_t *Xr = nullptr, *Tr = nullptr, *head = nullptr; // ring form kept by the device-side slide
    double *d_loss = nullptr;
    double *d_losses = nullptr;
    double *h_losses = nullptr; // pinned twin of d_losses: the caller's (pageable) array is filled from it after the sync.
                                // (The runtime's own staging path for a first large pageable copy cost the NEXT 20 windows
                                // 0.4 ms of device time -- tools/train_windows_probe.py.)
    int64_t losses_cap = 0;
    // global-norm clipping (lstm_hip_set_grad_clip): max_norm 0 = off
    double clip_max = 0.0;
    double *d_norms = nullptr;  // pre-clip norm of every Adagrad step of the current call (the window index of train_windows)
    double *norm_part = nullptr; // grad_norm_parts(total) workgroup partials of k_grad_sumsq
    float *clip_coef = nullptr;  // the coefficient of the step under way
    int64_t norms_cap = 0;       // d_norms holds this many
    int64_t norms_n = -1;        // steps of the last adagrad / train_windows call that recorded norms; -1: clipping was off
    int64_t call_updates = 0;    // updates launched by the call under way (do_adagrad): the slot of d_norms the next one writes
    // gradient accumulation (lstm_hip_set_grad_accumulation): acc_every 1 = off
    int32_t acc_every = 1, acc_mean = 0, acc_pending = 0; // windows per update / divide by it / windows summed in `acc` so far
    float *acc = nullptr;        // their summed gradient (flat block, internal width); allocated when accumulation is first turned on
    // the update rule (lstm_hip_set_optimizer): Adagrad, or Adam with m in `mem` and v in adam_v
    int opt_kind = LSTM_HIP_OPT_ADAGRAD;
    double beta1 = 0.0, beta2 = 0.0, adam_eps = 0.0, weight_decay = 0.0;
    int64_t opt_steps = 0;       // updates launched since create / the last change of kind
    float *adam_v = nullptr;     // Adam's second moment (flat block); allocated when Adam is first selected
    // the running weight average (lstm_hip_set_averaging): its own launch after the update launch, on due updates only
    int avg_kind = LSTM_HIP_AVG_OFF;
    double avg_decay = 0.0;
    int32_t avg_every = 1;
    int64_t avg_seen = 0, avg_n = 0; // updates launched with averaging on / of those, the due ones (the average's own count)
    float *avg = nullptr;            // the average (flat block, internal width); allocated when averaging is first turned on
    int infer_src = LSTM_HIP_SRC_PARAMS; // the block the inference calls read (infer_block)
    // weight drop (lstm_hip_set_weight_drop): rate 0 = off.  While it is on, a training window's recurrences read images
    // packed from Ue, and the U flags of `img` say that the images AND Ue are those of the current (rate, seed, t)
    double wd_rate = 0.0;
    uint64_t wd_seed = 0, wd_t = 0;
    uint32_t wd_thr = 0;         // floor(rate * 2^32)
    float wd_scale = 1.0f;       // 1 / (1 - rate)
    float *Ue = nullptr;         // the masked, rescaled U (4Np^2 floats); allocated when weight drop is first turned on
    uint8_t *text = nullptr;
    uint64_t text_len = 0;
    uint64_t *pos = nullptr;     // the live cursors and ring head: one half of pos_buf [2][B] / head_buf [2].  A slide carried
    uint64_t *pos_buf = nullptr; // by an update launch reads the live half and writes the other, then the halves change roles
    int32_t *head_buf = nullptr; // (do_adagrad)
    int32_t global_B = 0;
    // training on separate texts (lstm_hip_set_train_texts): the texts, their offsets, the tables of the plan
    // lstm_hip_text_plan(S - 1, B, ...) and the streams' prequential bits, all on the device; tt_streams 0: none set
    uint8_t *tt_text = nullptr;
    uint64_t *tt_off = nullptr;   // [streams + 1]
    int32_t *tt_slot = nullptr;   // [windows][B]
    int64_t *tt_first = nullptr;  // [streams]
    double *tt_bits = nullptr;    // [streams]
    float *tt_weight = nullptr;   // (lstm_hip_set_train_texts_weighted; null: unweighted) a weight per byte, indexed like tt_text
    float *tt_wt = nullptr;       // ... and the window's weights beside ti, [S][B]: scratch that text_window rewrites every window
    int32_t tt_streams = 0;
    int64_t tt_windows = 0, tt_next = 0; // the plan's length, the next window to run
    bool text_window = false;     // the window under way is one of those: do_forward launches the softmax's text form
    // soft targets (lstm_hip_set_soft_targets): off unless soft_on.  A student borrows its teacher:
    // before its own forward pass it runs the teacher's recurrence and Why * H product on its own stream (one stream: the
    // two handles' persistent recurrences are never in flight together) and its softmax launch reads the teacher's Y and by
    bool soft_on = false;
    lstm_hip_ctx *teacher = nullptr;
    lstm_hip_soft_targets soft_opt{};
    float *colkl = nullptr;       // [T] per-column KL(q || p_tau) in bits (teacher only)
    double *d_kls = nullptr;      // the per-window KL figures of the last forward / train_windows call
    int64_t kls_cap = 0, kls_n = -1, kl_idx = 0; // d_kls holds this many / figures of the last call (-1: none) / the window under way
    hipEvent_t ev_soft[2] = {nullptr, nullptr}; // the teacher's own stream -> the student's, and back
    // ... and on the teacher's side
    int lent = 0;                 // students that hold this handle as their teacher (lstm_hip_destroy refuses while > 0)
    bool teacher_pass = false;    // do_forward stops before the softmax launch: Y keeps the logits
    bool last_fwd_teacher = false; // the last forward pass was such a pass (lstm_hip_backward says so)
    bool window_lent = false;     // a student's forward pass of the call under way has overwritten xi (TeacherStream hands the rest over)
    lstm_hip_ctx *eval_h = nullptr; // internal B = 1 handle used by lstm_hip_eval_bits
    lstm_hip_ctx *texts_h = nullptr; // internal B = lanes handle used by lstm_hip_eval_texts (remade when lanes changes)
    char *gen_scratch = nullptr;    // lstm_hip_generate's working memory: grows to the largest call, freed with the handle
    size_t gen_scratch_bytes = 0;
    int stride = 1, carry_col = 1; // window advance per iteration and the column that becomes the carry
    bool fwd_done = false;
    bool dby_done = false;       // dby already produced by the loss launch of this window
    unsigned *cnt = nullptr;     // [2][persistent_counter_bytes]: fwd region, bwd region
    unsigned *abortp = nullptr;  // set by a timed-out spin inside a persistent kernel
    size_t cnt_bytes = 0;
    unsigned long long *stamps = nullptr; // LSTM_HIP_DEBUG_STAMPS: [fwd, bwd][2 workgroups][S][16] s_memtime values
    int loss_mode = 0; // LSTM_HIP_LOSS_*
    unsigned fwd_epoch = 0, bwd_epoch = 0; // launches so far on the cumulative hand-off counters
    int64_t counter_resets = 0;            // times either direction cleared its counters at EnginePlan::epoch_limit

    void *comm = nullptr;
    int nranks = 1, rank = 0;

    bool profiling = false;
    int64_t launches[K_COUNT] = {};
    double total_ms[K_COUNT] = {};
};

namespace {

// Every launch is checked: a kernel that could not be launched (resources, an attribute that was refused) must not leave the
// window to complete "successfully" on stale buffers.
int launch_status(int id) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(LSTM_HIP_EHIP, "launch of %s failed: %s", kernel_name(id), hipGetErrorString(e));
    return 0;
}
// ... and the launches that are not among the window's timed kernels and have no statistics row, under their own names:
// pad_copy (the boundary's layout copies), weight_drop, average, and lane_window / eval_fold / embed_fold of the text lanes
int untimed_status(const char *name) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(LSTM_HIP_EHIP, "launch of %s failed: %s", name, hipGetErrorString(e));
    return 0;
}
template <class F> int timed(lstm_hip_ctx *h, int id, F &&launch) {
    if (!h->profiling) {
        launch();
        return launch_status(id);
    }
    HIP_TRY(hipEventRecord(h->ev0, h->st));
    launch();
    if (int rc = launch_status(id)) return rc;
    HIP_TRY(hipEventRecord(h->ev1, h->st));
    HIP_TRY(hipEventSynchronize(h->ev1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    h->launches[id]++;
    h->total_ms[id] += ms;
    return 0;
}
#define RUN(id, ...)                                               \
    do {                                                           \
        int rc_ = timed(h, id, [&]() { __VA_ARGS__; });            \
        if (rc_) return rc_;                                       \
    } while (0)

int check(lstm_hip_ctx *h) {
    if (!h) return fail(LSTM_HIP_EINVAL, "null handle");
    HIP_TRY(hipSetDevice(h->cfg.device));
    lds_device = h->cfg.device; // (grant_lds, kernels.h)
    return 0;
}
#define CHECK(h)             \
    do {                     \
        int rc_ = check(h);  \
        if (rc_) return rc_; \
    } while (0)

// after a synchronisation point: did a persistent kernel give up on a hand-off?
int check_abort(lstm_hip_ctx *h) {
    const EnginePlan &p = h->plan;
    if (!p.persistent()) return 0;
    unsigned flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, h->abortp, sizeof(unsigned), hipMemcpyDeviceToHost, h->st));
    HIP_TRY(hipStreamSynchronize(h->st));
    if (flag != 0) {
        HIP_TRY(hipMemsetAsync(h->abortp, 0, sizeof(unsigned), h->st));
        HIP_TRY(hipMemsetAsync(h->cnt, 0, 2 * h->cnt_bytes, h->st)); // counters are inconsistent after an abort
        h->fwd_epoch = h->bwd_epoch = 0;
        // and so are the hand-off rings
        if (p.fwd == FwdForm::Cols8 || p.fwd == FwdForm::TwoHalf)
            HIP_TRY(hipMemsetAsync(h->Hx, 0xff, sizeof(float) * p.hx_floats, h->st));
        if (p.fwd == FwdForm::Bf16Halves)
            HIP_TRY(hipMemsetAsync(h->Hxb, 0xff, sizeof(unsigned short) * p.hxb_halfwords, h->st));
        h->ring_base = 0;
        if (p.bwd == BwdForm::Scatter || p.bwd == BwdForm::Bf16Scatter)
            HIP_TRY(hipMemsetAsync(h->DGx, 0xff, sizeof(float) * p.dgx_floats, h->st));
        h->ring_base_b = 0;
        return fail(LSTM_HIP_ESTATE, "a persistent recurrence kernel timed out waiting for a hand-off (results invalid)");
    }
    return 0;
}

// reported loss: all S-1 steps in bits (R/lstm.cc:204-207), or the last step only -- in nats
// (OV/lstm_eigen_class_CUDA/lstm.h:200-221) or in bits (cuLSTM::calculate_loss, cu_lstm.h:203-215);
// colloss holds -log2 p(target) per (step, column)
bool loss_last_step(const lstm_hip_ctx *h) { return h->loss_mode != LSTM_HIP_LOSS_ALL_STEPS_BITS; }
const float *loss_src(const lstm_hip_ctx *h) {
    return loss_last_step(h) ? h->colloss + (size_t)(h->cfg.S - 2) * h->cfg.B : h->colloss;
}
int loss_steps(const lstm_hip_ctx *h) { return loss_last_step(h) ? 1 : h->cfg.S - 1; }
float loss_scale(const lstm_hip_ctx *h) { return h->loss_mode == LSTM_HIP_LOSS_LAST_STEP_NATS ? 0.693147180559945f : 1.0f; }

// Weight drop (lstm_hip_set_weight_drop): one elementwise launch over U with the mask of the handle's (rate, seed, t), on the
// handle's stream.  Like average it is not one of the window's timed kernels: untimed_status, no statistics row.
int weight_drop_launch(lstm_hip_ctx *h, const float *src, float *dst) {
    weight_drop_mask(src, dst, h->cfg.N, h->N_log, h->wd_seed, h->wd_t, h->wd_thr, h->wd_scale, h->plan.n_cus, h->st);
    return untimed_status("weight_drop");
}

int do_forward(lstm_hip_ctx *h);
// A student's window, before its own forward pass: the teacher gets the window's inputs and, inside a window loop, slides as
// the student slid (its own column carry_col becomes its column 0); then its recurrence and its Why * H product run in the
// forms of its own plan.  The caller has put the teacher on the student's stream (TeacherStream).
int teacher_forward(lstm_hip_ctx *h) {
    lstm_hip_ctx *t = h->teacher;
    const size_t cols = (size_t)h->cfg.S * h->cfg.B, n = (size_t)t->cfg.N * t->cfg.B;
    HIP_TRY(hipMemcpyAsync(t->xi, h->xi, sizeof(int32_t) * cols, hipMemcpyDeviceToDevice, h->st));
    if (h->in_loop && h->carry_col > 0) {
        HIP_TRY(hipMemcpyAsync(t->H, t->H + h->carry_col * n, sizeof(float) * n, hipMemcpyDeviceToDevice, h->st));
        HIP_TRY(hipMemcpyAsync(t->C, t->C + h->carry_col * n, sizeof(float) * n, hipMemcpyDeviceToDevice, h->st));
    }
    t->window_lent = true; // (the end of the call brings its targets and its ring form along: TeacherStream)
    t->teacher_pass = true;
    const int rc = do_forward(t);
    t->teacher_pass = false;
    return rc;
}
// Puts a borrowed teacher on its student's stream for one call: an event pair each way orders what the caller left on the
// teacher's own stream before the call, and what the call leaves, before the teacher's next boundary call.  No host wait.
struct TeacherStream {
    lstm_hip_ctx *h, *t;
    hipStream_t own = nullptr;
    explicit TeacherStream(lstm_hip_ctx *h_) : h(h_), t(h_->soft_on ? h_->teacher : nullptr) {}
    int begin() {
        if (!t) return 0;
        HIP_TRY(hipEventRecord(h->ev_soft[0], t->st));
        HIP_TRY(hipStreamWaitEvent(h->st, h->ev_soft[0], 0));
        own = t->st;
        t->st = h->st;
        return 0;
    }
    // A teacher whose inputs a forward pass of this call overwrote gets the rest of the student's window too: the targets and
    // the ring form the device-side slide reads, head 0, as lstm_hip_set_window would leave them.  Its window is then one
    // window again -- the one lstm_hip_get_window returns is the one its own next lstm_hip_train_windows slides from -- and
    // not the student's inputs over its own targets and ring.  Once per call, on the student's stream.
    void hand_back_window() {
        if (!t->window_lent) return;
        t->window_lent = false;
        const size_t bytes = sizeof(int32_t) * h->cfg.S * h->cfg.B;
        (void)hipMemcpyAsync(t->ti, h->ti, bytes, hipMemcpyDeviceToDevice, h->st);
        (void)hipMemcpyAsync(t->Xr, t->xi, bytes, hipMemcpyDeviceToDevice, h->st);
        (void)hipMemcpyAsync(t->Tr, h->ti, bytes, hipMemcpyDeviceToDevice, h->st);
        (void)hipMemsetAsync(t->head, 0, sizeof(int32_t), h->st);
        t->pre_slid = false;
    }
    ~TeacherStream() {
        if (!own) return;
        hand_back_window();
        t->st = own;
        if (hipEventRecord(h->ev_soft[1], h->st) == hipSuccess) (void)hipStreamWaitEvent(own, h->ev_soft[1], 0);
        else (void)hipStreamSynchronize(h->st);
    }
};
// before anything of a student's window is launched
int soft_precheck(lstm_hip_ctx *h, const char *what) {
    if (!h->soft_on || !h->teacher) return 0;
    if (h->teacher->wd_rate > 0.0)
        return fail(LSTM_HIP_ESTATE, "%s: the teacher has weight drop on (lstm_hip_set_weight_drop); a teacher runs its unmasked "
                                     "parameters", what);
    return 0;
}

// A training window needs the images (the fourth event of WeightImages): whatever is stale is made from Usrc -- the
// parameters' U, or under weight drop the masked copy Ue, itself remade first -- and marked current.  Three functions, one
// per place the launches have in the window: the mask and the fp32 images before the hand-off epoch of do_forward, the bf16
// images of U behind it, the bf16 copies of Why behind the recurrence.
int window_images_fp32(lstm_hip_ctx *h, const float *Usrc) {
    const EnginePlan &p = h->plan;
    if (h->wd_rate > 0.0 && !h->img.u_current(p))
        if (int rc = weight_drop_launch(h, h->P + h->pl.U, h->Ue)) return rc;
    if (!h->img.packed && !p.bf16()) { // (the bf16 path packs its own images: window_images_bf16)
        RUN(K_PACK_U, pack_U(Usrc, p.ufwd4() ? nullptr : h->Ufwd, p.ubwd4() ? nullptr : h->Ubwd, h->cfg.N, h->st, h->Ubwd4,
                             h->Ufwd4, p.half_forms())); // one image per direction is live
        h->img.packed = true;
    }
    return 0;
}
int window_images_bf16(lstm_hip_ctx *h, const float *Usrc) {
    const EnginePlan &p = h->plan;
    const int N = h->cfg.N;
    if (p.bf16() && !h->img.packed16) { // (the one-recurrence forms' images only where one of them runs)
        RUN(K_PACK_U, (p.u16 ? pack_U_bf16(Usrc, h->Ufwd16, h->Ubwd16, N, h->st) : (void)0,
                       p.bwd == BwdForm::Bf16Scatter && !h->img.packed6b ? pack_U6_bf16(Usrc, h->Ubwd6b, N, h->st) : (void)0,
                       p.fwd == FwdForm::Bf16Halves && !h->img.packedf6b ? pack_Ufwd6_bf16(Usrc, h->Ufwd6b, N, h->st) : (void)0));
        h->img.packed16 = true;
    }
    return 0;
}
int window_images_why(lstm_hip_ctx *h) { // Why rounded once per update
    const int N = h->cfg.N;
    if (h->plan.bf16() && !h->img.why_packed) {
        RUN(K_PACK_U, (transpose_pack_bf16(h->P + h->pl.Why, N, 256, 256, h->WhyT_b, N, h->st),
                       pack_bf16(h->P + h->pl.Why, (size_t)256 * N, h->Why_b, h->st)));
        h->img.why_packed = true;
    }
    return 0;
}

int do_forward(lstm_hip_ctx *h) {
    const EnginePlan &p = h->plan;
    const int N = h->cfg.N, B = h->cfg.B, S = h->cfg.S, G4 = 4 * N;
    const bool fast = (h->cfg.flags & LSTM_HIP_FAST_MATH) != 0;
    float *W = h->P + h->pl.W, *bias = h->P + h->pl.b;
    if (h->soft_on && h->teacher) // the teacher's logits of this window first, on this stream
        if (int rc = teacher_forward(h)) return rc;
    // weight drop: the window's images of U are packed from the masked copy, remade whenever they are
    const float *Usrc = h->wd_rate > 0.0 ? h->Ue : h->P + h->pl.U;
    TRY(window_images_fp32(h, Usrc));
    h->n_dby_parts = softmax_parts(h->T);
    if (p.persistent()) {
        if (h->fwd_epoch >= p.epoch_limit) { // keep epoch * arrivals inside 32 bits
            HIP_TRY(hipMemsetAsync(h->cnt, 0, h->cnt_bytes, h->st));
            h->fwd_epoch = 0;
            h->counter_resets++;
        }
        h->fwd_epoch++;
    }
    TRY(window_images_bf16(h, Usrc));
    switch (p.fwd) {
    case FwdForm::Step:
        for (int t = 1; t < S; t++) {
            RUN(K_FWD_STEP, fwd_step(h->Ufwd, W, bias, h->H + (size_t)(t - 1) * N * B, h->C + (size_t)(t - 1) * N * B,
                                     h->H + (size_t)t * N * B, h->C + (size_t)t * N * B, h->G + (size_t)t * G4 * B,
                                     h->xi + (size_t)t * B, N, B, fast, h->st));
        }
        break;
    case FwdForm::Small:
        RUN(K_FWD_PERSIST, small_fwd(Usrc, W, bias, h->H, h->C, h->G, h->xi, N, S, fast, h->st));
        break;
    case FwdForm::Persistent:
        RUN(K_FWD_PERSIST, fwd_persistent(h->Ufwd, W, bias, h->H, h->C, h->G, h->xi, h->cnt, h->abortp, h->fwd_epoch, N, S, B, fast,
                                          h->st));
        break;
    case FwdForm::Cols8:
        RUN(K_FWD_PERSIST, fwd_persistent4(h->Ufwd4, W, bias, h->H, h->C, h->G, h->xi, h->Hx, h->cnt, h->abortp, h->fwd_epoch,
                                           h->ring_base, N, S, B, fast, p.poll_cfg, h->st, h->stamps));
        h->ring_base = fwd_ring_advance(h->ring_base, S);
        break;
    case FwdForm::TwoHalf: // as many groups per launch as are co-resident (one launch unless the batch is wide)
        for (int c0 = 0; c0 < B; c0 += p.launch_cols) {
            if (c0 > 0) h->fwd_epoch++;
            RUN(K_FWD_PERSIST, fwd_persistent6(h->Ufwd4, W, bias, h->H, h->C, h->G, h->xi, h->Hx, h->cnt, h->abortp, h->fwd_epoch,
                                               h->ring_base, N, S, B, fast, p.poll_cfg, c0, std::min(B - c0, p.launch_cols),
                                               p.group_cols, p.fwd_pin, h->st, h->stamps));
        }
        h->ring_base = fwd_ring_advance(h->ring_base, S); // (every column has made the same S - 1 hand-offs on its part of the ring)
        break;
    case FwdForm::Bf16:
        RUN(K_FWD_PERSIST, fwd_persistent_bf16(h->Ufwd16, W, bias, h->H, h->Hb, h->C, h->G, h->xi, h->cnt, h->abortp, h->fwd_epoch,
                                               N, S, B, fast, p.fwd_cols, h->st));
        break;
    case FwdForm::Bf16Halves: // likewise; the streams are independent
        for (int c0 = 0; c0 < B; c0 += p.launch_cols) {
            if (c0 > 0) h->fwd_epoch++;
            RUN(K_FWD_PERSIST, fwd_halves_bf16(h->Ufwd6b, W, bias, h->H, h->Hb, h->C, h->G, h->xi, h->Hxb, h->cnt, h->abortp,
                                               h->fwd_epoch, h->ring_base, N, S, B, c0, std::min(B - c0, p.launch_cols),
                                               p.group_cols, p.fwd_pin, fast, h->st, h->stamps));
        }
        h->ring_base = fwd_ring_advance(h->ring_base, S);
        break;
    }
    // Y = Why * H[1..S-1]   (R/lstm.cc:195 for every step at once)
    TRY(window_images_why(h));
    if (p.bf16()) { // bf16 operands (Why rounded once per update, the recurrence's own bf16 copy of h), fp32 accumulate
        RUN(K_GEMM_Y, gemm_bf16(256, h->T, N, h->WhyT_b, N, h->Hb + (size_t)N * B, N, h->Y + (size_t)256 * B, 256, 1, nullptr,
                                h->st));
    } else
    RUN(K_GEMM_Y, gemm(false, false, 256, h->T, N, h->P + h->pl.Why, 256, h->H + (size_t)N * B, N,
                       h->Y + (size_t)256 * B, 256, 1, nullptr, h->st));
    h->last_fwd_teacher = h->teacher_pass;
    if (h->teacher_pass) { // (a borrowed teacher: its student's softmax launch reads the logits; no training forward)
        h->pr_stale = true;
        h->fwd_done = false;
        return 0;
    }
    h->pr_stale = h->in_loop && !h->keep_outputs;
    if (h->soft_on) {
        const lstm_hip_soft_targets &o = h->soft_opt; // the scalars in double, narrowed (include/lstm_hip.h)
        SoftTargetArgs a{};
        a.alpha = (float)o.alpha, a.oma_tau = (float)((1.0 - o.alpha) * o.temperature), a.inv_tau = (float)(1.0 / o.temperature);
        a.ome = (float)(1.0 - o.smoothing), a.eps256 = (float)(o.smoothing / 256.0);
        a.tempered = o.temperature != 1.0;
        if (const lstm_hip_ctx *t = h->teacher) a.Yt = t->Y + (size_t)256 * B, a.by_t = t->P + t->pl.by, a.colkl = h->colkl;
        RUN(K_SOFTMAX_SOFT, softmax_soft(h->Y + (size_t)256 * B, h->pr_stale ? nullptr : h->Pr + (size_t)256 * B, h->P + h->pl.by,
                                         h->ti + B, h->colloss, h->dby_part, 0, h->T,
                                         (h->cfg.flags & LSTM_HIP_STABLE_SOFTMAX) != 0, a, h->st));
        if (h->teacher) // the window's KL figure: every step, in bits, summed as the window loss is
            RUN(K_LOSS, loss_reduce(h->colkl, S - 1, B, h->global_B, h->d_kls + h->kl_idx, nullptr, 0, nullptr, h->st, 1.0f));
    } else
    if (h->text_window && h->tt_weight) // (lstm_hip_train_text_windows on weighted texts: dy = weight * (probs - target))
        RUN(K_SOFTMAX_WEIGHTED, softmax_loss_dy_weighted(h->Y + (size_t)256 * B, h->pr_stale ? nullptr : h->Pr + (size_t)256 * B,
                                                         h->P + h->pl.by, h->ti + B, h->tt_wt + B, h->colloss, h->dby_part, 0,
                                                         h->T, (h->cfg.flags & LSTM_HIP_STABLE_SOFTMAX) != 0, h->st));
    else
    if (h->text_window) // (lstm_hip_train_text_windows only: a column without a target gets dy = 0)
        RUN(K_SOFTMAX_TEXT, softmax_loss_dy_text(h->Y + (size_t)256 * B, h->pr_stale ? nullptr : h->Pr + (size_t)256 * B,
                                                 h->P + h->pl.by, h->ti + B, h->colloss, h->dby_part, 0, h->T,
                                                 (h->cfg.flags & LSTM_HIP_STABLE_SOFTMAX) != 0, h->st));
    else
    RUN(K_SOFTMAX, softmax_loss_dy(h->Y + (size_t)256 * B, h->pr_stale ? nullptr : h->Pr + (size_t)256 * B, h->P + h->pl.by,
                                   h->ti + B, h->colloss, h->dby_part, 0, h->T, (h->cfg.flags & LSTM_HIP_STABLE_SOFTMAX) != 0,
                                   h->st));
    h->fwd_done = true;
    return 0;
}

int do_backward(lstm_hip_ctx *h) {
    const EnginePlan &p = h->plan;
    const int N = h->cfg.N, B = h->cfg.B, S = h->cfg.S, G4 = 4 * N, T = h->T;
    if (!h->fwd_done && h->last_fwd_teacher)
        return fail(LSTM_HIP_ESTATE, "backward: this handle's last forward pass was a teacher's, not a training forward");
    if (!h->fwd_done) return fail(LSTM_HIP_ESTATE, "backward called before forward");
    float *dY = h->Y + (size_t)256 * B;
    // dby = rowsum(dY) (R/lstm.cc:227): folded with the loss when the loop runs on the device
    if (!h->dby_done)
        RUN(K_DBY, loss_reduce(loss_src(h), loss_steps(h), B, h->global_B, h->d_loss, h->dby_part, h->n_dby_parts,
                               h->dP + h->pl.by, h->st, loss_scale(h)));
    h->dby_done = false;
    // fused mode: the backward recurrence produces DHy = Why^T * dY (R/lstm.cc:228) itself and accumulates dW, db, dWhy
    const bool fused = p.fused;
    if (p.bf16()) { // DHy = Why^T * dY on bf16 operands: both already have the contraction index m contiguous
        RUN(K_GEMM_DHY, (pack_bf16(dY, (size_t)T * 256, h->dYb, h->st),
                         gemm_bf16(N, T, 256, h->Why_b, 256, h->dYb, 256, h->DHy + (size_t)N * B, N, 1, nullptr, h->st)));
    } else if (!fused && p.bwd != BwdForm::Scatter && p.bwd != BwdForm::Small) // (those compute Why^T dy themselves)
        RUN(K_GEMM_DHY, gemm(true, false, N, T, 256, h->P + h->pl.Why, 256, dY, 256, h->DHy + (size_t)N * B, N, 1, nullptr,
                             h->st));
    // Unfused two-half form, single GPU: the sums that do not feed the recurrence run on st2 beside it -- the column sort of
    // the dW pass and dWhy = dY H^T while the recurrence runs (one workgroup per CU leaves room), the dW / db sums beside
    // the dU product.  (Profiling runs keep everything on `st`, one timed launch after the other.)
    const bool side = p.side_stream && !h->comm && !h->profiling;
    if (side) {
        HIP_TRY(hipEventRecord(h->ev_fork, h->st));
        HIP_TRY(hipStreamWaitEvent(h->st2, h->ev_fork, 0));
        dW_sort(h->xi + B, T, G4, h->dw_scratch, h->st2);
        gemm(false, true, 256, N, T, dY, 256, h->H + (size_t)N * B, N, h->dP + h->pl.Why, 256, h->splits_dWhy, h->slabs, h->st2);
        if (int rc = launch_status(K_SIDE_SUMS)) return rc;
    }
    unsigned *cb = h->cnt + h->cnt_bytes / sizeof(unsigned);
    unsigned long long *stamps_b = h->stamps ? h->stamps + (size_t)2 * S * 16 : nullptr;
    float *gpart = fused ? h->gpart : nullptr;
    if (p.persistent()) {
        if (h->bwd_epoch >= p.epoch_limit) {
            HIP_TRY(hipMemsetAsync(cb, 0, h->cnt_bytes, h->st));
            h->bwd_epoch = 0;
            h->counter_resets++;
        }
        h->bwd_epoch++;
    }
    h->dgt_written = false;
    switch (p.bwd) {
    case BwdForm::Step:
        HIP_TRY(hipMemsetAsync(h->dcnext, 0, sizeof(float) * N * B, h->st)); // R/lstm.cc:216-217
        for (int t = S - 1; t >= 1; t--) {
            RUN(K_BWD_STEP, bwd_step(h->Ubwd, t < S - 1 ? h->DG + (size_t)(t + 1) * G4 * B : nullptr,
                                     h->DHy + (size_t)t * N * B, h->G + (size_t)t * G4 * B, h->C + (size_t)t * N * B,
                                     h->C + (size_t)(t - 1) * N * B, h->dcnext, h->DG + (size_t)t * G4 * B, N, B, h->st));
        }
        break;
    case BwdForm::Small:
        RUN(K_BWD_PERSIST, small_bwd(h->Ubwd, h->P + h->pl.Why, dY, h->G, h->C, h->DG, N, S, h->st));
        break;
    case BwdForm::Persistent:
    case BwdForm::Cols8:
        RUN(K_BWD_PERSIST, bwd_persistent(p.bwd == BwdForm::Cols8 ? h->Ubwd4 : h->Ubwd, h->DG, h->DHy, h->G, h->C, h->H, h->xi, gpart,
                                          h->P + h->pl.Why, dY, cb, h->abortp, h->bwd_epoch, N, S, B, p.bwd_cols, p.bwd_spread, h->st,
                                          stamps_b, nullptr));
        break;
    case BwdForm::Scatter: // one launch per co-resident range of columns; every group of the batch has its own ring region
        for (int c0 = 0; c0 < B; c0 += p.launch_cols) { // and partial gradient block
            if (c0 > 0) h->bwd_epoch++;
            RUN(K_BWD_PERSIST, bwd_scatter(h->Ubwd4, h->DG, h->P + h->pl.Why, dY, h->G, h->C, h->H, h->xi, gpart, h->DGx, cb, h->abortp,
                                           h->bwd_epoch, h->ring_base_b, N, S, B, p.bwd_cfg, c0, std::min(B - c0, p.launch_cols),
                                           p.group_cols, p.bwd_pin, h->st, stamps_b));
        }
        h->ring_base_b = bwds_ring_advance(h->ring_base_b, S);
        break;
    case BwdForm::Bf16:
        RUN(K_BWD_PERSIST, bwd_persistent(reinterpret_cast<const float4 *>(h->Ubwd16), h->DG, h->DHy, h->G, h->C, h->H, h->xi, nullptr,
                                          h->P + h->pl.Why, dY, cb, h->abortp, h->bwd_epoch, N, S, B, p.bwd_cols, p.bwd_spread, h->st,
                                          nullptr, h->DGb));
        break;
    case BwdForm::Bf16Scatter: // one launch per co-resident range of columns
        h->dgt_written = p.direct_dgt;
        for (int c0 = 0; c0 < B; c0 += p.launch_cols) {
            if (c0 > 0) h->bwd_epoch++;
            RUN(K_BWD_PERSIST, bwd_scatter_bf16(h->Ubwd6b, h->DG, h->DHy, h->G, h->C, h->DGx, cb, h->abortp, h->bwd_epoch,
                                                h->ring_base_b, N, S, B, c0, std::min(B - c0, p.launch_cols), p.group_cols,
                                                p.bwd_pin, h->st, stamps_b, p.direct_dgt ? h->DGt_b : nullptr, h->Tpad));
        }
        h->ring_base_b = bwd_scatter_bf16_ring_advance(h->ring_base_b, S); // (every group's region has had its S - 2 publications)
        break;
    }
    // dWhy = dY * H[1..]^T             R/lstm.cc:226
    if (p.bf16()) {
        // the contraction runs over the window's columns: k-contiguous bf16 images of dy, h and dg first (zero-padded to
        // Tpad); dy_t pairs with h_t, i.e. column (t-1)*B+b of dY with column t*B+b of H: the h image shifted by B columns
        RUN(K_GEMM_DWHY, (transpose_pack_bf16(dY, T, 256, 256, h->dYt_b, h->Tpad, h->st),
                          transpose_pack_bf16(h->H, S * B, N, N, h->Ht_b, h->SBpad, h->st),
                          gemm_bf16(256, N, h->Tpad, h->dYt_b, h->Tpad, h->Ht_b + B, h->SBpad, h->dP + h->pl.Why, 256,
                                    h->splits_dWhy, h->slabs, h->st)));
    } else if (!fused && !side)
        RUN(K_GEMM_DWHY, gemm(false, true, 256, N, T, dY, 256, h->H + (size_t)N * B, N, h->dP + h->pl.Why, 256,
                              h->splits_dWhy, h->slabs, h->st));
    // dW, db                           R/lstm.cc:251-252
    // Inside the single-GPU loop nobody reads the gradient block between here and Adagrad: the folds of the group
    // partials and of the dU slabs are left to the Adagrad launch (do_adagrad), three launches fewer per window.
    const bool defer_fold = fused && h->in_loop && !h->comm;
    h->dp_stale = defer_fold && !h->keep_outputs;
    if (defer_fold) {
        h->fold_pending = true;
    } else if (fused) { // accumulated per column group inside the recurrence: fold the groups in order
        const int NGb = (B + p.gpart_cols - 1) / p.gpart_cols;
        const size_t psz = bwd_partial_floats(N);
        // b and Why are adjacent both in the flat block and in the partial blocks: one fold covers both.  With the early
        // all-reduce below the folds go to st2 with it, so the dU product on `st` does not wait for them.
        const bool on_st2 = h->comm && h->in_loop && !h->profiling;
        hipStream_t fs = h->st;
        if (on_st2) {
            HIP_TRY(hipEventRecord(h->ev_fork, h->st));
            HIP_TRY(hipStreamWaitEvent(h->st2, h->ev_fork, 0));
            fs = h->st2;
        }
        RUN(K_DW_DB, (gemm_fold(h->gpart, NGb, G4 * 256, 1, h->dP + h->pl.W, G4 * 256, fs, psz),
                      gemm_fold(h->gpart + (size_t)G4 * 256 + (size_t)G4 * N, NGb, G4 + 256 * N, 1, h->dP + h->pl.b,
                                G4 + 256 * N, fs, psz)));
    } else if (side) {
        HIP_TRY(hipEventRecord(h->ev_mid, h->st)); // DG is complete
        HIP_TRY(hipStreamWaitEvent(h->st2, h->ev_mid, 0));
        dW_sums(h->DG + (size_t)G4 * B, T, G4, h->dP + h->pl.W, h->dP + h->pl.b, h->dw_scratch, h->st2);
        if (int rc = launch_status(K_SIDE_SUMS)) return rc;
        HIP_TRY(hipEventRecord(h->ev_join, h->st2));
    } else if (p.side_stream) {
        // a side-stream shape in a profiling pass or under a communicator: the side stream's own passes, in line.  (dW_db takes
        // its one-pass table for short windows, which sums in another order: a profiled window must give the bits of an
        // unprofiled one.)
        RUN(K_DW_DB, (dW_sort(h->xi + B, T, G4, h->dw_scratch, h->st),
                      dW_sums(h->DG + (size_t)G4 * B, T, G4, h->dP + h->pl.W, h->dP + h->pl.b, h->dw_scratch, h->st)));
    } else {
        RUN(K_DW_DB, dW_db(h->DG + (size_t)G4 * B, h->xi + B, T, G4, h->dP + h->pl.W, h->dP + h->pl.b, h->dw_scratch, h->st));
    }
    // Everything but dU is final here.  Inside the device-resident loop their all-reduce starts now, on st2, beside the dU
    // product: ranges [dW] and [db | dWhy | dby] of the flat block (one group).  The dU range follows on `st` behind the
    // product, ordered after ev_join, so the communicator never runs two collectives at once (do_allreduce).
    if (h->comm && h->in_loop && !h->profiling) {
        if (!fused) { // (fused: st2 already follows `st` from the end of the recurrence, with the folds queued on it)
            HIP_TRY(hipEventRecord(h->ev_fork, h->st));
            HIP_TRY(hipStreamWaitEvent(h->st2, h->ev_fork, 0));
        }
        int rc = 0;
        if (g_rccl.GroupStart && g_rccl.GroupEnd) g_rccl.GroupStart();
        rc = g_rccl.AllReduce(h->dP, h->dP, h->pl.U, /*ncclFloat*/ 7, /*ncclSum*/ 0, h->comm, h->st2);
        if (rc == 0)
            rc = g_rccl.AllReduce(h->dP + h->pl.b, h->dP + h->pl.b, h->pl.total - h->pl.b, 7, 0, h->comm, h->st2);
        if (g_rccl.GroupStart && g_rccl.GroupEnd) {
            const int rc2 = g_rccl.GroupEnd();
            if (rc == 0) rc = rc2;
        }
        if (rc != 0)
            return fail(LSTM_HIP_ERCCL, "ncclAllReduce (early ranges): %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "error");
        // With LSTM_HIP_DU_SPLIT=1 the dU product runs as two column halves and the first half's all-reduce also goes on st2,
        // behind the early ranges and beside the second half's product; only the second half is left for `st`.  Off by
        // default: two half-size products cost more than the whole one, about what hiding half of the dU all-reduce can
        // win back (measured with a 1-rank communicator, tools/comm_overhead_probe.py); to be decided on a multi-GPU node.
        // The switch is read at create (plan_engine) and the path depends on nothing else, so every rank of a job (same
        // environment) posts the same sequence of collectives.
        h->dU_reduced = 0;
        if (p.du_split) {
            int n1 = (N / 2) / 64 * 64; // whole 64-column tiles in the first half
            if (n1 == 0) n1 = N / 2;
            gemm(false, true, G4, n1, T, h->DG + (size_t)G4 * B, G4, h->H, N, h->dP + h->pl.U, G4, h->splits_dU, h->slabs_dU, h->st);
            if (int rc_ = launch_status(K_DU_HALVES)) return rc_;
            HIP_TRY(hipEventRecord(h->ev_mid, h->st));
            gemm(false, true, G4, N - n1, T, h->DG + (size_t)G4 * B, G4, h->H + n1, N, h->dP + h->pl.U + (size_t)G4 * n1, G4,
                 h->splits_dU, h->slabs_dU, h->st);
            if (int rc_ = launch_status(K_DU_HALVES)) return rc_;
            HIP_TRY(hipStreamWaitEvent(h->st2, h->ev_mid, 0));
            h->dU_reduced = (size_t)G4 * n1;
            rc = g_rccl.AllReduce(h->dP + h->pl.U, h->dP + h->pl.U, h->dU_reduced, 7, 0, h->comm, h->st2);
            if (rc != 0)
                return fail(LSTM_HIP_ERCCL, "ncclAllReduce (dU, first half): %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "error");
            h->n_slabs_dU = 0;
        }
        HIP_TRY(hipEventRecord(h->ev_join, h->st2));
        h->early_reduced = true;
        if (h->dU_reduced) return 0; // the product is done
    }
    // dU = DG * H[0..S-2]^T            R/lstm.cc:250
    if (p.bf16()) { // dg_t pairs with h_{t-1}: column (t-1)*B+b of both images
        h->n_slabs_dU = 0;
        RUN(K_GEMM_DU, (h->dgt_written ? (void)0 : transpose_pack_bf16(h->DG + (size_t)G4 * B, T, G4, G4, h->DGt_b, h->Tpad, h->st),
                        gemm_bf16(G4, N, h->Tpad, h->DGt_b, h->Tpad, h->Ht_b, h->SBpad, h->dP + h->pl.U, G4, h->splits_dU,
                                  h->slabs_dU, h->st)));
    } else if (defer_fold && h->splits_dU > 1 && !(h->wd_rate > 0.0)) // (weight drop masks the finished dU: no deferral)
        RUN(K_GEMM_DU, h->n_slabs_dU = gemm_slabs(false, true, G4, N, T, h->DG + (size_t)G4 * B, G4, h->H, N, h->slabs_dU,
                                                   h->splits_dU, h->st));
    else {
        h->n_slabs_dU = 0;
        RUN(K_GEMM_DU, gemm(false, true, G4, N, T, h->DG + (size_t)G4 * B, G4, h->H, N, h->dP + h->pl.U, G4, h->splits_dU,
                            h->slabs_dU, h->st));
    }
    // weight drop: dU <- keep ? dUe * s : 0, the gradient with respect to U itself, before any all-reduce, norm or update
    if (h->wd_rate > 0.0)
        if (int rc = weight_drop_launch(h, h->dP + h->pl.U, h->dP + h->pl.U)) return rc;
    if (side) HIP_TRY(hipStreamWaitEvent(h->st, h->ev_join, 0)); // the gradient block is complete on `st` from here
    return 0;
}

// SUM all-reduce of the flat gradient block [dW | dU | db | dWhy | dby] over the ranks (SUM, not mean: the reference's
// weight gradients are sums over batch columns, OV/lstm_eigen_opt/lstm.cc:271,297-299).  When do_backward has already
// started the ranges that were final before the dU product (early_reduced), only dU is left: it goes on `st` behind the
// product and behind ev_join, i.e. after the early ranges have finished on st2.
int do_allreduce(lstm_hip_ctx *h) {
    if (!h->comm) return 0;
    int rc = 0;
    if (h->early_reduced) {
        h->early_reduced = false;
        HIP_TRY(hipStreamWaitEvent(h->st, h->ev_join, 0));
        const size_t done = h->dU_reduced;
        h->dU_reduced = 0;
        RUN(K_ALLREDUCE, rc = g_rccl.AllReduce(h->dP + h->pl.U + done, h->dP + h->pl.U + done, h->pl.b - h->pl.U - done, 7, 0, h->comm,
                                               h->st));
    } else
    RUN(K_ALLREDUCE, rc = g_rccl.AllReduce(h->dP, h->dP, h->pl.total, /*ncclFloat*/ 7, /*ncclSum*/ 0, h->comm, h->st));
    if (rc != 0)
        return fail(LSTM_HIP_ERCCL, "ncclAllReduce: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "error");
    return 0;
}

// The running weight average (lstm_hip_set_averaging) after an update of a handle that asked for it: count the update and,
// when it is due, fold the parameters the update has just written into the average.  n and w are host numbers; the launch
// goes to the handle's stream behind the update launch, with no readback and no synchronisation.  Like pad_copy it is not
// one of the window's timed kernels: untimed_status and no statistics row.  The counters move only once the launch has
// been accepted.
int average_step(lstm_hip_ctx *h) {
    const int64_t seen = h->avg_seen + 1;
    if (seen % h->avg_every == 0) {
        const int64_t n = h->avg_n + 1;
        const float w = h->avg_kind == LSTM_HIP_AVG_EMA ? (float)(1.0 - h->avg_decay) : (float)(1.0 / (double)n);
        average(h->P, h->avg, h->pl.total, w, n == 1, h->plan.n_cus, h->st);
        if (int rc = untimed_status("average")) return rc;
        h->avg_n = n;
    }
    h->avg_seen = seen;
    return 0;
}
// the fp32 block the inference calls read (lstm_hip_set_inference_source); training never asks
const float *infer_block(const lstm_hip_ctx *h) { return h->infer_src == LSTM_HIP_SRC_AVERAGE ? h->avg : h->P; }

// One micro-window's gradient: the update, or under gradient accumulation (acc_every > 1) the accumulate launch and, at
// the last window of a cycle only, the update on the accumulated block.
// norm_idx: the slot of d_norms this step's norm goes to (clipping on only): the index of the update within the call
int do_adagrad(lstm_hip_ctx *h, double lr, int64_t norm_idx) {
    const EnginePlan &p = h->plan;
    const int N = h->cfg.N;
    uint64_t *pos_next = h->pos == h->pos_buf ? h->pos_buf + h->cfg.B : h->pos_buf;
    int32_t *head_next = h->head == h->head_buf ? h->head_buf + 1 : h->head_buf;
    const SlideJob slide{h->text, h->text_len, h->pos, h->Xr, h->Tr, h->head, h->xi, h->ti, h->H, h->C,
                         h->cfg.S, h->cfg.B, N, h->stride, h->carry_col, pos_next, head_next};
    const TailJob tail{loss_src(h), loss_steps(h), h->cfg.B, h->global_B, loss_scale(h), h->tail_loss, h->dby_part, h->n_dby_parts};
    AdagradJob job{};
    job.P = h->P, job.dP = h->dP, job.mem = h->mem, job.n = h->pl.total, job.u_off = h->pl.U, job.N = N, job.lr = (float)lr;
    // The same launch refreshes every live image of U: the fp32 ones in the layouts of the plan's forms; on the bf16 path (whose
    // one-recurrence images pack_U_bf16 repacks) the two-half images, whose 8-byte elements are the four rows an Adagrad thread
    // holds, and both bf16 copies of Why.
    if (!p.bf16()) {
        job.Ufwd = p.ufwd4() ? nullptr : h->Ufwd, job.Ubwd = p.ubwd4() ? nullptr : h->Ubwd;
        job.Ufwd4 = h->Ufwd4, job.Ubwd4 = h->Ubwd4, job.half_forms = p.half_forms();
    } else {
        job.u6b = h->Ubwd6b, job.u6_uw = bwd_scatter_bf16_units(N), job.uf6b = h->Ufwd6b, job.uf6_uw = fwd_halves_bf16_units(N);
        job.why_b = h->Why_b, job.whyT_b = h->WhyT_b, job.why_off = h->pl.Why;
    }
    if (h->fold_pending) { // the fused backward pass left the gradient in pieces (single-GPU loop)
        h->fold_pending = false;
        job.gpart = h->gpart, job.n_groups = (h->cfg.B + p.gpart_cols - 1) / p.gpart_cols, job.group_stride = bwd_partial_floats(N);
        job.slabs = h->n_slabs_dU > 0 ? h->slabs_dU : nullptr, job.n_slabs = h->n_slabs_dU, job.slab_stride = (size_t)4 * N * N;
        job.by_off = h->pl.by;
        job.skip_dP_store = !h->keep_outputs;
        job.tail = h->tail ? &tail : nullptr;
    } else if (h->tail)
        return fail(LSTM_HIP_ESTATE, "update launch: a loss tail without a pending gradient fold");
    h->tail = false;
    if (h->acc_every > 1) { // (loop_window keeps the tail off: the loss and dby are in place, keep_outputs is true)
        const bool last = h->acc_pending + 1 == h->acc_every;
        const int mode = last ? GRAD_ACC_LAST : h->acc_pending == 0 ? GRAD_ACC_FIRST : GRAD_ACC_ADD;
        RUN(K_GRAD_ACCUMULATE, grad_accumulate(job, h->acc, mode, h->acc_mean != 0, (float)(1.0 / (double)h->acc_every), h->st));
        if (!last) { // no update: the slide, if any, is the next window's own launch
            h->acc_pending++;
            h->carry_slide = false;
            return 0;
        }
        h->acc_pending = 0;
        job.gpart = nullptr, job.slabs = nullptr; // the gradient block holds the cycle's sum: the update reads it plainly
    }
    job.slide = h->carry_slide ? &slide : nullptr;
    job.quad = p.adagrad_quad;
    if (h->clip_max > 0.0) { // norm of the whole (summed, all-reduced) block first; the fold moves into k_grad_sumsq
        RUN(K_GRAD_SUMSQ, grad_sumsq(job, h->norm_part, h->st));
        RUN(K_GRAD_NORM, grad_norm(h->norm_part, grad_norm_parts(job.n), h->clip_max, h->d_norms + norm_idx, h->clip_coef, h->st));
        job.gpart = nullptr, job.slabs = nullptr;
        job.clip = h->clip_coef;
    }
    const bool adam = h->opt_kind == LSTM_HIP_OPT_ADAM;
    if (adam) { // this step's scalars, in double and narrowed (include/lstm_hip.h); t counts every update of the handle
        const double t = (double)(h->opt_steps + 1);
        job.v = h->adam_v;
        job.adam.decay = h->weight_decay > 0.0 ? (float)(1.0 - lr * h->weight_decay) : 1.0f;
        job.adam.omb1 = (float)(1.0 - h->beta1);
        job.adam.b2 = (float)h->beta2;
        job.adam.omb2 = (float)(1.0 - h->beta2);
        job.adam.step = (float)(lr / (1.0 - std::pow(h->beta1, t)));
        job.adam.bc2s = (float)std::sqrt(1.0 - std::pow(h->beta2, t));
        job.adam.eps = (float)h->adam_eps;
    }
    RUN(adam ? K_ADAM : K_ADAGRAD, adagrad(job, h->st));
    h->opt_steps++;
    h->call_updates++;
    if (job.slide) { // the launch wrote the next window's cursors and head to the other halves
        h->pre_slid = true;
        h->pos = pos_next;
        h->head = head_next;
    }
    h->carry_slide = false;
    h->img.update_ran(p, h->wd_rate > 0.0); // the same launch refreshed the images it is given above
    if (h->wd_rate > 0.0) h->wd_t++;        // weight drop: the next window has the next mask
    // the running average, in a launch of its own behind the update launch (never inside it: include/lstm_hip.h)
    if (h->avg_kind != LSTM_HIP_AVG_OFF) return average_step(h);
    return 0;
}

} // namespace

static int create_body(lstm_hip_ctx *h, const lstm_hip_config *cfg);

namespace {
// LSTM_HIP_PAD_HIDDEN: the internal width of a logical hidden size N >= 1 (include/lstm_hip.h).  A function of N and the flags
// only, never of S or B: the evaluator's B = 1 handle, the ranks of a communicator and an explicit Np handle must all agree
// on the layout.  0: refused.
int padded_hidden(int N, unsigned flags) {
    const auto up = [](int n, int k) { return (n + k - 1) / k * k; };
    if (flags & LSTM_HIP_STEP_KERNELS) return up(N, 16);
    if (flags & LSTM_HIP_BF16_RECURRENCE) return up(N, 128) <= 1024 ? up(N, 128) : 0;
    if (N <= 64 || N > 1024) return up(N, 16);
    if (N % 64 == 0) return N;
    // only these widths have forms for wide batches (the two-half forms at 256 / 512); a generic width's grid is not
    // co-resident at B = 1024 and would fall back to the per-step engine (448 against 512 for N = 400)
    for (int w : {128, 256, 512})
        if (N <= w) return w;
    return 1024;
}
} // namespace

extern "C" {

const char *lstm_hip_last_error(void) { return g_err; }

size_t lstm_hip_param_count(int32_t N, int32_t M) { return ParamLayout::make(N, M).total; }

int lstm_hip_device_info(int32_t device, char name[64], int32_t *cus, int32_t *clock_mhz) {
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (name) snprintf(name, 64, "%s (%s)", prop.name, prop.gcnArchName);
    if (cus) *cus = prop.multiProcessorCount;
    if (clock_mhz) *clock_mhz = prop.clockRate / 1000;
    return 0;
}

int lstm_hip_create(const lstm_hip_config *user_cfg, lstm_hip_t **out) {
    if (!user_cfg || !out) return fail(LSTM_HIP_EINVAL, "null argument");
    *out = nullptr;
    lstm_hip_config padded_cfg = *user_cfg; // from here on cfg->N is the internal width
    const lstm_hip_config *cfg = &padded_cfg;
    if (cfg->M != LSTM_HIP_VOCAB) return fail(LSTM_HIP_EINVAL, "M must be %d (got %d)", LSTM_HIP_VOCAB, cfg->M);
    if (cfg->flags & LSTM_HIP_PAD_HIDDEN) {
        if (cfg->N < 1 || cfg->N > (1 << 24)) return fail(LSTM_HIP_EINVAL, "N must be in [1, 2^24] (got %d)", cfg->N);
        padded_cfg.N = padded_hidden(user_cfg->N, cfg->flags);
        if (padded_cfg.N == 0)
            return fail(LSTM_HIP_EINVAL, "LSTM_HIP_BF16_RECURRENCE needs N <= 1024 (got %d)", user_cfg->N);
    } else if (cfg->N < 16 || cfg->N % 16 != 0)
        return fail(LSTM_HIP_EINVAL, "N must be a positive multiple of 16 (got %d)", cfg->N);
    if (cfg->S < 2) return fail(LSTM_HIP_EINVAL, "S must be >= 2 (got %d)", cfg->S);
    if (cfg->B < 1) return fail(LSTM_HIP_EINVAL, "B must be >= 1 (got %d)", cfg->B);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(LSTM_HIP_ENODEV, "no HIP device visible");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(LSTM_HIP_ENODEV, "device %d out of range (%d visible)", cfg->device, ndev);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, cfg->device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(LSTM_HIP_ENODEV, "device %d is %s; this library is built for gfx950 only", cfg->device, prop.gcnArchName);
    HIP_TRY(hipSetDevice(cfg->device));
    lds_device = cfg->device;
    // everything that can be refused is refused before the first allocation
    const EnginePlan plan = plan_engine(cfg->N, cfg->B, cfg->flags, prop.multiProcessorCount);
    if (plan.refusal[0]) return fail(LSTM_HIP_EINVAL, "%s", plan.refusal);

    lstm_hip_ctx *h = new lstm_hip_ctx();
    h->N_log = user_cfg->N;
    h->plan = plan;
    const int rc = create_body(h, cfg);
    if (rc != 0) {
        char keep[sizeof(g_err)];
        memcpy(keep, g_err, sizeof(keep)); // destroy must not overwrite the reason
        (void)lstm_hip_destroy(h);         // frees whatever had been allocated (the owner's list; the rest is null-checked)
        memcpy(g_err, keep, sizeof(keep));
        return rc;
    }
    *out = h;
    return 0;
}

} // extern "C"

static int create_body(lstm_hip_ctx *h, const lstm_hip_config *cfg) {
    h->cfg = *cfg;
    h->pl = ParamLayout::make(cfg->N, cfg->M);
    const size_t N = cfg->N, B = cfg->B, S = cfg->S, G4 = 4 * N;
    h->T = (int)((S - 1) * B);
    h->global_B = cfg->B;
    HIP_TRY(hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking));
    HIP_TRY(hipEventCreate(&h->ev0));
    HIP_TRY(hipEventCreate(&h->ev1));
    HIP_TRY(hipEventCreate(&h->evt0)); // train_windows' elapsed time (ev0 / ev1 belong to the per-kernel profiling)
    HIP_TRY(hipEventCreate(&h->evt1));
    { // first use of timed events on the stream, here rather than inside somebody's measurement
        float ms = 0.0f;
        HIP_TRY(hipEventRecord(h->evt0, h->st));
        HIP_TRY(hipEventRecord(h->evt1, h->st));
        HIP_TRY(hipEventSynchronize(h->evt1));
        HIP_TRY(hipEventElapsedTime(&ms, h->evt0, h->evt1));
    }
    const EnginePlan &p = h->plan;
    DeviceMem &m = h->own;
    TRY(m.alloc(h->P, h->pl.total));
    TRY(m.alloc(h->dP, h->pl.total));
    TRY(m.alloc(h->mem, h->pl.total));
    TRY(m.alloc(h->H, N * B * S));
    TRY(m.alloc(h->C, N * B * S));
    TRY(m.alloc(h->G, G4 * B * S));
    TRY(m.alloc(h->DG, G4 * B * S));
    TRY(m.alloc(h->Y, 256 * B * S));
    TRY(m.alloc(h->Pr, 256 * B * S));
    TRY(m.alloc(h->DHy, N * B * S));
    TRY(m.alloc(h->dcnext, N * B));
    TRY(m.alloc(h->colloss, B * S));
    TRY(m.alloc(h->dby_part, (size_t)256 * softmax_parts(h->T)));
    h->splits_dWhy = gemm_pick_splits(false, true, 256, (int)N, h->T, p.n_cus);
    h->splits_dU = gemm_pick_splits(false, true, (int)G4, (int)N, h->T, p.n_cus);
    if (p.bf16()) {
        h->Tpad = (h->T + 63) / 64 * 64;
        h->SBpad = ((int)B + h->Tpad + 63) / 64 * 64;
        h->splits_dWhy = gemm_bf16_pick_splits(256, (int)N, h->Tpad);
        h->splits_dU = gemm_bf16_pick_splits((int)G4, (int)N, h->Tpad);
    }
    TRY(m.alloc(h->slabs, (size_t)h->splits_dWhy * 256 * N));
    TRY(m.alloc(h->slabs_dU, (size_t)h->splits_dU * G4 * N));
    TRY(m.alloc(h->dw_scratch, dW_scratch_bytes(h->T, (int)G4)));
    TRY(m.alloc(h->xi, S * B, 0xff)); // -1: all-zero columns (opt:122,125)
    TRY(m.alloc(h->ti, S * B, 0xff));
    TRY(m.alloc(h->Xr, S * B, 0xff));
    TRY(m.alloc(h->Tr, S * B, 0xff));
    TRY(m.alloc(h->head_buf, 2));
    h->head = h->head_buf;
    TRY(m.alloc(h->d_loss, 1));
    TRY(m.alloc(h->pos_buf, 2 * (size_t)B));
    h->pos = h->pos_buf;
    h->cnt_bytes = persistent_counter_bytes((int)S, (int)B);
    TRY(m.alloc(h->cnt, 2 * h->cnt_bytes / sizeof(unsigned)));
    TRY(m.alloc(h->abortp, 4));
    // what the plan's forms use: weight images, bf16 operand copies, hand-off rings (sentinel-filled), partial blocks
    if (!p.bf16()) {
        TRY(m.alloc(h->Ufwd, N * N));
        TRY(m.alloc(h->Ubwd, N * N));
    }
    if (p.ufwd4()) TRY(m.alloc(h->Ufwd4, N * N));
    if (p.ubwd4()) TRY(m.alloc(h->Ubwd4, N * N));
    if (p.bf16()) {
        TRY(m.alloc(h->Hb, S * B * N));
        TRY(m.alloc(h->DGb, S * B * G4));
        TRY(m.alloc(h->WhyT_b, 256 * N));
        TRY(m.alloc(h->Why_b, 256 * N));
        TRY(m.alloc(h->Ht_b, N * (size_t)h->SBpad));
        TRY(m.alloc(h->dYt_b, (size_t)256 * h->Tpad));
        TRY(m.alloc(h->DGt_b, G4 * (size_t)h->Tpad));
        TRY(m.alloc(h->dYb, (size_t)h->T * 256));
    }
    if (p.u16) {
        TRY(m.alloc(h->Ufwd16, (size_t)8 * N * N, DeviceMem::kNoFill));
        TRY(m.alloc(h->Ubwd16, (size_t)8 * N * N, DeviceMem::kNoFill));
    }
    if (p.fwd == FwdForm::Bf16Halves) TRY(m.alloc(h->Ufwd6b, (size_t)8 * N * N, DeviceMem::kNoFill));
    if (p.bwd == BwdForm::Bf16Scatter) TRY(m.alloc(h->Ubwd6b, (size_t)8 * N * N, DeviceMem::kNoFill));
    if (p.hx_floats) TRY(m.alloc(h->Hx, p.hx_floats, 0xff));
    if (p.hxb_halfwords) TRY(m.alloc(h->Hxb, p.hxb_halfwords, 0xff));
    if (p.dgx_floats) TRY(m.alloc(h->DGx, p.dgx_floats, 0xff));
    if (p.fused) TRY(m.alloc(h->gpart, (size_t)((B + p.gpart_cols - 1) / p.gpart_cols) * bwd_partial_floats(cfg->N)));
    HIP_TRY(hipStreamCreateWithFlags(&h->st2, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&h->ev_mid, hipEventDisableTiming));
    if (p.stamps) TRY(m.alloc(h->stamps, 4 * S * 16));
    if (h->padded()) // the largest logical-width copy: the parameter block, or g of one step (4N x B; h0 and c0 for the sampler)
        TRY(m.alloc(h->stage, std::max({ParamLayout::make(h->N_log, cfg->M).total, (size_t)4 * h->N_log * B, (size_t)2 * h->N_log})));
    HIP_TRY(hipDeviceSynchronize());
    return 0;
}

extern "C" {

int lstm_hip_destroy(lstm_hip_t *h) {
    if (!h) return 0;
    if (h->lent > 0)
        return fail(LSTM_HIP_ESTATE, "destroy: %d student handle(s) hold this handle as their teacher (lstm_hip_set_soft_targets); "
                                     "clear or destroy them first", h->lent);
    (void)hipSetDevice(h->cfg.device);
    lds_device = h->cfg.device;
    if (h->teacher) h->teacher->lent--;
    h->teacher = nullptr;
    if (h->eval_h) (void)lstm_hip_destroy(h->eval_h);
    if (h->texts_h) (void)lstm_hip_destroy(h->texts_h);
    if (h->st) (void)hipStreamSynchronize(h->st);
    if (h->st2) (void)hipStreamSynchronize(h->st2);
    if (h->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(h->comm);
    h->own.free_all();
    for (hipEvent_t e : h->ev_soft)
        if (e) (void)hipEventDestroy(e);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->evt0) (void)hipEventDestroy(h->evt0);
    if (h->evt1) (void)hipEventDestroy(h->evt1);
    for (hipEvent_t e : {h->ev_fork, h->ev_join, h->ev_mid})
        if (e) (void)hipEventDestroy(e);
    if (h->st2) (void)hipStreamDestroy(h->st2);
    if (h->st) (void)hipStreamDestroy(h->st);
    delete h;
    return 0;
}

static float *block_of(lstm_hip_ctx *h, int which) {
    return which == 0 ? h->P : which == 1 ? h->dP : which == 2 ? h->mem : which == 3 ? h->adam_v : nullptr;
}
// which = 3 (Adam's second moment) exists only while the handle is on Adam
static int check_block(lstm_hip_ctx *h, int which, const char *what) {
    if (which == 3 && h->opt_kind != LSTM_HIP_OPT_ADAM)
        return fail(LSTM_HIP_ESTATE, "%s: block 3 (Adam's second moment) needs a handle set to LSTM_HIP_OPT_ADAM", what);
    return 0;
}

// one flat block between the host (logical N) and the device (internal width), synchronised
static int block_from_host(lstm_hip_ctx *h, float *dst, const float *host_block) {
    if (h->padded()) { // logical block -> staging -> padded block, padding entries 0
        const PadMap m = pad_map_params(h->N_log, h->cfg.N, h->cfg.M);
        HIP_TRY(hipMemcpyAsync(h->stage, host_block, sizeof(float) * m.total_l, hipMemcpyHostToDevice, h->st));
        pad_copy(h->stage, dst, m, true, h->st);
        if (int rc = untimed_status("pad_copy")) return rc;
    } else
    HIP_TRY(hipMemcpyAsync(dst, host_block, sizeof(float) * h->pl.total, hipMemcpyHostToDevice, h->st));
    HIP_TRY(hipStreamSynchronize(h->st));
    return 0;
}
static int block_to_host(lstm_hip_ctx *h, const float *src, float *host_block) {
    if (h->padded()) {
        const PadMap m = pad_map_params(h->N_log, h->cfg.N, h->cfg.M);
        pad_copy(src, h->stage, m, false, h->st);
        if (int rc = untimed_status("pad_copy")) return rc;
        HIP_TRY(hipMemcpyAsync(host_block, h->stage, sizeof(float) * m.total_l, hipMemcpyDeviceToHost, h->st));
    } else
    HIP_TRY(hipMemcpyAsync(host_block, src, sizeof(float) * h->pl.total, hipMemcpyDeviceToHost, h->st));
    HIP_TRY(hipStreamSynchronize(h->st));
    return 0;
}

int lstm_hip_set_params(lstm_hip_t *h, int which, const float *host_block) {
    CHECK(h);
    if (int rc = check_block(h, which, "set_params")) return rc;
    float *dst = block_of(h, which);
    if (!dst || !host_block) return fail(LSTM_HIP_EINVAL, "set_params: bad block id %d or null pointer", which);
    if (int rc = block_from_host(h, dst, host_block)) return rc;
    if (which == 0) h->img.params_written();
    return 0;
}
int lstm_hip_get_params(lstm_hip_t *h, int which, float *host_block) {
    CHECK(h);
    if (int rc = check_block(h, which, "get_params")) return rc;
    float *src = block_of(h, which);
    if (!src || !host_block) return fail(LSTM_HIP_EINVAL, "get_params: bad block id %d or null pointer", which);
    if (which == 1 && h->dp_stale)
        return fail(LSTM_HIP_ESTATE, "get_params: the gradient block holds no whole window (a window loop ended early); run backward first");
    if (int rc = block_to_host(h, src, host_block)) return rc;
    return check_abort(h);
}

int lstm_hip_set_state(lstm_hip_t *h, int32_t t, const float *h_t, const float *c_t) {
    if (h) h->pre_slid = false; // (a window slid ahead by an interrupted loop is not the caller's window any more)
    CHECK(h);
    if (t < 0 || t >= h->cfg.S) return fail(LSTM_HIP_EINVAL, "set_state: t=%d outside [0,%d)", t, h->cfg.S);
    const size_t n = (size_t)h->cfg.N * h->cfg.B;
    if (h->padded()) { // N_log x B -> staging -> Np x B (rows N_log.. zero)
        const PadMap m = pad_map_rows(1, h->N_log, h->cfg.N, h->cfg.B);
        for (int k = 0; k < 2; k++) {
            const float *src = k ? c_t : h_t;
            if (!src) continue;
            HIP_TRY(hipMemcpyAsync(h->stage, src, sizeof(float) * m.total_l, hipMemcpyHostToDevice, h->st));
            pad_copy(h->stage, (k ? h->C : h->H) + t * n, m, true, h->st);
            if (int rc = untimed_status("pad_copy")) return rc;
        }
        HIP_TRY(hipStreamSynchronize(h->st));
        return 0;
    }
    if (h_t) HIP_TRY(hipMemcpyAsync(h->H + t * n, h_t, sizeof(float) * n, hipMemcpyHostToDevice, h->st));
    if (c_t) HIP_TRY(hipMemcpyAsync(h->C + t * n, c_t, sizeof(float) * n, hipMemcpyHostToDevice, h->st));
    HIP_TRY(hipStreamSynchronize(h->st));
    return 0;
}
int lstm_hip_get_state(lstm_hip_t *h, int32_t t, float *h_t, float *c_t) {
    CHECK(h);
    if (t < 0 || t >= h->cfg.S) return fail(LSTM_HIP_EINVAL, "get_state: t=%d outside [0,%d)", t, h->cfg.S);
    const size_t n = (size_t)h->cfg.N * h->cfg.B;
    if (h->padded()) {
        const PadMap m = pad_map_rows(1, h->N_log, h->cfg.N, h->cfg.B);
        for (int k = 0; k < 2; k++) {
            float *dst = k ? c_t : h_t;
            if (!dst) continue;
            pad_copy((k ? h->C : h->H) + t * n, h->stage, m, false, h->st);
            if (int rc = untimed_status("pad_copy")) return rc;
            HIP_TRY(hipMemcpyAsync(dst, h->stage, sizeof(float) * m.total_l, hipMemcpyDeviceToHost, h->st));
            HIP_TRY(hipStreamSynchronize(h->st)); // (the staging buffer is reused for c)
        }
        return 0;
    }
    if (h_t) HIP_TRY(hipMemcpyAsync(h_t, h->H + t * n, sizeof(float) * n, hipMemcpyDeviceToHost, h->st));
    if (c_t) HIP_TRY(hipMemcpyAsync(c_t, h->C + t * n, sizeof(float) * n, hipMemcpyDeviceToHost, h->st));
    HIP_TRY(hipStreamSynchronize(h->st));
    return 0;
}
int lstm_hip_get_activations(lstm_hip_t *h, int32_t t, float *g_t, float *probs_t) {
    CHECK(h);
    if (t < 1 || t >= h->cfg.S) return fail(LSTM_HIP_EINVAL, "get_activations: t=%d outside [1,%d)", t, h->cfg.S);
    const size_t B = h->cfg.B, G4 = 4 * (size_t)h->cfg.N;
    if (probs_t && h->pr_stale)
        return fail(LSTM_HIP_ESTATE, "get_activations: the probabilities hold no whole window (a window loop ended early); run forward first");
    if (g_t && h->padded()) { // gate blocks [i;o;f;u] of Np rows -> of N_log rows
        const PadMap m = pad_map_rows(4, h->N_log, h->cfg.N, h->cfg.B);
        pad_copy(h->G + t * G4 * B, h->stage, m, false, h->st);
        if (int rc = untimed_status("pad_copy")) return rc;
        HIP_TRY(hipMemcpyAsync(g_t, h->stage, sizeof(float) * m.total_l, hipMemcpyDeviceToHost, h->st));
    } else
    if (g_t) HIP_TRY(hipMemcpyAsync(g_t, h->G + t * G4 * B, sizeof(float) * G4 * B, hipMemcpyDeviceToHost, h->st));
    if (probs_t) HIP_TRY(hipMemcpyAsync(probs_t, h->Pr + t * 256 * B, sizeof(float) * 256 * B, hipMemcpyDeviceToHost, h->st));
    HIP_TRY(hipStreamSynchronize(h->st));
    return 0;
}

int lstm_hip_set_window(lstm_hip_t *h, const int32_t *xi, const int32_t *ti) {
    if (h) h->pre_slid = false; // (a window slid ahead by an interrupted loop is not the caller's window any more)
    CHECK(h);
    if (!xi || !ti) return fail(LSTM_HIP_EINVAL, "set_window: null pointer");
    const size_t n = (size_t)h->cfg.S * h->cfg.B;
    for (size_t i = 0; i < n; i++)
        if (xi[i] >= LSTM_HIP_VOCAB || ti[i] >= LSTM_HIP_VOCAB)
            return fail(LSTM_HIP_EINVAL, "set_window: index %d/%d at %zu is >= %d", xi[i], ti[i], i, LSTM_HIP_VOCAB);
    HIP_TRY(hipMemcpyAsync(h->xi, xi, sizeof(int32_t) * n, hipMemcpyHostToDevice, h->st));
    HIP_TRY(hipMemcpyAsync(h->ti, ti, sizeof(int32_t) * n, hipMemcpyHostToDevice, h->st));
    HIP_TRY(hipMemcpyAsync(h->Xr, xi, sizeof(int32_t) * n, hipMemcpyHostToDevice, h->st)); // rings, head = 0
    HIP_TRY(hipMemcpyAsync(h->Tr, ti, sizeof(int32_t) * n, hipMemcpyHostToDevice, h->st));
    HIP_TRY(hipMemsetAsync(h->head, 0, sizeof(int32_t), h->st));
    HIP_TRY(hipStreamSynchronize(h->st));
    return 0;
}
int lstm_hip_set_inputs_dense(lstm_hip_t *h, const float *h0, const float *c0, const float *x, const float *target) {
    if (h) h->pre_slid = false; // (a window slid ahead by an interrupted loop is not the caller's window any more)
    CHECK(h);
    if (!x || !target) return fail(LSTM_HIP_EINVAL, "set_inputs_dense: null x or target");
    const size_t cols = (size_t)h->cfg.S * h->cfg.B;
    std::vector<int32_t> xi(cols), ti(cols);
    for (int which = 0; which < 2; which++) {
        const float *m = which ? target : x;
        std::vector<int32_t> &out = which ? ti : xi;
        for (size_t c = 0; c < cols; c++) {
            int32_t idx = -1;
            for (int r = 0; r < LSTM_HIP_VOCAB; r++) {
                const float v = m[c * LSTM_HIP_VOCAB + r];
                if (v == 0.0f) continue;
                if (v != 1.0f || idx >= 0)
                    return fail(LSTM_HIP_EINVAL, "set_inputs_dense: column %zu of %s is not one-hot (row %d holds %g)", c,
                                which ? "target" : "x", r, (double)v);
                idx = r;
            }
            out[c] = idx;
        }
    }
    int rc = lstm_hip_set_window(h, xi.data(), ti.data());
    if (rc) return rc;
    if (h0 || c0) return lstm_hip_set_state(h, 0, h0, c0);
    return 0;
}
int lstm_hip_get_window(lstm_hip_t *h, int32_t *xi, int32_t *ti) {
    CHECK(h);
    const size_t n = (size_t)h->cfg.S * h->cfg.B;
    if (xi) HIP_TRY(hipMemcpyAsync(xi, h->xi, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h->st));
    if (ti) HIP_TRY(hipMemcpyAsync(ti, h->ti, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h->st));
    HIP_TRY(hipStreamSynchronize(h->st));
    return 0;
}
int lstm_hip_reset_window(lstm_hip_t *h) {
    CHECK(h);
    const size_t n = (size_t)h->cfg.S * h->cfg.B;
    HIP_TRY(hipMemsetAsync(h->xi, 0xff, sizeof(int32_t) * n, h->st));
    HIP_TRY(hipMemsetAsync(h->ti, 0xff, sizeof(int32_t) * n, h->st));
    HIP_TRY(hipMemsetAsync(h->Xr, 0xff, sizeof(int32_t) * n, h->st));
    HIP_TRY(hipMemsetAsync(h->Tr, 0xff, sizeof(int32_t) * n, h->st));
    HIP_TRY(hipMemsetAsync(h->head, 0, sizeof(int32_t), h->st));
    return 0;
}

static int slide_state(lstm_hip_ctx *h) {
    const size_t n = (size_t)h->cfg.N * h->cfg.B;
    if (h->cfg.S < 2) return 0;
    HIP_TRY(hipMemcpyAsync(h->H, h->H + n, sizeof(float) * n, hipMemcpyDeviceToDevice, h->st));
    HIP_TRY(hipMemcpyAsync(h->C, h->C + n, sizeof(float) * n, hipMemcpyDeviceToDevice, h->st));
    return 0;
}
int lstm_hip_slide_state(lstm_hip_t *h) {
    CHECK(h);
    return slide_state(h);
}

int lstm_hip_forward(lstm_hip_t *h) {
    CHECK(h);
    if (int rc = soft_precheck(h, "forward")) return rc;
    TeacherStream ts{h};
    if (int rc = ts.begin()) return rc;
    h->kl_idx = 0;
    h->kls_n = -1;
    if (int rc = do_forward(h)) return rc;
    if (h->soft_on && h->teacher) h->kls_n = 1;
    return 0;
}
int lstm_hip_loss(lstm_hip_t *h, double *loss_bits) {
    CHECK(h);
    if (!loss_bits) return fail(LSTM_HIP_EINVAL, "loss: null pointer");
    if (!h->fwd_done) return fail(LSTM_HIP_ESTATE, "loss called before forward");
    RUN(K_LOSS, loss_reduce(loss_src(h), loss_steps(h), h->cfg.B, h->global_B, h->d_loss, nullptr, 0, nullptr, h->st, loss_scale(h)));
    HIP_TRY(hipMemcpyAsync(loss_bits, h->d_loss, sizeof(double), hipMemcpyDeviceToHost, h->st));
    HIP_TRY(hipStreamSynchronize(h->st));
    if (h->soft_on && h->teacher)
        if (int rc = check_abort(h->teacher)) return rc;
    return check_abort(h);
}
int lstm_hip_backward(lstm_hip_t *h) {
    CHECK(h);
    return do_backward(h);
}
int lstm_hip_adagrad(lstm_hip_t *h, double learning_rate) {
    CHECK(h);
    h->norms_n = -1;
    h->call_updates = 0;
    if (int rc = do_adagrad(h, learning_rate, h->call_updates)) return rc;
    if (h->clip_max > 0.0) h->norms_n = h->call_updates;
    return 0;
}

// global-norm clipping before every Adagrad step (include/lstm_hip.h).  The scratch memory is made on the first use and kept
// with the handle: d_norms grows with the longest train_windows call (train_windows, outside its loop).
static const int64_t FIGURES_FLOOR = 8192; // the least room a per-window array of figures (norms, KLs, losses) is given
static int ensure_norms(lstm_hip_ctx *h, int64_t count) {
    return h->own.grow(h->st, h->d_norms, h->norms_cap, count, FIGURES_FLOOR);
}
int lstm_hip_set_grad_clip(lstm_hip_t *h, double max_norm) {
    CHECK(h);
    if (std::isnan(max_norm) || max_norm < 0.0)
        return fail(LSTM_HIP_EINVAL, "set_grad_clip: max_norm must be >= 0 (0 = off, +inf = measure only; got %g)", max_norm);
    if (max_norm > 0.0) {
        if (int rc = ensure_norms(h, 1)) return rc;
        if (!h->norm_part) TRY(h->own.alloc(h->norm_part, grad_norm_parts(h->pl.total), DeviceMem::kNoFill));
        if (!h->clip_coef) TRY(h->own.alloc(h->clip_coef, 1, DeviceMem::kNoFill));
    }
    h->clip_max = max_norm;
    return 0;
}
int lstm_hip_get_grad_norms(lstm_hip_t *h, double *norms, int64_t n) {
    CHECK(h);
    if (h->norms_n < 0) return fail(LSTM_HIP_ESTATE, "get_grad_norms: clipping was off for the last adagrad / train_windows call");
    if (n < 0 || n > h->norms_n || (n > 0 && !norms))
        return fail(LSTM_HIP_EINVAL, "get_grad_norms: n = %lld outside [0, %lld] or null pointer", (long long)n, (long long)h->norms_n);
    if (n > 0) HIP_TRY(hipMemcpyAsync(norms, h->d_norms, sizeof(double) * n, hipMemcpyDeviceToHost, h->st));
    HIP_TRY(hipStreamSynchronize(h->st));
    return 0;
}

// gradient accumulation (include/lstm_hip.h).  The block is allocated when accumulation is first
// turned on and kept with the handle; a new (every, mean) pair starts an empty cycle, the same pair again keeps the cycle.
int lstm_hip_set_grad_accumulation(lstm_hip_t *h, int32_t every, int32_t mean) {
    CHECK(h);
    if (every < 1) return fail(LSTM_HIP_EINVAL, "set_grad_accumulation: every must be >= 1 (1 = off; got %d)", every);
    if (mean != 0 && mean != 1) return fail(LSTM_HIP_EINVAL, "set_grad_accumulation: mean must be 0 or 1 (got %d)", mean);
    if (every > 1 && h->comm)
        return fail(LSTM_HIP_ESTATE, "set_grad_accumulation: a handle with a communicator cannot accumulate gradients");
    if (every == h->acc_every && mean == h->acc_mean) return 0;
    if (every > 1 && !h->acc) TRY(h->own.alloc(h->acc, h->pl.total, DeviceMem::kNoFill));
    h->acc_every = every, h->acc_mean = mean, h->acc_pending = 0;
    return 0;
}
int lstm_hip_get_grad_accumulation(lstm_hip_t *h, int32_t *every, int32_t *mean, int32_t *pending) {
    if (!h || !every || !mean || !pending) return fail(LSTM_HIP_EINVAL, "get_grad_accumulation: null argument");
    *every = h->acc_every, *mean = h->acc_mean, *pending = h->acc_pending;
    return 0;
}
static int need_accumulation(lstm_hip_ctx *h, const char *what) {
    if (h->acc_every == 1) return fail(LSTM_HIP_ESTATE, "%s: gradient accumulation is off on this handle (lstm_hip_set_grad_accumulation)", what);
    return 0;
}
int lstm_hip_get_grad_accumulator(lstm_hip_t *h, float *host_block) {
    CHECK(h);
    if (!host_block) return fail(LSTM_HIP_EINVAL, "get_grad_accumulator: null pointer");
    if (int rc = need_accumulation(h, "get_grad_accumulator")) return rc;
    if (h->acc_pending == 0) { // (nothing summed yet: the block's bytes are those of an earlier cycle, or none)
        std::memset(host_block, 0, sizeof(float) * ParamLayout::make(h->N_log, h->cfg.M).total);
        return 0;
    }
    if (int rc = block_to_host(h, h->acc, host_block)) return rc;
    return check_abort(h);
}
int lstm_hip_set_grad_accumulator(lstm_hip_t *h, const float *host_block, int32_t pending) {
    CHECK(h);
    if (!host_block) return fail(LSTM_HIP_EINVAL, "set_grad_accumulator: null pointer");
    if (int rc = need_accumulation(h, "set_grad_accumulator")) return rc;
    if (pending < 0 || pending >= h->acc_every)
        return fail(LSTM_HIP_EINVAL, "set_grad_accumulator: pending must be in [0, %d] (got %d)", h->acc_every - 1, pending);
    if (int rc = block_from_host(h, h->acc, host_block)) return rc;
    h->acc_pending = pending;
    return 0;
}

// the update rule (include/lstm_hip.h).  A new kind starts from zero state: the memory / first moment, the second moment
// (allocated on the first switch to Adam, kept with the handle) and the step count.
int lstm_hip_set_optimizer(lstm_hip_t *h, int32_t kind, double beta1, double beta2, double eps, double weight_decay) {
    CHECK(h);
    if (kind == LSTM_HIP_OPT_ADAGRAD) {
        if (beta1 != 0.0 || beta2 != 0.0 || eps != 0.0 || weight_decay != 0.0)
            return fail(LSTM_HIP_EINVAL, "set_optimizer: LSTM_HIP_OPT_ADAGRAD takes no parameters (all four must be 0)");
    } else if (kind == LSTM_HIP_OPT_ADAM) {
        const bool ok = std::isfinite(beta1) && std::isfinite(beta2) && std::isfinite(eps) && std::isfinite(weight_decay) &&
                        beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps > 0.0 && weight_decay >= 0.0;
        if (!ok)
            return fail(LSTM_HIP_EINVAL, "set_optimizer: Adam needs 0 <= beta1, beta2 < 1, eps > 0 and weight_decay >= 0, all finite "
                                         "(got %g, %g, %g, %g)", beta1, beta2, eps, weight_decay);
    } else
        return fail(LSTM_HIP_EINVAL, "set_optimizer: unknown kind %d", kind);
    if (kind != h->opt_kind) {
        HIP_TRY(hipStreamSynchronize(h->st));
        if (kind == LSTM_HIP_OPT_ADAM && !h->adam_v) TRY(h->own.alloc(h->adam_v, h->pl.total, DeviceMem::kNoFill));
        HIP_TRY(hipMemsetAsync(h->mem, 0, sizeof(float) * h->pl.total, h->st));
        if (h->adam_v) HIP_TRY(hipMemsetAsync(h->adam_v, 0, sizeof(float) * h->pl.total, h->st));
        HIP_TRY(hipStreamSynchronize(h->st));
        h->opt_kind = kind;
        h->opt_steps = 0;
    }
    h->beta1 = beta1, h->beta2 = beta2, h->adam_eps = eps, h->weight_decay = weight_decay;
    return 0;
}
int lstm_hip_get_optimizer_steps(lstm_hip_t *h, int64_t *steps) {
    if (!h || !steps) return fail(LSTM_HIP_EINVAL, "get_optimizer_steps: null argument");
    *steps = h->opt_steps;
    return 0;
}
int lstm_hip_set_optimizer_steps(lstm_hip_t *h, int64_t steps) {
    if (!h) return fail(LSTM_HIP_EINVAL, "null handle");
    if (steps < 0) return fail(LSTM_HIP_EINVAL, "set_optimizer_steps: steps must be >= 0 (got %lld)", (long long)steps);
    h->opt_steps = steps;
    return 0;
}

// the running weight average and the inference source (include/lstm_hip.h).  A new kind starts from a zero block and zero
// counters, as a new optimizer kind does; the block is allocated on the first use and kept with the handle.
int lstm_hip_set_averaging(lstm_hip_t *h, int32_t kind, double decay, int32_t every) {
    CHECK(h);
    if (kind != LSTM_HIP_AVG_OFF && kind != LSTM_HIP_AVG_EMA && kind != LSTM_HIP_AVG_UNIFORM)
        return fail(LSTM_HIP_EINVAL, "set_averaging: unknown kind %d", kind);
    if (every < 1) return fail(LSTM_HIP_EINVAL, "set_averaging: every must be >= 1 (got %d)", every);
    if (kind == LSTM_HIP_AVG_EMA) {
        if (!std::isfinite(decay) || decay < 0.0 || decay >= 1.0)
            return fail(LSTM_HIP_EINVAL, "set_averaging: LSTM_HIP_AVG_EMA needs 0 <= decay < 1, finite (got %g)", decay);
    } else if (decay != 0.0) // (NaN compares unequal: refused here too)
        return fail(LSTM_HIP_EINVAL, "set_averaging: decay must be 0 for %s (got %g)",
                    kind == LSTM_HIP_AVG_OFF ? "LSTM_HIP_AVG_OFF" : "LSTM_HIP_AVG_UNIFORM", decay);
    if (kind != h->avg_kind) {
        if (kind != LSTM_HIP_AVG_OFF) {
            HIP_TRY(hipStreamSynchronize(h->st));
            if (!h->avg) TRY(h->own.alloc(h->avg, h->pl.total, DeviceMem::kNoFill));
            HIP_TRY(hipMemsetAsync(h->avg, 0, sizeof(float) * h->pl.total, h->st));
            HIP_TRY(hipStreamSynchronize(h->st));
        }
        h->avg_kind = kind;
        h->avg_seen = h->avg_n = 0;
        h->infer_src = LSTM_HIP_SRC_PARAMS; // (no average to read: off, or n = 0 again)
    }
    h->avg_decay = decay, h->avg_every = every;
    return 0;
}
static int need_averaging(lstm_hip_ctx *h, const char *what) {
    if (h->avg_kind == LSTM_HIP_AVG_OFF) return fail(LSTM_HIP_ESTATE, "%s: averaging is off on this handle (lstm_hip_set_averaging)", what);
    return 0;
}
int lstm_hip_get_average(lstm_hip_t *h, float *host_block) {
    CHECK(h);
    if (!host_block) return fail(LSTM_HIP_EINVAL, "get_average: null pointer");
    if (int rc = need_averaging(h, "get_average")) return rc;
    if (int rc = block_to_host(h, h->avg, host_block)) return rc;
    return check_abort(h);
}
int lstm_hip_set_average(lstm_hip_t *h, const float *host_block) {
    CHECK(h);
    if (!host_block) return fail(LSTM_HIP_EINVAL, "set_average: null pointer");
    if (int rc = need_averaging(h, "set_average")) return rc;
    return block_from_host(h, h->avg, host_block);
}
int lstm_hip_get_averaging_counts(lstm_hip_t *h, int64_t *seen, int64_t *n) {
    if (!h || !seen || !n) return fail(LSTM_HIP_EINVAL, "get_averaging_counts: null argument");
    if (int rc = need_averaging(h, "get_averaging_counts")) return rc;
    *seen = h->avg_seen, *n = h->avg_n;
    return 0;
}
int lstm_hip_set_averaging_counts(lstm_hip_t *h, int64_t seen, int64_t n) {
    if (!h) return fail(LSTM_HIP_EINVAL, "null handle");
    if (int rc = need_averaging(h, "set_averaging_counts")) return rc;
    if (n < 0 || n > seen)
        return fail(LSTM_HIP_EINVAL, "set_averaging_counts: needs 0 <= n <= seen (got seen = %lld, n = %lld)", (long long)seen, (long long)n);
    if (n == 0 && h->infer_src == LSTM_HIP_SRC_AVERAGE)
        return fail(LSTM_HIP_ESTATE, "set_averaging_counts: n = 0 while the inference source is LSTM_HIP_SRC_AVERAGE");
    h->avg_seen = seen, h->avg_n = n;
    return 0;
}
int lstm_hip_set_inference_source(lstm_hip_t *h, int32_t source) {
    if (!h) return fail(LSTM_HIP_EINVAL, "null handle");
    if (source != LSTM_HIP_SRC_PARAMS && source != LSTM_HIP_SRC_AVERAGE)
        return fail(LSTM_HIP_EINVAL, "set_inference_source: unknown source %d", source);
    if (source == LSTM_HIP_SRC_AVERAGE && (h->avg_kind == LSTM_HIP_AVG_OFF || h->avg_n == 0))
        return fail(LSTM_HIP_ESTATE, "set_inference_source: LSTM_HIP_SRC_AVERAGE needs averaging on and at least one averaged "
                                     "update (n >= 1): the average is still the zero block");
    h->infer_src = source;
    return 0;
}

// weight drop (include/lstm_hip.h).  Every call drops fwd_done and marks every image of U stale, so
// the next forward pass packs from the right source: Ue under the new (rate, seed, t), or the parameters once it is off.
static bool weight_drop_rate_ok(double rate) { return rate >= 0.0 && rate < 1.0; } // (NaN fails both comparisons)
int lstm_hip_set_weight_drop(lstm_hip_t *h, double rate, uint64_t seed, uint64_t t) {
    CHECK(h);
    if (!weight_drop_rate_ok(rate)) return fail(LSTM_HIP_EINVAL, "set_weight_drop: rate must be 0 (off) or 0 < rate < 1 (got %g)", rate);
    if (h->plan.du_split)
        return fail(LSTM_HIP_ESTATE, "set_weight_drop: this handle runs the dU product in halves (LSTM_HIP_DU_SPLIT), whose first "
                                     "half is all-reduced before the mask could be applied");
    if (rate > 0.0 && !h->Ue) {
        TRY(h->own.alloc(h->Ue, (size_t)4 * h->cfg.N * h->cfg.N, DeviceMem::kNoFill));
        HIP_TRY(hipMemsetAsync(h->Ue, 0, sizeof(float) * 4 * h->cfg.N * h->cfg.N, h->st));
    }
    h->wd_rate = rate, h->wd_seed = seed, h->wd_t = t;
    h->wd_thr = rate > 0.0 ? weight_drop::threshold(rate) : 0;
    h->wd_scale = rate > 0.0 ? weight_drop::scale(rate) : 1.0f;
    h->img.mask_changed();
    h->fwd_done = false;
    return 0;
}
int lstm_hip_get_weight_drop(lstm_hip_t *h, double *rate, uint64_t *seed, uint64_t *t) {
    if (!h || !rate || !seed || !t) return fail(LSTM_HIP_EINVAL, "get_weight_drop: null argument");
    *rate = h->wd_rate, *seed = h->wd_seed, *t = h->wd_t;
    return 0;
}
int lstm_hip_weight_drop_mask(int32_t N, double rate, uint64_t seed, uint64_t t, uint8_t *keep) {
    if (N < 1 || !keep) return fail(LSTM_HIP_EINVAL, "weight_drop_mask: need N >= 1 and an output pointer (got N = %d)", N);
    if (!weight_drop_rate_ok(rate)) return fail(LSTM_HIP_EINVAL, "weight_drop_mask: rate must be 0 (off) or 0 < rate < 1 (got %g)", rate);
    const uint64_t n = (uint64_t)4 * N * N;
    const uint32_t thr = rate > 0.0 ? weight_drop::threshold(rate) : 0; // (rate 0: every word >= 0, all kept)
    for (uint64_t q = 0; 4 * q < n; q++) {
        const weight_drop::Words w = weight_drop::quad_words(q, seed, t);
        for (uint64_t c = 0; c < 4 && 4 * q + c < n; c++) keep[4 * q + c] = weight_drop::keep_word(w.w[c], thr) ? 1 : 0;
    }
    return 0;
}

// soft targets (include/lstm_hip.h).  Everything is checked before anything changes; a successful call
// drops the forward pass, as lstm_hip_set_weight_drop does.
static int ensure_kls(lstm_hip_ctx *h, int64_t count);
int lstm_hip_set_soft_targets(lstm_hip_t *h, lstm_hip_t *teacher, const lstm_hip_soft_targets *opt) {
    CHECK(h);
    const char *what = "set_soft_targets";
    if (!opt && teacher) return fail(LSTM_HIP_EINVAL, "%s: a teacher needs options (opt is NULL)", what);
    lstm_hip_soft_targets o{(uint32_t)sizeof(lstm_hip_soft_targets), 1.0, 1.0, 0.0};
    if (opt) {
        if (opt->size != sizeof(lstm_hip_soft_targets))
            return fail(LSTM_HIP_EINVAL, "%s: opt->size is %u, not sizeof(lstm_hip_soft_targets) = %zu", what, opt->size,
                        sizeof(lstm_hip_soft_targets));
        o = *opt;
    }
    if (!(o.alpha >= 0.0 && o.alpha <= 1.0)) return fail(LSTM_HIP_EINVAL, "%s: alpha must lie in [0, 1] (got %g)", what, o.alpha);
    if (!(o.temperature > 0.0) || !std::isfinite(o.temperature))
        return fail(LSTM_HIP_EINVAL, "%s: temperature must be finite and > 0 (got %g)", what, o.temperature);
    if (!(o.smoothing >= 0.0 && o.smoothing < 1.0))
        return fail(LSTM_HIP_EINVAL, "%s: smoothing must lie in [0, 1) (got %g)", what, o.smoothing);
    if (!teacher && (o.alpha != 1.0 || o.temperature != 1.0))
        return fail(LSTM_HIP_EINVAL, "%s: without a teacher alpha and temperature must be 1 (got %g, %g)", what, o.alpha, o.temperature);
    if (teacher) {
        if (teacher == h) return fail(LSTM_HIP_EINVAL, "%s: a handle cannot be its own teacher", what);
        if (teacher->teacher) return fail(LSTM_HIP_EINVAL, "%s: the teacher has a teacher of its own", what);
        if (h->lent > 0) return fail(LSTM_HIP_EINVAL, "%s: this handle is itself held as a teacher", what);
        if (teacher->cfg.S != h->cfg.S || teacher->cfg.B != h->cfg.B || teacher->cfg.device != h->cfg.device)
            return fail(LSTM_HIP_EINVAL, "%s: the teacher's (S, B, device) = (%d, %d, %d) differ from the student's (%d, %d, %d)", what,
                        teacher->cfg.S, teacher->cfg.B, teacher->cfg.device, h->cfg.S, h->cfg.B, h->cfg.device);
    }
    const bool on = teacher || o.smoothing != 0.0;
    if (on && h->comm)
        return fail(LSTM_HIP_ESTATE, "%s: this handle has a communicator; soft targets run on one device", what);
    if (teacher) { // the teacher's memory, before anything changes
        if (!h->colkl) TRY(h->own.alloc(h->colkl, h->T, DeviceMem::kNoFill));
        if (int rc = ensure_kls(h, 1)) return rc;
        for (hipEvent_t &e : h->ev_soft)
            if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    if (h->teacher) h->teacher->lent--;
    h->teacher = teacher;
    if (teacher) teacher->lent++;
    h->soft_on = on;
    h->soft_opt = o;
    h->kls_n = -1;
    h->fwd_done = false;
    return 0;
}
int lstm_hip_get_soft_targets(lstm_hip_t *h, lstm_hip_t **teacher, lstm_hip_soft_targets *opt) {
    if (!h || !teacher || !opt) return fail(LSTM_HIP_EINVAL, "get_soft_targets: null argument");
    *teacher = h->teacher;
    *opt = lstm_hip_soft_targets{(uint32_t)sizeof(lstm_hip_soft_targets), 1.0, 1.0, 0.0};
    if (h->soft_on) *opt = h->soft_opt;
    return 0;
}
int lstm_hip_get_teacher_kl(lstm_hip_t *h, double *kl_bits, int64_t n) {
    CHECK(h);
    if (!h->teacher) return fail(LSTM_HIP_ESTATE, "get_teacher_kl: this handle has no teacher (lstm_hip_set_soft_targets)");
    if (h->kls_n < 0) return fail(LSTM_HIP_ESTATE, "get_teacher_kl: no forward / train_windows call since the teacher was set");
    if (n < 0 || n > h->kls_n || (n > 0 && !kl_bits))
        return fail(LSTM_HIP_EINVAL, "get_teacher_kl: n = %lld outside [0, %lld] or null pointer", (long long)n, (long long)h->kls_n);
    if (n > 0) HIP_TRY(hipMemcpyAsync(kl_bits, h->d_kls, sizeof(double) * n, hipMemcpyDeviceToHost, h->st));
    HIP_TRY(hipStreamSynchronize(h->st));
    return 0;
}

int lstm_hip_comm_unique_id(uint8_t id[LSTM_HIP_UNIQUE_ID_BYTES]) {
    int rc = rccl_load();
    if (rc) return rc;
    UniqueId u;
    rc = g_rccl.GetUniqueId(&u);
    if (rc != 0) return fail(LSTM_HIP_ERCCL, "ncclGetUniqueId failed (%d)", rc);
    memcpy(id, u.internal, LSTM_HIP_UNIQUE_ID_BYTES);
    return 0;
}
int lstm_hip_comm_init(lstm_hip_t *h, const uint8_t id[LSTM_HIP_UNIQUE_ID_BYTES], int32_t nranks, int32_t rank) {
    CHECK(h);
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail(LSTM_HIP_EINVAL, "comm_init: rank %d of %d", rank, nranks);
    if (h->soft_on) return fail(LSTM_HIP_ESTATE, "comm_init: soft targets are on (lstm_hip_set_soft_targets); they run on one device");
    if (h->acc_every > 1)
        return fail(LSTM_HIP_ESTATE, "comm_init: gradient accumulation is on (lstm_hip_set_grad_accumulation); it runs on one device");
    int rc = rccl_load();
    if (rc) return rc;
    UniqueId u;
    memcpy(u.internal, id, LSTM_HIP_UNIQUE_ID_BYTES);
    rc = g_rccl.CommInitRank(&h->comm, nranks, u, rank);
    if (rc != 0) {
        h->comm = nullptr;
        return fail(LSTM_HIP_ERCCL, "ncclCommInitRank: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "error");
    }
    h->nranks = nranks;
    h->rank = rank;
    return 0;
}
int lstm_hip_allreduce_grads(lstm_hip_t *h) {
    CHECK(h);
    return do_allreduce(h);
}

int lstm_hip_set_text(lstm_hip_t *h, const uint8_t *text, size_t len) {
    if (h) h->pre_slid = false; // (a window slid ahead by an interrupted loop is not the caller's window any more)
    CHECK(h);
    if (!text || len <= (size_t)h->cfg.S) return fail(LSTM_HIP_EINVAL, "set_text: need more than S=%d bytes (got %zu)", h->cfg.S, len);
    HIP_TRY(hipStreamSynchronize(h->st));
    TRY(h->own.release(h->text));
    TRY(h->own.alloc(h->text, len, DeviceMem::kNoFill));
    HIP_TRY(hipMemcpy(h->text, text, len, hipMemcpyHostToDevice));
    h->text_len = len;
    return 0;
}
int lstm_hip_set_cursors(lstm_hip_t *h, const uint64_t *pos) {
    if (h) h->pre_slid = false; // (a window slid ahead by an interrupted loop is not the caller's window any more)
    CHECK(h);
    if (!pos) return fail(LSTM_HIP_EINVAL, "set_cursors: null pointer");
    if (!h->text) return fail(LSTM_HIP_ESTATE, "set_cursors before set_text");
    for (int b = 0; b < h->cfg.B; b++)
        if (pos[b] >= h->text_len) return fail(LSTM_HIP_EINVAL, "set_cursors: pos[%d]=%llu >= len %llu", b, (unsigned long long)pos[b], (unsigned long long)h->text_len);
    HIP_TRY(hipMemcpyAsync(h->pos, pos, sizeof(uint64_t) * h->cfg.B, hipMemcpyHostToDevice, h->st));
    HIP_TRY(hipStreamSynchronize(h->st));
    return 0;
}
int lstm_hip_get_cursors(lstm_hip_t *h, uint64_t *pos) {
    CHECK(h);
    if (!pos) return fail(LSTM_HIP_EINVAL, "get_cursors: null pointer");
    HIP_TRY(hipMemcpyAsync(pos, h->pos, sizeof(uint64_t) * h->cfg.B, hipMemcpyDeviceToHost, h->st));
    HIP_TRY(hipStreamSynchronize(h->st));
    return 0;
}
int lstm_hip_set_stride(lstm_hip_t *h, int32_t stride, int32_t carry_col) {
    if (h) h->pre_slid = false; // (a window slid ahead by an interrupted loop is not the caller's window any more)
    if (!h) return fail(LSTM_HIP_EINVAL, "null handle");
    if (stride < 1 || stride >= h->cfg.S || carry_col < 0 || carry_col >= h->cfg.S)
        return fail(LSTM_HIP_EINVAL, "set_stride: need 1 <= stride < S and 0 <= carry_col < S (got %d, %d)", stride, carry_col);
    h->stride = stride;
    h->carry_col = carry_col;
    return 0;
}
int lstm_hip_set_global_batch(lstm_hip_t *h, int32_t global_B) {
    if (!h || global_B < h->cfg.B) return fail(LSTM_HIP_EINVAL, "set_global_batch: %d < local B", global_B);
    h->global_B = global_B;
    return 0;
}

int lstm_hip_set_loss_mode(lstm_hip_t *h, int32_t mode) {
    if (!h || (mode != LSTM_HIP_LOSS_ALL_STEPS_BITS && mode != LSTM_HIP_LOSS_LAST_STEP_NATS && mode != LSTM_HIP_LOSS_LAST_STEP_BITS))
        return fail(LSTM_HIP_EINVAL, "set_loss_mode: unknown mode %d", mode);
    h->loss_mode = mode;
    return 0;
}

// the window loops (lstm_hip_train_windows, the adaptive coder): room for `count` per-window losses
static int ensure_kls(lstm_hip_ctx *h, int64_t count) {
    return h->own.grow(h->st, h->d_kls, h->kls_cap, count, FIGURES_FLOOR);
}
static int ensure_losses(lstm_hip_ctx *h, int64_t count) { // the device array and its pinned twin grow together
    if (count <= h->losses_cap) return 0;
    TRY(h->own.grow(h->st, h->d_losses, h->losses_cap, count, FIGURES_FLOOR));
    TRY(h->own.release(h->h_losses));
    const int rc = h->own.alloc_pinned(h->h_losses, (size_t)h->losses_cap);
    if (rc) h->losses_cap = 0; // (no twin: the next call makes both again)
    return rc;
}
// One window of a device-resident loop, before its forward pass: does its loss ride in the update launch (wherever the
// gradient fold does, do_backward's defer_fold, but not under clipping -- the norm needs dby first -- nor in a profiling pass,
// which times the launches one by one, nor under gradient accumulation, whose accumulating windows have no update launch),
// and does it store the probabilities and the folded gradient (`last`: nothing inside
// the loop reads them, and only the last window's can be seen afterwards).  Returns whether the caller launches the loss itself.
static bool loop_window(lstm_hip_ctx *h, bool last, double *loss_out) {
    h->tail = h->plan.fused && !h->comm && !h->profiling && !(h->clip_max > 0.0) && h->acc_every == 1;
    h->tail_loss = loss_out;
    h->keep_outputs = last || !h->tail;
    return !h->tail;
}
struct LoopGuard { // leaves the loop state clean on every return path
    lstm_hip_ctx *h;
    bool completed = false;
    ~LoopGuard() {
        h->in_loop = false;
        h->keep_outputs = true;
        if (completed) return;
        // error exit somewhere inside a window: nothing of that window may leak into a later standalone call
        h->fold_pending = false;
        h->early_reduced = false;
        h->dU_reduced = 0;
        h->n_slabs_dU = 0;
        h->dby_done = false;
        h->fwd_done = false;
        h->carry_slide = false;
        h->tail = false;
        h->pr_stale = h->dp_stale = true; // (whichever window broke: its stores may have been skipped or never reached)
        if (h->st2) (void)hipStreamSynchronize(h->st2); // side-stream work of the broken window (folds, early all-reduce)
        if (h->st) (void)hipStreamSynchronize(h->st);
    }
};

int lstm_hip_train_windows(lstm_hip_t *h, int64_t count, double learning_rate, double *losses, float *elapsed_ms) {
    CHECK(h);
    if (count < 0) return fail(LSTM_HIP_EINVAL, "train_windows: count < 0");
    if (!h->text) return fail(LSTM_HIP_ESTATE, "train_windows before set_text/set_cursors");
    if (int rc = soft_precheck(h, "train_windows")) return rc;
    if (int rc = ensure_losses(h, count)) return rc;
    const bool distil = h->soft_on && h->teacher;
    h->kls_n = -1;
    if (distil)
        if (int rc = ensure_kls(h, count)) return rc;
    TeacherStream ts{h};
    if (int rc = ts.begin()) return rc;
    struct KlIndex { // the single-window calls fold their figure into slot 0
        lstm_hip_ctx *h;
        ~KlIndex() { h->kl_idx = 0; }
    } kl_index{h};
    h->norms_n = -1;
    h->call_updates = 0;
    const bool clip = h->clip_max > 0.0;
    if (clip)
        if (int rc = ensure_norms(h, count)) return rc;
    // the handle's own event pair (made and exercised once at create: the first timed record on a stream costs ~0.5 ms of
    // device time, which a 20-window measurement would carry)
    if (elapsed_ms) HIP_TRY(hipEventRecord(h->evt0, h->st));
    h->in_loop = true;
    LoopGuard guard{h};
    for (int64_t i = 0; i < count; i++) {
        // (from the second window on the slide has been done by the previous window's Adagrad launch, in extra workgroups)
        if (!h->pre_slid)
            RUN(K_SLIDE, slide_window(h->text, h->text_len, h->pos, h->Xr, h->Tr, h->head, h->xi, h->ti, h->H, h->C,
                                      h->cfg.S, h->cfg.B, h->cfg.N, h->stride, h->carry_col, h->st));
        h->pre_slid = false;
        int rc = 0;
        const bool own_loss = loop_window(h, i + 1 == count, h->d_losses + i);
        h->kl_idx = i;
        if ((rc = do_forward(h))) return rc;
        if (own_loss)
            RUN(K_LOSS, loss_reduce(loss_src(h), loss_steps(h), h->cfg.B, h->global_B, h->d_losses + i, h->dby_part,
                                    h->n_dby_parts, h->dP + h->pl.by, h->st, loss_scale(h)));
        h->dby_done = true;
        if ((rc = do_backward(h))) return rc;
        if ((rc = do_allreduce(h))) return rc;
        // not behind the last window (the handle is left on the window it trained on) and not in a profiling pass.  The
        // paths that keep their separate loss launch (loop_window) also keep the slide's for windows above 2 048 columns.
        h->carry_slide = i + 1 < count && !h->profiling && (h->tail || (int64_t)h->cfg.S * h->cfg.B <= 2048);
        if ((rc = do_adagrad(h, learning_rate, h->call_updates))) return rc;
    }
    if (elapsed_ms) {
        HIP_TRY(hipEventRecord(h->evt1, h->st));
        HIP_TRY(hipEventSynchronize(h->evt1));
        HIP_TRY(hipEventElapsedTime(elapsed_ms, h->evt0, h->evt1));
    }
    if (losses && count > 0)
        HIP_TRY(hipMemcpyAsync(h->h_losses, h->d_losses, sizeof(double) * count, hipMemcpyDeviceToHost, h->st));
    HIP_TRY(hipStreamSynchronize(h->st));
    if (losses && count > 0) std::memcpy(losses, h->h_losses, sizeof(double) * count);
    guard.completed = true;
    if (clip) h->norms_n = h->call_updates; // (one norm per update: `count` of them unless gradient accumulation is on)
    if (distil) {
        h->kls_n = count;
        if (int rc = check_abort(h->teacher)) return rc; // (still on this stream, which has just been drained)
    }
    return check_abort(h);
}

// test(), OV/lstm_eigen_class_CUDA/lstm.cc:661-720: one stream from h = c = 0, bits/char over the text.
// Where the persistent forward recurrence exists for this hidden size, the text is run through it in
// chunks on an internal B = 1 handle (the carry moves from the last column of a chunk to column 0 of the
// next); otherwise by the single-workgroup kernel.
// internal B = 1 handle behind the evaluator (its own copy of the parameters and their fragment images)
static const int AUX_S = 129; // 128 characters per evaluator chunk
static int ensure_aux_handle(lstm_hip_ctx *h) {
    if (h->eval_h) return 0;
    lstm_hip_config c = h->cfg; // (cfg.N is the parent's internal width: a padded parent's aux handle is an unpadded Np one)
    c.S = AUX_S;
    c.B = 1;
    c.flags = (h->cfg.flags & (LSTM_HIP_FAST_MATH | LSTM_HIP_STABLE_SOFTMAX)) | LSTM_HIP_NO_FUSED_GRADS;
    return lstm_hip_create(&c, &h->eval_h);
}

// The one-workgroup evaluator and sampler of a handle on the per-step engine keep h, c and the gates in LDS: refused, before
// anything is allocated, where the device cannot grant that much to one workgroup.
static int b1_lds_check(lstm_hip_ctx *h, const char *who) {
    int optin = 0;
    HIP_TRY(hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin, h->cfg.device));
    const size_t need = b1_lds_bytes(h->cfg.N);
    if (need > (size_t)optin)
        return fail(LSTM_HIP_EINVAL, "%s: N=%d (internal width %d) needs %zu bytes of LDS in one workgroup, the device grants %d (N <= %d)",
                    who, h->N_log, h->cfg.N, need, optin, (optin / 4 - 256) / 6 / 16 * 16);
    return 0;
}
static int b1_status(const char *who, hipError_t e) {
    if (e != hipSuccess) return fail(LSTM_HIP_EHIP, "launch of %s failed: %s", who, hipGetErrorString(e));
    return 0;
}

int lstm_hip_eval_bits(lstm_hip_t *h, const uint8_t *text, size_t len, double *bits_per_char) {
    CHECK(h);
    if (!text || len < 2 || !bits_per_char) return fail(LSTM_HIP_EINVAL, "eval_bits: need >= 2 bytes and an output pointer");
    const int N = h->cfg.N;
    if (!h->plan.persistent()) {
        if (int rc = b1_lds_check(h, "eval_bits")) return rc;
        DeviceTemp<uint8_t> d_text;
        TRY(d_text.alloc(len));
        HIP_TRY(hipMemcpyAsync(d_text, text, len, hipMemcpyHostToDevice, h->st));
        // (one spelling per source: tests/test_hidden_widths_cpu.py pins the text of the launch from the parameters)
        const bool stable = (h->cfg.flags & LSTM_HIP_STABLE_SOFTMAX) != 0;
        if (int rc = h->infer_src == LSTM_HIP_SRC_AVERAGE
                         ? b1_status("eval_bits", eval_bits(h->avg, N, d_text, len, h->d_loss, nullptr, stable, h->st))
                         : b1_status("eval_bits", eval_bits(h->P, N, d_text, len, h->d_loss, nullptr, stable, h->st)))
            return rc;
        double sum = 0.0;
        HIP_TRY(hipMemcpyAsync(&sum, h->d_loss, sizeof(double), hipMemcpyDeviceToHost, h->st));
        HIP_TRY(hipStreamSynchronize(h->st));
        *bits_per_char = sum / (double)(len - 1);
        return 0;
    }
    HIP_TRY(hipStreamSynchronize(h->st));
    const int Se = AUX_S;
    {
        int rc = ensure_aux_handle(h);
        if (rc) return rc;
    }
    lstm_hip_ctx *e = h->eval_h;
    HIP_TRY(hipMemcpy(e->P, infer_block(h), sizeof(float) * h->pl.total, hipMemcpyDeviceToDevice));
    if (e->plan.bf16()) return fail(LSTM_HIP_ESTATE, "eval_bits: the internal handle is not fp32"); // (ensure_aux_handle: its only live flag is `packed`)
    e->img.params_written();
    HIP_TRY(hipMemset(e->H, 0, sizeof(float) * N)); // h = c = 0 (reset_std = 0, lstm.cc:45,676-677)
    HIP_TRY(hipMemset(e->C, 0, sizeof(float) * N));
    std::vector<int32_t> xi(Se), ti(Se);
    double sum = 0.0;
    for (size_t pos = 0; pos + 1 < len; pos += Se - 1) {
        const size_t steps = std::min<size_t>(Se - 1, len - 1 - pos);
        xi[0] = ti[0] = -1;
        for (int t = 1; t < Se; t++) {
            const bool in = (size_t)t <= steps;
            xi[t] = in ? (int32_t)text[pos + t - 1] : -1; // past the end: empty columns, no loss
            ti[t] = in ? (int32_t)text[pos + t] : -1;
        }
        int rc = lstm_hip_set_window(e, xi.data(), ti.data());
        if (rc) return rc;
        if ((rc = do_forward(e))) return rc;
        double part = 0.0;
        if ((rc = lstm_hip_loss(e, &part))) return rc;
        sum += part;
        // carry: the state after the chunk's last real character becomes column 0
        HIP_TRY(hipMemcpyAsync(e->H, e->H + (size_t)steps * N, sizeof(float) * N, hipMemcpyDeviceToDevice, e->st));
        HIP_TRY(hipMemcpyAsync(e->C, e->C + (size_t)steps * N, sizeof(float) * N, hipMemcpyDeviceToDevice, e->st));
    }
    HIP_TRY(hipStreamSynchronize(e->st));
    *bits_per_char = sum / (double)(len - 1);
    return 0;
}

int lstm_hip_sample(lstm_hip_t *h, float *h0, float *c0, const double *u, int32_t count, uint8_t *out) {
    CHECK(h);
    if (!h0 || !c0 || !u || !out || count < 0) return fail(LSTM_HIP_EINVAL, "sample: null pointer or negative count");
    // Persistent engine: the batched generator with one stream (per character one gen_head and one k_fwd_step launch; the
    // sampled byte never leaves the device).  (k_sample does the whole 4N x N product in ONE workgroup: 395 us per
    // character at N = 512.)  Fixed cost per call: one pack_U of the current U (4N^2 floats, about 10 us at N = 512; P
    // changes under many calls, so the image is not cached) and the uploads; the scratch memory stays with the handle.
    if (h->plan.persistent() && count > 0)
        return lstm_hip_generate(h, 1, nullptr, nullptr, h0, c0, 1.0, u, count, out, nullptr, h0, c0);
    const int N = h->cfg.N;
    if (int rc = b1_lds_check(h, "sample")) return rc;
    DeviceTemp<float> d_hc;
    DeviceTemp<double> d_u;
    DeviceTemp<uint8_t> d_out;
    TRY(d_hc.alloc((size_t)2 * N));
    TRY(d_u.alloc((size_t)count + 1));
    TRY(d_out.alloc((size_t)count + 1));
    const PadMap hc_map = pad_map_rows(1, h->N_log, N, 2); // [h | c] as two columns
    if (h->padded()) {
        HIP_TRY(hipMemcpyAsync(h->stage, h0, sizeof(float) * h->N_log, hipMemcpyHostToDevice, h->st));
        HIP_TRY(hipMemcpyAsync(h->stage + h->N_log, c0, sizeof(float) * h->N_log, hipMemcpyHostToDevice, h->st));
        pad_copy(h->stage, d_hc, hc_map, true, h->st);
        if (int rc = untimed_status("pad_copy")) return rc;
    } else {
        HIP_TRY(hipMemcpyAsync(d_hc, h0, sizeof(float) * N, hipMemcpyHostToDevice, h->st));
        HIP_TRY(hipMemcpyAsync(d_hc + N, c0, sizeof(float) * N, hipMemcpyHostToDevice, h->st));
    }
    HIP_TRY(hipMemcpyAsync(d_u, u, sizeof(double) * count, hipMemcpyHostToDevice, h->st));
    const bool stable = (h->cfg.flags & LSTM_HIP_STABLE_SOFTMAX) != 0; // (one spelling per source, as in lstm_hip_eval_bits)
    if (int rc = h->infer_src == LSTM_HIP_SRC_AVERAGE ? b1_status("sample", sample(h->avg, N, d_hc, d_u, count, d_out, nullptr, stable, h->st))
                                                      : b1_status("sample", sample(h->P, N, d_hc, d_u, count, d_out, nullptr, stable, h->st)))
        return rc;
    if (h->padded()) {
        pad_copy(d_hc, h->stage, hc_map, false, h->st);
        if (int rc = untimed_status("pad_copy")) return rc;
        HIP_TRY(hipMemcpyAsync(h0, h->stage, sizeof(float) * h->N_log, hipMemcpyDeviceToHost, h->st));
        HIP_TRY(hipMemcpyAsync(c0, h->stage + h->N_log, sizeof(float) * h->N_log, hipMemcpyDeviceToHost, h->st));
    } else {
        HIP_TRY(hipMemcpyAsync(h0, d_hc, sizeof(float) * N, hipMemcpyDeviceToHost, h->st));
        HIP_TRY(hipMemcpyAsync(c0, d_hc + N, sizeof(float) * N, hipMemcpyDeviceToHost, h->st));
    }
    HIP_TRY(hipMemcpyAsync(out, d_out, count, hipMemcpyDeviceToHost, h->st));
    HIP_TRY(hipStreamSynchronize(h->st));
    return 0;
}

} // extern "C"

// ---- what generate, beam search, score and the coders share around their loops (the loops themselves differ and stay apart)
namespace {

// the generator's and the coder's working memory: one allocation on the handle, grown to the largest call
int reserve_gen_scratch(lstm_hip_t *h, size_t bytes) { // (no floor: the first call's size)
    return h->own.grow(h->st, h->gen_scratch, h->gen_scratch_bytes, bytes);
}

// A call's layout of that memory: 256-byte aligned pieces in the order they are named.  Each piece is named once: the pointer
// to fill, its element count, and whether it is there at all.  An absent piece takes no room and leaves its pointer null (the
// kernels test some of them); a present one gets an address even when it has no elements.  commit reserves the sum and fills
// the pointers.
class Scratch {
    struct Piece {
        void *slot; // the caller's T *
        size_t at;
    };
    std::vector<Piece> pieces;
    size_t bytes = 0;

  public:
    template <class T> Scratch &piece(T *&p, size_t count, bool present = true) {
        p = nullptr;
        if (present) {
            pieces.push_back({&p, bytes});
            bytes += (count * sizeof(T) + 255) / 256 * 256;
        }
        return *this;
    }
    int commit(lstm_hip_t *h) {
        if (int rc = reserve_gen_scratch(h, bytes)) return rc;
        for (const Piece &q : pieces) {
            char *at = h->gen_scratch + q.at;
            memcpy(q.slot, &at, sizeof(at));
        }
        return 0;
    }
};

// The start state of `cols` columns, host h0 / c0 (either may be null: zeros) to the device's H / Cs.  A padded handle takes
// the logical-width columns through `stage` ([2][cols * N_log], a piece of the call's scratch) and pad_copy: padding rows zero.
// (N, N_log: the internal and the logical width of the model whose state it is -- the handle's own, or a guide's)
int upload_states(lstm_hip_t *h, int N, int N_log, const float *h0, const float *c0, float *H, float *Cs, float *stage, int cols) {
    const size_t n = (size_t)N * cols, nl = (size_t)N_log * cols;
    const PadMap map = pad_map_rows(1, N_log, N, cols);
    for (int k = 0; k < 2; k++) {
        const float *src = k ? c0 : h0;
        float *dst = k ? Cs : H;
        if (!src) HIP_TRY(hipMemsetAsync(dst, 0, sizeof(float) * n, h->st));
        else if (N_log != N) {
            HIP_TRY(hipMemcpyAsync(stage + k * nl, src, sizeof(float) * nl, hipMemcpyHostToDevice, h->st));
            pad_copy(stage + k * nl, dst, map, true, h->st);
            if (int rc = untimed_status("pad_copy")) return rc;
        } else
            HIP_TRY(hipMemcpyAsync(dst, src, sizeof(float) * n, hipMemcpyHostToDevice, h->st));
    }
    return 0;
}
int upload_states(lstm_hip_t *h, const float *h0, const float *c0, float *H, float *Cs, float *stage, int cols) {
    return upload_states(h, h->cfg.N, h->N_log, h0, c0, H, Cs, stage, cols);
}
// the same in reverse: the device's H / Cs to those of h_out / c_out that are wanted
int download_states(lstm_hip_t *h, int N, int N_log, float *h_out, float *c_out, const float *H, const float *Cs, float *stage,
                    int cols) {
    const size_t n = (size_t)N * cols, nl = (size_t)N_log * cols;
    const PadMap map = pad_map_rows(1, N_log, N, cols);
    for (int k = 0; k < 2; k++) {
        float *dst = k ? c_out : h_out;
        const float *src = k ? Cs : H;
        if (!dst) continue;
        if (N_log != N) {
            pad_copy(src, stage + k * nl, map, false, h->st);
            if (int rc = untimed_status("pad_copy")) return rc;
            HIP_TRY(hipMemcpyAsync(dst, stage + k * nl, sizeof(float) * nl, hipMemcpyDeviceToHost, h->st));
        } else
            HIP_TRY(hipMemcpyAsync(dst, src, sizeof(float) * n, hipMemcpyDeviceToHost, h->st));
    }
    return 0;
}

int download_states(lstm_hip_t *h, float *h_out, float *c_out, const float *H, const float *Cs, float *stage, int cols) {
    return download_states(h, h->cfg.N, h->N_log, h_out, c_out, H, Cs, stage, cols);
}

// offsets of `streams` streams: off[0] == 0, never decreasing
int check_offsets(const char *what, const char *name, const uint64_t *off, int32_t streams) {
    if (!off) return fail(LSTM_HIP_EINVAL, "%s: null %s", what, name);
    if (off[0] != 0) return fail(LSTM_HIP_EINVAL, "%s: %s[0] must be 0 (got %llu)", what, name, (unsigned long long)off[0]);
    for (int s = 0; s < streams; s++)
        if (off[s + 1] < off[s])
            return fail(LSTM_HIP_EINVAL, "%s: %s decreases at stream %d (%llu < %llu)", what, name, s,
                        (unsigned long long)off[s + 1], (unsigned long long)off[s]);
    return 0;
}
uint64_t longest(const uint64_t *off, int32_t streams) { // the longest stream of checked offsets
    uint64_t len = 0;
    for (int s = 0; s < streams; s++) len = std::max<uint64_t>(len, off[s + 1] - off[s]);
    return len;
}

// Every stream's bytes walked through a checked byte automaton, from cstate[s] to the state after them.  A forbidden byte is
// refused (`noun`: what the caller calls a byte); qpos, where given, takes the state each byte stands in.
int walk_constraint(const char *what, const char *noun, const lstm_hip_constraint *con, int32_t streams, const uint8_t *bytes,
                    const uint64_t *off, std::vector<int32_t> &cstate, uint16_t *qpos) {
    for (int s = 0; s < streams; s++)
        for (uint64_t j = off[s]; j < off[s + 1]; j++) {
            const uint16_t v = con->next[(size_t)cstate[s] * 256 + bytes[j]];
            if (v == 0xFFFF)
                return fail(LSTM_HIP_EINVAL, "%s: stream %d: %s 0x%02x at offset %llu is forbidden in state %d", what, s, noun,
                            (unsigned)bytes[j], (unsigned long long)(j - off[s]), cstate[s]);
            if (qpos) qpos[j] = (uint16_t)cstate[s];
            cstate[s] = v;
        }
    return 0;
}

// the model an inference call reads: the five pieces of infer_block(h), resolved once per call
struct Model {
    const float *W, *U, *b, *Why, *by;
};
Model model_of(const lstm_hip_ctx *h) {
    const float *P = infer_block(h);
    return {P + h->pl.W, P + h->pl.U, P + h->pl.b, P + h->pl.Why, P + h->pl.by};
}
// one k_fwd_step over `cols` columns: the inputs xi and the state (Hf, Cf) to the state (Ht, Ct), on h's stream.  N and fast are
// the width and the LSTM_HIP_FAST_MATH flag of the model m belongs to: the handle's own, or a guide's
int step_columns(lstm_hip_t *h, const Model &m, int N, bool fast, const float4 *Ufwd, const float *Hf, const float *Cf, float *Ht,
                 float *Ct, float *G, const int32_t *xi, int cols) {
    RUN(K_FWD_STEP, fwd_step(Ufwd, m.W, m.b, Hf, Cf, Ht, Ct, G, xi, N, cols, fast, h->st));
    return 0;
}
int step_columns(lstm_hip_t *h, const Model &m, const float4 *Ufwd, const float *Hf, const float *Cf, float *Ht, float *Ct,
                 float *G, const int32_t *xi, int cols) {
    return step_columns(h, m, h->cfg.N, (h->cfg.flags & LSTM_HIP_FAST_MATH) != 0, Ufwd, Hf, Cf, Ht, Ct, G, xi, cols);
}

// a head's launcher that returned an error has launched nothing: its request for dynamic LDS was refused
int head_refused(const char *what, const char *head, hipError_t e) {
    return fail(LSTM_HIP_EHIP, "%s: the LDS request of %s was refused: %s", what, head, hipGetErrorString(e));
}

// ---- the guides of lstm_hip_generate_guided / lstm_hip_score_guided: other models fed the main
// model's inputs, each with a state of its own, their logits mixed into the head's.  Everything of a guide is only read: its
// parameter block, its widths, its flags and its stream (once, for the event the call waits on).  A guide's fragment image of
// U, its two state pairs, its gate scratch and the mixed sum are pieces of the MAIN handle's scratch, behind every other piece.
struct Guides {
    int count = 0; // 0: an unguided call -- nothing below is touched, no piece is added, nothing is launched
    float wmain = 1.0f;
    float *gsum = nullptr; // [streams][256]
    struct One {
        lstm_hip_ctx *g;
        Model m;
        int N, N_log;
        bool fast;
        float w;
        size_t n; // N * streams
        float4 *Ufwd;
        float *H, *Cs, *G, *ho, *stage;
    } r[LSTM_HIP_MAX_GUIDES];
};
// the refusals of a guidance block (include/lstm_hip.h); on success gs holds what the call reads of every guide
int check_guidance(const char *what, lstm_hip_t *h, const lstm_hip_guidance *gd, Guides &gs) {
    if (gd->size != sizeof(lstm_hip_guidance))
        return fail(LSTM_HIP_EINVAL, "%s: guidance of %u bytes, expected %zu", what, gd->size, sizeof(lstm_hip_guidance));
    if (gd->nguides < 1 || gd->nguides > LSTM_HIP_MAX_GUIDES)
        return fail(LSTM_HIP_EINVAL, "%s: nguides must be in [1, %d] (got %d)", what, LSTM_HIP_MAX_GUIDES, gd->nguides);
    if (!gd->guides) return fail(LSTM_HIP_EINVAL, "%s: guidance with null guides", what);
    if (!std::isfinite(gd->main_weight)) return fail(LSTM_HIP_EINVAL, "%s: main_weight must be finite (got %g)", what, gd->main_weight);
    for (int k = 0; k < gd->nguides; k++) {
        const lstm_hip_guide &u = gd->guides[k];
        if (!u.model) return fail(LSTM_HIP_EINVAL, "%s: guide %d: null model", what, k);
        if (!std::isfinite(u.weight)) return fail(LSTM_HIP_EINVAL, "%s: guide %d: weight must be finite (got %g)", what, k, u.weight);
        if (u.model->cfg.device != h->cfg.device)
            return fail(LSTM_HIP_EINVAL, "%s: guide %d is on device %d, the call's handle on device %d", what, k, u.model->cfg.device,
                        h->cfg.device);
        if (u.model->cfg.N > 16384) return fail(LSTM_HIP_EINVAL, "%s: guide %d: hidden width %d above 16384", what, k, u.model->cfg.N);
    }
    gs.count = gd->nguides;
    gs.wmain = (float)gd->main_weight;
    for (int k = 0; k < gs.count; k++) {
        Guides::One &r = gs.r[k];
        r.g = gd->guides[k].model;
        r.m = model_of(r.g);
        r.N = r.g->cfg.N;
        r.N_log = r.g->N_log;
        r.fast = (r.g->cfg.flags & LSTM_HIP_FAST_MATH) != 0;
        r.w = (float)gd->guides[k].weight;
    }
    return 0;
}
// the guides' pieces of the call's scratch: named last, so that every earlier offset is the unguided call's
void guide_pieces(Scratch &mem, Guides &gs, const lstm_hip_guidance *gd, int streams) {
    for (int k = 0; k < gs.count; k++) {
        Guides::One &r = gs.r[k];
        r.n = (size_t)r.N * streams;
        mem.piece(r.Ufwd, (size_t)r.N * r.N).piece(r.H, 2 * r.n).piece(r.Cs, 2 * r.n).piece(r.G, 4 * r.n);
        mem.piece(r.ho, 2 * r.n, gd->guides[k].h_out || gd->guides[k].c_out);
        mem.piece(r.stage, 2 * (size_t)r.N_log * streams, r.N_log != r.N);
    }
    mem.piece(gs.gsum, (size_t)256 * streams, gs.count > 0);
}
// ahead of the loop: the main stream waits for what the caller queued on every other guide's stream, then the guides' start
// states and fragment images; ga gets what does not change from step to step
int guides_begin(lstm_hip_t *h, Guides &gs, const lstm_hip_guidance *gd, int streams, GuideLogitsArgs &ga) {
    for (int k = 0; k < gs.count; k++) {
        Guides::One &r = gs.r[k];
        if (r.g != h) {
            hipEvent_t ev;
            HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            hipError_t e = hipEventRecord(ev, r.g->st);
            if (e == hipSuccess) e = hipStreamWaitEvent(h->st, ev, 0);
            (void)hipEventDestroy(ev); // (released once it has completed)
            HIP_TRY(e);
        }
        if (int rc = upload_states(h, r.N, r.N_log, gd->guides[k].h0, gd->guides[k].c0, r.H, r.Cs, r.stage, streams)) return rc;
        RUN(K_PACK_U, pack_U(r.m.U, r.Ufwd, nullptr, r.N, h->st));
        ga.Why[k] = r.m.Why;
        ga.by[k] = r.m.by;
        ga.h_out[k] = r.ho;
        ga.c_out[k] = r.ho ? r.ho + r.n : nullptr;
        ga.N[k] = r.N;
        ga.w[k] = r.w;
    }
    ga.gsum = gs.gsum;
    ga.nguides = gs.count;
    ga.streams = streams;
    return 0;
}
// per step, ahead of the head: the guides' weighted logit sum on their states `cur`
int guides_logits(lstm_hip_t *h, const char *what, const Guides &gs, GuideLogitsArgs &ga, int cur, long long t) {
    for (int k = 0; k < gs.count; k++) {
        ga.H[k] = gs.r[k].H + cur * gs.r[k].n;
        ga.C[k] = gs.r[k].Cs + cur * gs.r[k].n;
    }
    hipError_t refused = hipSuccess;
    RUN(K_GUIDE_LOGITS, refused = guide_logits(ga, t, h->st));
    if (refused != hipSuccess) return head_refused(what, "guide_logits", refused);
    return 0;
}
// per step, behind the main model's: every guide from its state `cur` to the other one, on the same inputs
int guides_step(lstm_hip_t *h, const Guides &gs, int cur, const int32_t *xi, int streams) {
    for (int k = 0; k < gs.count; k++) {
        const Guides::One &r = gs.r[k];
        if (int rc = step_columns(h, r.m, r.N, r.fast, r.Ufwd, r.H + cur * r.n, r.Cs + cur * r.n, r.H + (cur ^ 1) * r.n,
                                  r.Cs + (cur ^ 1) * r.n, r.G, xi, streams))
            return rc;
    }
    return 0;
}
// behind the loop: the guides' end states home
int guides_finish(lstm_hip_t *h, const Guides &gs, const lstm_hip_guidance *gd, int streams) {
    for (int k = 0; k < gs.count; k++) {
        const Guides::One &r = gs.r[k];
        if (int rc = download_states(h, r.N, r.N_log, gd->guides[k].h_out, gd->guides[k].c_out, r.ho, r.ho ? r.ho + r.n : nullptr,
                                     r.stage, streams))
            return rc;
    }
    return 0;
}

} // namespace

extern "C" {

// Batched, prompted generation and per-text scoring (include/lstm_hip.h).  All streams advance together: per step one
// gen_head launch (logits, prompt bits, the next input of every stream, final states) and one k_fwd_step over all streams,
// from the fp32 master parameters P and a fragment image of U made for this call.  Nothing of the training state is
// read or written except P; everything else lives in one scratch allocation kept on the handle (gen_scratch).
// Sampling controls: a filter, a stop byte or a request for `kept` selects gen_head's FILTER
// instantiation (a.end set); without them the launches are those of lstm_hip_generate before the controls existed.
// Constraint: a byte automaton selects gen_head's CONSTRAIN instantiation (a.ctab set).  The table is
// validated and every stream's state walked over its prompt here, on the host, before anything is launched; the table, the
// allowed counts and the states then live in the same scratch allocation.  Without one the call is lstm_hip_generate_ex's.
int lstm_hip_generate(lstm_hip_t *h, int32_t streams, const uint8_t *prompts, const uint64_t *prompt_off, const float *h0,
                      const float *c0, double temperature, const double *u, int32_t count, uint8_t *out, double *bits,
                      float *h_out, float *c_out) {
    const lstm_hip_sampling opt{(uint32_t)sizeof(lstm_hip_sampling), temperature, 0, 1.0, -1};
    return lstm_hip_generate_ex(h, streams, prompts, prompt_off, h0, c0, &opt, u, count, out, bits, h_out, c_out, nullptr, nullptr);
}

int lstm_hip_generate_ex(lstm_hip_t *h, int32_t streams, const uint8_t *prompts, const uint64_t *prompt_off, const float *h0,
                         const float *c0, const lstm_hip_sampling *opt, const double *u, int32_t count, uint8_t *out,
                         double *bits, float *h_out, float *c_out, int32_t *out_len, uint16_t *kept) {
    return lstm_hip_generate_constrained(h, streams, prompts, prompt_off, h0, c0, opt, u, count, out, bits, h_out, c_out, out_len,
                                         kept, nullptr, nullptr, nullptr);
}

// the well-formed-UTF-8 automaton (include/lstm_hip.h): state 0 is the character boundary, 1..2 await one / two more
// continuation bytes, 3..4 follow E0 / ED, 5 awaits three, 6..7 follow F0 / F4
int32_t lstm_hip_dfa_utf8(uint16_t *next) {
    if (!next) return 8;
    std::fill(next, next + 8 * 256, (uint16_t)0xFFFF);
    auto range = [&](int q, int lo, int hi, int to) {
        for (int b = lo; b <= hi; b++) next[q * 256 + b] = (uint16_t)to;
    };
    range(0, 0x00, 0x7F, 0);
    range(0, 0xC2, 0xDF, 1);
    range(0, 0xE0, 0xE0, 3);
    range(0, 0xE1, 0xEC, 2);
    range(0, 0xED, 0xED, 4);
    range(0, 0xEE, 0xEF, 2);
    range(0, 0xF0, 0xF0, 6);
    range(0, 0xF1, 0xF3, 5);
    range(0, 0xF4, 0xF4, 7);
    range(1, 0x80, 0xBF, 0);
    range(2, 0x80, 0xBF, 1);
    range(3, 0xA0, 0xBF, 1);
    range(4, 0x80, 0x9F, 1);
    range(5, 0x80, 0xBF, 2);
    range(6, 0x90, 0xBF, 2);
    range(7, 0x80, 0x8F, 2);
    return 8;
}

int lstm_hip_dfa_restrict(uint16_t *next, int32_t states, const uint8_t allow[256]) {
    if (!next || !allow) return fail(LSTM_HIP_EINVAL, "dfa_restrict: null table or allow list");
    if (states < 1 || states > 4096) return fail(LSTM_HIP_EINVAL, "dfa_restrict: states must be in [1, 4096] (got %d)", states);
    for (size_t e = 0; e < (size_t)states * 256; e++)
        if (next[e] != 0xFFFF && next[e] >= states)
            return fail(LSTM_HIP_EINVAL, "dfa_restrict: entry next[%zu][%zu] = %u is neither a state below %d nor 0xFFFF", e / 256,
                        e % 256, (unsigned)next[e], states);
    for (int q = 0; q < states; q++)
        for (int b = 0; b < 256; b++)
            if (!allow[b]) next[(size_t)q * 256 + b] = 0xFFFF;
    std::vector<char> empty(states);
    for (bool changed = true; changed;) { // forbid what leads into a state with no allowed byte, until nothing changes
        changed = false;
        for (int q = 0; q < states; q++) {
            const uint16_t *row = next + (size_t)q * 256;
            empty[q] = std::all_of(row, row + 256, [](uint16_t v) { return v == 0xFFFF; });
        }
        for (size_t e = 0; e < (size_t)states * 256; e++)
            if (next[e] != 0xFFFF && empty[next[e]]) {
                next[e] = 0xFFFF;
                changed = true;
            }
    }
    if (empty[0]) return fail(LSTM_HIP_EINVAL, "dfa_restrict: state 0 has no allowed byte left");
    return 0;
}

// The deadline rows of a checked byte automaton with accepting states (include/lstm_hip.h, lstm_hip_beam_search_constrained):
// frows[R * fwords + q / 32] bit q % 32 is F[R][q] for R = 0 .. count.  F[0][q] = acc(q); F[R][q] = some allowed byte b of q:
// acc(next) if b is the stop byte, else F[R - 1][next].  Every stream must start (cstate: the state after its prompt) where
// F[count] holds.  Shared by beam search and the accepting sampler.
static int deadline_rows(const char *what, const lstm_hip_constraint *con, const uint8_t *accept, int stop_byte, int32_t count,
                         const std::vector<int32_t> &cstate, std::vector<uint32_t> &frows) {
    const int Q = con->states, fwords = (Q + 31) / 32;
    if (((long long)count + 1) * Q > (1ll << 28))
        return fail(LSTM_HIP_EINVAL, "%s: (count + 1) x states = %lld above 2^28 with accepting states", what, ((long long)count + 1) * Q);
    std::vector<std::vector<uint16_t>> succ(Q); // the distinct states q's allowed bytes other than the stop byte lead to
    std::vector<char> stops(Q, 0);              // q's stop byte is allowed and leads into an accepting state
    for (int q = 0; q < Q; q++) {
        for (int b = 0; b < 256; b++) {
            const uint16_t v = con->next[(size_t)q * 256 + b];
            if (v == 0xFFFF) continue;
            if (b == stop_byte) stops[q] = accept[v] != 0;
            else succ[q].push_back(v);
        }
        std::sort(succ[q].begin(), succ[q].end());
        succ[q].erase(std::unique(succ[q].begin(), succ[q].end()), succ[q].end());
    }
    frows.assign((size_t)(count + 1) * fwords, 0u);
    auto bit = [&](int R, int q) { return (frows[(size_t)R * fwords + (q >> 5)] >> (q & 31)) & 1u; };
    for (int q = 0; q < Q; q++)
        if (accept[q]) frows[q >> 5] |= 1u << (q & 31);
    // a row is a function of the row before it: once two rows in sequence are equal every later one is, and is copied
    bool settled = false;
    for (int R = 1; R <= count; R++) {
        uint32_t *row = frows.data() + (size_t)R * fwords;
        if (settled) {
            std::copy(row - fwords, row, row);
            continue;
        }
        for (int q = 0; q < Q; q++) {
            bool f = stops[q];
            for (size_t i = 0; !f && i < succ[q].size(); i++) f = bit(R - 1, succ[q][i]);
            if (f) row[q >> 5] |= 1u << (q & 31);
        }
        settled = std::equal(row, row + fwords, row - fwords);
    }
    for (size_t s = 0; s < cstate.size(); s++)
        if (!bit(count, cstate[s]))
            return fail(LSTM_HIP_EINVAL, "%s: stream %d: no accepted string of %d bytes or fewer ending in the stop byte "
                        "from state %d", what, (int)s, count, cstate[s]);
    return 0;
}

// the table checks of a byte automaton (include/lstm_hip.h, lstm_hip_generate_constrained): on success ccount holds the allowed
// bytes of every state and cstate every stream's start state
static int check_constraint(const char *what, const lstm_hip_constraint *con, int32_t streams, const int32_t *start_state,
                            std::vector<int32_t> &cstate, std::vector<uint16_t> &ccount) {
    const int Q = con->states;
    if (con->size != sizeof(lstm_hip_constraint))
        return fail(LSTM_HIP_EINVAL, "%s: constraint of %u bytes, expected %zu", what, con->size, sizeof(lstm_hip_constraint));
    if (Q < 1 || Q > 4096) return fail(LSTM_HIP_EINVAL, "%s: constraint states must be in [1, 4096] (got %d)", what, Q);
    if (!con->next) return fail(LSTM_HIP_EINVAL, "%s: constraint with a null table", what);
    ccount.assign(Q, 0);
    for (int q = 0; q < Q; q++)
        for (int b = 0; b < 256; b++) {
            const uint16_t v = con->next[(size_t)q * 256 + b];
            if (v != 0xFFFF && v >= Q)
                return fail(LSTM_HIP_EINVAL, "%s: constraint entry next[%d][%d] = %u is neither a state below %d nor 0xFFFF", what,
                            q, b, (unsigned)v, Q);
            ccount[q] += v != 0xFFFF;
        }
    cstate.assign(streams, 0);
    std::vector<char> seen(Q, 0);
    std::vector<int32_t> queue; // breadth-first from the start states
    for (int s = 0; s < streams; s++) {
        if (start_state) cstate[s] = start_state[s];
        if (cstate[s] < 0 || cstate[s] >= Q)
            return fail(LSTM_HIP_EINVAL, "%s: start_state[%d] = %d is outside [0, %d)", what, s, cstate[s], Q);
        if (!seen[cstate[s]]) {
            seen[cstate[s]] = 1;
            queue.push_back(cstate[s]);
        }
    }
    for (size_t i = 0; i < queue.size(); i++) {
        const int q = queue[i];
        if (ccount[q] == 0)
            return fail(LSTM_HIP_EINVAL, "%s: constraint state %d can be reached and has no allowed byte", what, q);
        for (int b = 0; b < 256; b++) {
            const uint16_t v = con->next[(size_t)q * 256 + b];
            if (v != 0xFFFF && !seen[v]) {
                seen[v] = 1;
                queue.push_back(v);
            }
        }
    }
    return 0;
}

// the regex compiler and the product of two tables (dfa_regex.cpp; neither needs a device or a handle)
int32_t lstm_hip_dfa_regex(const uint8_t *pattern, size_t len, int32_t stop_byte, uint16_t *next, uint8_t *accept, int32_t cap,
                           int32_t *error_pos) {
    std::string msg;
    const int32_t q = dfa::regex(pattern, len, stop_byte, next, accept, cap, error_pos, msg);
    return q < 0 ? fail(LSTM_HIP_EINVAL, "%s", msg.c_str()) : q;
}

int32_t lstm_hip_dfa_intersect(const uint16_t *a, int32_t qa, const uint8_t *acc_a, const uint16_t *b, int32_t qb,
                               const uint8_t *acc_b, uint16_t *next, uint8_t *accept, int32_t cap) {
    std::string msg;
    const int32_t q = dfa::intersect(a, qa, acc_a, b, qb, acc_b, next, accept, cap, msg);
    return q < 0 ? fail(LSTM_HIP_EINVAL, "%s", msg.c_str()) : q;
}

int lstm_hip_generate_constrained(lstm_hip_t *h, int32_t streams, const uint8_t *prompts, const uint64_t *prompt_off,
                                  const float *h0, const float *c0, const lstm_hip_sampling *opt, const double *u, int32_t count,
                                  uint8_t *out, double *bits, float *h_out, float *c_out, int32_t *out_len, uint16_t *kept,
                                  const lstm_hip_constraint *con, const int32_t *start_state, int32_t *end_state) {
    const lstm_hip_beam_constraint bc{(uint32_t)sizeof(lstm_hip_beam_constraint), con, nullptr};
    return lstm_hip_generate_accepting(h, streams, prompts, prompt_off, h0, c0, opt, u, count, out, bits, h_out, c_out, out_len,
                                       kept, con ? &bc : nullptr, start_state, end_state);
}

// Accepting states: with bc->accept the deadline rows F are made on the host as beam search makes them,
// and gen_head's DEADLINE instantiation (a.frows set) masks what the rows rule out.  The accept bytes and the rows are the last
// pieces of the scratch layout: without them every offset, upload and launch is lstm_hip_generate_constrained's.
int lstm_hip_generate_accepting(lstm_hip_t *h, int32_t streams, const uint8_t *prompts, const uint64_t *prompt_off,
                                const float *h0, const float *c0, const lstm_hip_sampling *opt, const double *u, int32_t count,
                                uint8_t *out, double *bits, float *h_out, float *c_out, int32_t *out_len, uint16_t *kept,
                                const lstm_hip_beam_constraint *bc, const int32_t *start_state, int32_t *end_state) {
    return lstm_hip_generate_processed(h, streams, prompts, prompt_off, h0, c0, opt, u, count, out, bits, h_out, c_out, out_len, kept,
                                       bc, start_state, end_state, nullptr);
}

// Logit processors: a bias, min-p or the n-gram rule selects gen_head's PROCESS instantiation
// (a.process set).  The block is checked here before anything is launched; the bias and each stream's history ++ prompt (the
// text the n-gram rule scans, with the drawn bytes behind it) are the last pieces of the scratch layout: with lp NULL or
// everything off every offset, upload and launch is lstm_hip_generate_accepting's.  (The body is lstm_hip_generate_guided's,
// below: this function is its caller with gd = NULL.)
int lstm_hip_generate_processed(lstm_hip_t *h, int32_t streams, const uint8_t *prompts, const uint64_t *prompt_off,
                                const float *h0, const float *c0, const lstm_hip_sampling *opt, const double *u, int32_t count,
                                uint8_t *out, double *bits, float *h_out, float *c_out, int32_t *out_len, uint16_t *kept,
                                const lstm_hip_beam_constraint *bc, const int32_t *start_state, int32_t *end_state,
                                const lstm_hip_logit_processors *lp) {
    return lstm_hip_generate_guided(h, streams, prompts, prompt_off, h0, c0, opt, u, count, out, bits, h_out, c_out, out_len, kept, bc,
                                    start_state, end_state, lp, nullptr);
}

// Guides: other models, fed the same bytes from states of their own, whose logits are mixed into the
// main model's ahead of the processors.  Per step one guide_logits launch ahead of the head (all guides: their weighted logit
// sum, and their end states where a stream has had its last input) and one k_fwd_step per guide behind the main model's; the
// head's PROCESS instantiation (a.gsum set) mixes.  The block is checked here before anything is launched; the guides' images,
// states and the sum are the last pieces of the scratch layout: with gd NULL every offset, upload and launch is
// lstm_hip_generate_processed's.
int lstm_hip_generate_guided(lstm_hip_t *h, int32_t streams, const uint8_t *prompts, const uint64_t *prompt_off, const float *h0,
                             const float *c0, const lstm_hip_sampling *opt, const double *u, int32_t count, uint8_t *out,
                             double *bits, float *h_out, float *c_out, int32_t *out_len, uint16_t *kept,
                             const lstm_hip_beam_constraint *bc, const int32_t *start_state, int32_t *end_state,
                             const lstm_hip_logit_processors *lp, const lstm_hip_guidance *gd) {
    CHECK(h);
    if (!opt) return fail(LSTM_HIP_EINVAL, "generate: null sampling options");
    if (opt->size != sizeof(lstm_hip_sampling))
        return fail(LSTM_HIP_EINVAL, "generate: sampling options of %u bytes, expected %zu", opt->size, sizeof(lstm_hip_sampling));
    const double temperature = opt->temperature;
    if (opt->top_k < 0 || opt->top_k > 256) return fail(LSTM_HIP_EINVAL, "generate: top_k must be in [0, 256] (got %d)", opt->top_k);
    if (!(opt->top_p > 0.0 && opt->top_p <= 1.0)) return fail(LSTM_HIP_EINVAL, "generate: top_p must be in (0, 1] (got %g)", opt->top_p);
    if (opt->stop_byte < -1 || opt->stop_byte > 255)
        return fail(LSTM_HIP_EINVAL, "generate: stop_byte must be -1 or in [0, 255] (got %d)", opt->stop_byte);
    if (streams < 1 || streams > 4096) return fail(LSTM_HIP_EINVAL, "generate: streams must be in [1, 4096] (got %d)", streams);
    if (count < 0) return fail(LSTM_HIP_EINVAL, "generate: count < 0 (%d)", count);
    if (!std::isfinite(temperature) || temperature < 0.0)
        return fail(LSTM_HIP_EINVAL, "generate: temperature must be finite and >= 0 (got %g)", temperature);
    if (count > 0 && temperature > 0.0 && !u) return fail(LSTM_HIP_EINVAL, "generate: draws u are needed unless temperature is 0");
    if (count > 0 && !out) return fail(LSTM_HIP_EINVAL, "generate: null out with count > 0");
    if (prompts && !prompt_off) return fail(LSTM_HIP_EINVAL, "generate: prompts without prompt_off");
    if (prompt_off) {
        if (int rc = check_offsets("generate", "prompt_off", prompt_off, streams)) return rc;
        if (prompt_off[streams] > 0 && !prompts) return fail(LSTM_HIP_EINVAL, "generate: prompt_off without prompts");
    }
    const uint64_t max_len = prompt_off ? longest(prompt_off, streams) : 0;
    const int N = h->cfg.N;
    if (N > 16384) return fail(LSTM_HIP_EINVAL, "generate: hidden width %d above 16384", N);
    // the logit processors: the block is checked, then each stream's history ++ prompt is laid out for the n-gram scan
    std::vector<uint8_t> ptext;
    std::vector<uint64_t> ptoff;
    if (lp) {
        if (lp->size != sizeof(lstm_hip_logit_processors))
            return fail(LSTM_HIP_EINVAL, "generate: logit processors of %u bytes, expected %zu", lp->size, sizeof(lstm_hip_logit_processors));
        if (lp->bias)
            for (int b = 0; b < 256; b++)
                if (!std::isfinite(lp->bias[b]))
                    return fail(LSTM_HIP_EINVAL, "generate: bias[%d] = %g is not finite (to ban a byte, restrict a table with "
                                "lstm_hip_dfa_restrict)", b, (double)lp->bias[b]);
        if (!(lp->min_p >= 0.0 && lp->min_p <= 1.0)) return fail(LSTM_HIP_EINVAL, "generate: min_p must be in [0, 1] (got %g)", lp->min_p);
        if (lp->no_repeat < 0 || lp->no_repeat > 64)
            return fail(LSTM_HIP_EINVAL, "generate: no_repeat must be in [0, 64] (got %d)", lp->no_repeat);
        if (lp->history && !lp->history_off) return fail(LSTM_HIP_EINVAL, "generate: history without history_off");
        if (lp->history_off && !lp->history) return fail(LSTM_HIP_EINVAL, "generate: history_off without history");
        if (lp->history_off)
            if (int rc = check_offsets("generate", "history_off", lp->history_off, streams)) return rc;
        if (lp->history && lp->no_repeat == 0) return fail(LSTM_HIP_EINVAL, "generate: history given with no_repeat 0: nothing reads it");
        if (lp->no_repeat > 0) {
            ptoff.assign((size_t)streams + 1, 0);
            uint64_t most = 0;
            for (int s = 0; s < streams; s++) {
                const uint64_t hl = lp->history_off ? lp->history_off[s + 1] - lp->history_off[s] : 0;
                const uint64_t pl = prompt_off ? prompt_off[s + 1] - prompt_off[s] : 0;
                ptoff[s + 1] = ptoff[s] + hl + pl;
                most = std::max(most, hl + pl);
            }
            if (most + (uint64_t)count > 65536)
                return fail(LSTM_HIP_EINVAL, "generate: no_repeat over a text of %llu bytes (the longest history + prompt, + count), "
                            "above 65536: the scan is linear in the text at every draw", (unsigned long long)(most + (uint64_t)count));
            ptext.resize(ptoff[streams]);
            for (int s = 0; s < streams; s++) {
                uint8_t *to = ptext.data() + ptoff[s];
                if (lp->history_off) to = std::copy(lp->history + lp->history_off[s], lp->history + lp->history_off[s + 1], to);
                if (prompt_off) std::copy(prompts + prompt_off[s], prompts + prompt_off[s + 1], to);
            }
        }
    }
    const bool lp_bias = lp && lp->bias, lp_min_p = lp && lp->min_p > 0.0, lp_ngram = lp && lp->no_repeat > 0;
    const bool processors = lp_bias || lp_min_p || lp_ngram; // gen_head's PROCESS instantiation (as guides: `process` below)
    // the constraint: the table is checked, then every stream's state walks its prompt
    std::vector<int32_t> cstate; // [streams] the state after each prompt
    std::vector<uint16_t> ccount; // [states] allowed bytes
    std::vector<uint32_t> frows;  // [count + 1][fwords] bit q of row R: F[R][q]
    if (!bc && (start_state || end_state)) return fail(LSTM_HIP_EINVAL, "generate: start_state / end_state given without a constraint");
    if (bc && bc->size != sizeof(lstm_hip_beam_constraint))
        return fail(LSTM_HIP_EINVAL, "generate: beam constraint of %u bytes, expected %zu", bc->size, sizeof(lstm_hip_beam_constraint));
    if (bc && !bc->con) return fail(LSTM_HIP_EINVAL, "generate: beam constraint with a null constraint");
    const lstm_hip_constraint *con = bc ? bc->con : nullptr;
    const uint8_t *accept = bc ? bc->accept : nullptr;
    const int Q = con ? con->states : 0, fwords = (Q + 31) / 32;
    if (con) {
        if (int rc = check_constraint("generate", con, streams, start_state, cstate, ccount)) return rc;
        if (prompt_off)
            if (int rc = walk_constraint("generate", "prompt byte", con, streams, prompts, prompt_off, cstate, nullptr)) return rc;
    }
    if (accept) // (with count 0 this asks that every stream stands in an accepting state)
        if (int rc = deadline_rows("generate", con, accept, opt->stop_byte, count, cstate, frows)) return rc;
    Guides gs; // (a guided draw is a processed draw)
    if (gd)
        if (int rc = check_guidance("generate", h, gd, gs)) return rc;
    const bool process = processors || gs.count > 0;
    const uint64_t total = prompt_off ? prompt_off[streams] : 0;
    const size_t n = (size_t)N * streams, nl = (size_t)h->N_log * streams, nd = (size_t)count * streams;
    const bool keep = h_out || c_out;
    const bool top_k_on = opt->top_k >= 1 && opt->top_k <= 255, nucleus = opt->top_p < 1.0;
    const bool controls = top_k_on || nucleus || opt->stop_byte >= 0 || kept || con || process; // gen_head's FILTER instantiation

    float4 *Ufwd;
    float *H, *Cs, *G, *ho, *stage, *d_bias;
    int32_t *xi, *d_end, *d_q;
    uint64_t *d_off, *d_ptoff;
    uint8_t *d_prompts, *d_out, *d_acc, *d_ptext;
    uint32_t *d_F;
    double *d_u, *d_bits;
    uint16_t *d_kept, *d_tab, *d_cnt;
    Scratch mem;
    mem.piece(Ufwd, (size_t)N * N).piece(H, 2 * n).piece(Cs, 2 * n).piece(G, 4 * n).piece(ho, 2 * n, keep);
    mem.piece(stage, 2 * nl, h->padded()).piece(xi, streams);
    mem.piece(d_off, streams + 1, prompt_off != nullptr).piece(d_prompts, total, total != 0);
    mem.piece(d_u, nd, count > 0 && temperature >= (double)FLT_MIN).piece(d_out, nd).piece(d_bits, streams);
    mem.piece(d_end, streams, controls).piece(d_kept, nd, kept != nullptr);
    mem.piece(d_tab, 256 * (size_t)Q, con != nullptr).piece(d_cnt, Q, con != nullptr).piece(d_q, streams, con != nullptr);
    mem.piece(d_acc, Q, accept != nullptr).piece(d_F, (size_t)count * fwords, accept != nullptr);
    mem.piece(d_bias, 256, lp_bias).piece(d_ptoff, (size_t)streams + 1, lp_ngram).piece(d_ptext, ptext.size(), !ptext.empty());
    guide_pieces(mem, gs, gd, streams);
    if (int rc = mem.commit(h)) return rc;

    // start state (padding rows zero), inputs
    if (int rc = upload_states(h, h0, c0, H, Cs, stage, streams)) return rc;
    if (d_off) HIP_TRY(hipMemcpyAsync(d_off, prompt_off, sizeof(uint64_t) * (streams + 1), hipMemcpyHostToDevice, h->st));
    if (d_prompts) HIP_TRY(hipMemcpyAsync(d_prompts, prompts, total, hipMemcpyHostToDevice, h->st));
    if (d_u) HIP_TRY(hipMemcpyAsync(d_u, u, sizeof(double) * nd, hipMemcpyHostToDevice, h->st));
    HIP_TRY(hipMemsetAsync(d_bits, 0, sizeof(double) * streams, h->st));
    if (d_end) HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_end), count, streams, h->st));
    if (d_kept && nd) HIP_TRY(hipMemsetAsync(d_kept, 0, sizeof(uint16_t) * nd, h->st)); // 0 wherever a stream has stopped
    if (opt->stop_byte >= 0 && nd) HIP_TRY(hipMemsetAsync(d_out, 0, nd, h->st));
    if (con) {
        HIP_TRY(hipMemcpyAsync(d_tab, con->next, sizeof(uint16_t) * 256 * (size_t)Q, hipMemcpyHostToDevice, h->st));
        HIP_TRY(hipMemcpyAsync(d_cnt, ccount.data(), sizeof(uint16_t) * Q, hipMemcpyHostToDevice, h->st));
        HIP_TRY(hipMemcpyAsync(d_q, cstate.data(), sizeof(int32_t) * streams, hipMemcpyHostToDevice, h->st));
    }
    if (accept) { // rows 0 .. count - 1: draw i reads row count - 1 - i
        HIP_TRY(hipMemcpyAsync(d_acc, accept, (size_t)Q, hipMemcpyHostToDevice, h->st));
        if (count > 0) HIP_TRY(hipMemcpyAsync(d_F, frows.data(), sizeof(uint32_t) * (size_t)count * fwords, hipMemcpyHostToDevice, h->st));
    }
    if (lp_bias) HIP_TRY(hipMemcpyAsync(d_bias, lp->bias, sizeof(float) * 256, hipMemcpyHostToDevice, h->st));
    if (lp_ngram) {
        HIP_TRY(hipMemcpyAsync(d_ptoff, ptoff.data(), sizeof(uint64_t) * ((size_t)streams + 1), hipMemcpyHostToDevice, h->st));
        if (d_ptext) HIP_TRY(hipMemcpyAsync(d_ptext, ptext.data(), ptext.size(), hipMemcpyHostToDevice, h->st));
    }
    const Model m = model_of(h);
    RUN(K_PACK_U, pack_U(m.U, Ufwd, nullptr, N, h->st));
    GuideLogitsArgs ga{};
    if (int rc = guides_begin(h, gs, gd, streams, ga)) return rc;
    ga.off = d_off;
    ga.end = d_end;
    ga.count = count;

    GenHeadArgs a{};
    a.Why = m.Why;
    a.by = m.by;
    a.prompts = d_prompts;
    a.off = d_off;
    a.u = d_u;
    a.out = d_out;
    a.bits = bits ? d_bits : nullptr;
    a.x_next = xi;
    a.h_out = ho;
    a.c_out = ho ? ho + n : nullptr;
    a.N = N;
    a.streams = streams;
    a.count = count;
    // a temperature below the smallest normal float is the greedy limit (in float it would be 0 or denormal: (z - max z) / tau
    // would give 0 / 0 at the maximum)
    a.mode = temperature < (double)FLT_MIN ? 2 : temperature == 1.0 ? 0 : 1;
    a.tau = (float)temperature;
    a.keep_k = top_k_on ? opt->top_k : 256;
    a.nucleus = nucleus;
    a.top_p = (float)opt->top_p;
    a.filter = top_k_on || nucleus;
    a.stop_byte = opt->stop_byte;
    a.end = d_end;
    a.kept = d_kept;
    a.ctab = d_tab;
    a.ccount = d_cnt;
    a.cstate = d_q;
    a.accept = d_acc;
    a.frows = d_F;
    a.fwords = fwords;
    a.process = process;
    a.bias = d_bias;
    a.min_p = lp ? (float)lp->min_p : 0.0f;
    a.no_repeat = lp ? lp->no_repeat : 0;
    a.ptext = d_ptext;
    a.ptoff = d_ptoff;
    a.gsum = gs.gsum;
    a.wmain = gs.wmain;
    const bool stable = (h->cfg.flags & LSTM_HIP_STABLE_SOFTMAX) != 0;
    const long long steps = (long long)max_len + count; // inputs of the longest stream
    int cur = 0;
    for (long long t = 0;; t++) {
        a.H = H + cur * n;
        a.C = Cs + cur * n;
        if (gs.count)
            if (int rc = guides_logits(h, "generate", gs, ga, cur, t)) return rc;
        hipError_t refused = hipSuccess; // (only the FILTER instantiations ever report one)
        RUN(K_GEN_HEAD, refused = gen_head(a, t, stable, h->st));
        if (refused != hipSuccess) return head_refused("generate", "gen_head", refused);
        if (t == steps) break;
        if (int rc = step_columns(h, m, Ufwd, a.H, a.C, H + (cur ^ 1) * n, Cs + (cur ^ 1) * n, G, xi, streams)) return rc;
        if (int rc = guides_step(h, gs, cur, xi, streams)) return rc;
        cur ^= 1;
    }

    if (count > 0) HIP_TRY(hipMemcpyAsync(out, d_out, nd, hipMemcpyDeviceToHost, h->st));
    if (bits) HIP_TRY(hipMemcpyAsync(bits, d_bits, sizeof(double) * streams, hipMemcpyDeviceToHost, h->st));
    if (out_len) {
        if (d_end) HIP_TRY(hipMemcpyAsync(out_len, d_end, sizeof(int32_t) * streams, hipMemcpyDeviceToHost, h->st));
        else std::fill(out_len, out_len + streams, count);
    }
    if (kept && nd) HIP_TRY(hipMemcpyAsync(kept, d_kept, sizeof(uint16_t) * nd, hipMemcpyDeviceToHost, h->st));
    if (end_state) HIP_TRY(hipMemcpyAsync(end_state, d_q, sizeof(int32_t) * streams, hipMemcpyDeviceToHost, h->st));
    if (int rc = download_states(h, h_out, c_out, a.h_out, a.c_out, stage, streams)) return rc;
    if (int rc = guides_finish(h, gs, gd, streams)) return rc;
    HIP_TRY(hipStreamSynchronize(h->st));
    return 0;
}

// ---- arithmetic coding of bytes with the model (include/lstm_hip.h)
uint32_t lstm_hip_coder_version(void) { return 1; }

size_t lstm_hip_code_bound(uint64_t len) {
    if (len == 0) return 0;
    if (len > (SIZE_MAX - 4) / 3) return SIZE_MAX;
    return (size_t)(3 * len + 4);
}

// Beam search (include/lstm_hip.h): the generator's loop over streams * beams columns.  Per step one
// beam_head launch (selection, tables, the states gathered by parent into the second pair of buffers) and one k_fwd_step
// from that pair back into the first; after the loop one beam_backtrack launch.  No readback inside the loop.
// Constraint: a byte automaton selects beam_head's CONSTRAIN instantiation (a.ctab set).  As in
// lstm_hip_generate_constrained the table is validated and every stream's state walked over its prompt on the host before
// anything is launched; with accepting states the reachability rows F[R][q] are made here too, one bit per (R, q).  The
// table, the slots' states, the accept bytes and the rows are the last pieces of the scratch layout, so that without a
// constraint every offset, upload and launch is that of the call before constraints existed.
int lstm_hip_beam_search(lstm_hip_t *h, int32_t streams, const uint8_t *prompts, const uint64_t *prompt_off, const float *h0,
                         const float *c0, const lstm_hip_beam *opt, int32_t count, uint8_t *out, int32_t *out_len, double *bits,
                         uint8_t *trace_parent, uint8_t *trace_byte) {
    return lstm_hip_beam_search_constrained(h, streams, prompts, prompt_off, h0, c0, opt, count, out, out_len, bits, trace_parent,
                                            trace_byte, nullptr, nullptr, nullptr);
}

int lstm_hip_beam_search_constrained(lstm_hip_t *h, int32_t streams, const uint8_t *prompts, const uint64_t *prompt_off,
                                     const float *h0, const float *c0, const lstm_hip_beam *opt, int32_t count, uint8_t *out,
                                     int32_t *out_len, double *bits, uint8_t *trace_parent, uint8_t *trace_byte,
                                     const lstm_hip_beam_constraint *bc, const int32_t *start_state, int32_t *end_state) {
    CHECK(h);
    if (!opt) return fail(LSTM_HIP_EINVAL, "beam_search: null options");
    if (opt->size != sizeof(lstm_hip_beam))
        return fail(LSTM_HIP_EINVAL, "beam_search: options of %u bytes, expected %zu", opt->size, sizeof(lstm_hip_beam));
    const int W = opt->beams;
    if (W < 1 || W > 32) return fail(LSTM_HIP_EINVAL, "beam_search: beams must be in [1, 32] (got %d)", W);
    if (opt->stop_byte < -1 || opt->stop_byte > 255)
        return fail(LSTM_HIP_EINVAL, "beam_search: stop_byte must be -1 or in [0, 255] (got %d)", opt->stop_byte);
    if (streams < 1 || (long long)streams * W > 4096)
        return fail(LSTM_HIP_EINVAL, "beam_search: streams must be >= 1 and streams * beams <= 4096 (got %d x %d)", streams, W);
    if (count < 0) return fail(LSTM_HIP_EINVAL, "beam_search: count < 0 (%d)", count);
    if (count > 0 && (!out || !out_len || !bits)) return fail(LSTM_HIP_EINVAL, "beam_search: null out, out_len or bits with count > 0");
    if (prompts && !prompt_off) return fail(LSTM_HIP_EINVAL, "beam_search: prompts without prompt_off");
    if (prompt_off) {
        if (int rc = check_offsets("beam_search", "prompt_off", prompt_off, streams)) return rc;
        if (prompt_off[streams] > 0 && !prompts) return fail(LSTM_HIP_EINVAL, "beam_search: prompt_off without prompts");
    }
    const uint64_t max_len = prompt_off ? longest(prompt_off, streams) : 0;
    const int N = h->cfg.N, Nl = h->N_log, cols = streams * W;
    if ((long long)N * W > 16384)
        return fail(LSTM_HIP_EINVAL, "beam_search: hidden width %d x %d beams above 16384 floats of LDS", N, W);
    // the constraint: the table is checked, every stream's state walks its prompt, then the deadline rows
    if (!bc && (start_state || end_state)) return fail(LSTM_HIP_EINVAL, "beam_search: start_state / end_state given without a constraint");
    if (bc && bc->size != sizeof(lstm_hip_beam_constraint))
        return fail(LSTM_HIP_EINVAL, "beam_search: beam constraint of %u bytes, expected %zu", bc->size, sizeof(lstm_hip_beam_constraint));
    if (bc && !bc->con) return fail(LSTM_HIP_EINVAL, "beam_search: beam constraint with a null constraint");
    const lstm_hip_constraint *con = bc ? bc->con : nullptr;
    const uint8_t *accept = bc ? bc->accept : nullptr;
    std::vector<int32_t> cstate;  // [streams] the state after each prompt (q0)
    std::vector<uint16_t> ccount; // (the allowed counts are checked, not used)
    std::vector<uint32_t> frows;  // [count + 1][fwords] bit q of row R: F[R][q]
    const int Q = con ? con->states : 0, fwords = (Q + 31) / 32;
    if (con) {
        if (int rc = check_constraint("beam_search", con, streams, start_state, cstate, ccount)) return rc;
        if (prompt_off)
            if (int rc = walk_constraint("beam_search", "prompt byte", con, streams, prompts, prompt_off, cstate, nullptr)) return rc;
    }
    if (accept)
        if (int rc = deadline_rows("beam_search", con, accept, opt->stop_byte, count, cstate, frows)) return rc;
    if (count == 0) { // nothing is selected: every slot is as it starts
        for (int c = 0; c < cols; c++) {
            if (out_len) out_len[c] = 0;
            if (bits) bits[c] = c % W == 0 ? 0.0 : (double)INFINITY;
            if (end_state) end_state[c] = cstate[c / W];
        }
        return 0;
    }
    const uint64_t total = prompt_off ? prompt_off[streams] : 0;
    const size_t n = (size_t)N * cols, nl = (size_t)Nl * cols, nd = (size_t)count * cols;

    float4 *Ufwd;
    float *H, *Cs, *G, *stage;
    int32_t *xi, *d_len, *d_fin, *d_q;
    uint64_t *d_off;
    uint8_t *d_prompts, *d_tp, *d_tb, *d_out, *d_acc;
    double *d_cost;
    uint16_t *d_tab;
    uint32_t *d_F;
    Scratch mem;
    mem.piece(Ufwd, (size_t)N * N).piece(H, 2 * n).piece(Cs, 2 * n).piece(G, 4 * n);
    mem.piece(stage, 2 * nl, h->padded()).piece(xi, cols);
    mem.piece(d_off, streams + 1, prompt_off != nullptr).piece(d_prompts, total, total != 0);
    mem.piece(d_tp, nd).piece(d_tb, nd).piece(d_out, nd).piece(d_cost, cols).piece(d_len, cols).piece(d_fin, cols);
    mem.piece(d_tab, 256 * (size_t)Q, con != nullptr).piece(d_q, cols, con != nullptr);
    mem.piece(d_acc, Q, accept != nullptr).piece(d_F, (size_t)count * fwords, accept != nullptr);
    if (int rc = mem.commit(h)) return rc;

    // start state: every slot of a stream starts from the stream's column (padding rows zero)
    std::vector<float> rep[2]; // (h0 / c0 with each column W times: alive until the synchronize behind the upload)
    for (int k = 0; k < 2; k++) {
        const float *src = k ? c0 : h0;
        if (!src) continue;
        rep[k].resize(nl);
        for (int c = 0; c < cols; c++) std::copy(src + (size_t)(c / W) * Nl, src + (size_t)(c / W + 1) * Nl, rep[k].begin() + (size_t)c * Nl);
    }
    if (int rc = upload_states(h, h0 ? rep[0].data() : nullptr, c0 ? rep[1].data() : nullptr, H, Cs, stage, cols)) return rc;
    if (h0 || c0) HIP_TRY(hipStreamSynchronize(h->st));
    if (d_off) HIP_TRY(hipMemcpyAsync(d_off, prompt_off, sizeof(uint64_t) * (streams + 1), hipMemcpyHostToDevice, h->st));
    if (d_prompts) HIP_TRY(hipMemcpyAsync(d_prompts, prompts, total, hipMemcpyHostToDevice, h->st));
    std::vector<double> cost0(cols, (double)INFINITY);
    for (int s = 0; s < streams; s++) cost0[(size_t)s * W] = 0.0;
    HIP_TRY(hipMemcpyAsync(d_cost, cost0.data(), sizeof(double) * cols, hipMemcpyHostToDevice, h->st));
    HIP_TRY(hipMemsetAsync(d_len, 0, sizeof(int32_t) * cols, h->st));
    HIP_TRY(hipMemsetAsync(d_fin, 0, sizeof(int32_t) * cols, h->st));
    std::vector<int32_t> fin0, q0; // (alive until the synchronize below)
    if (con) { // slots 1..W-1 start finished ("no such hypothesis"), every slot in its stream's state
        fin0.assign(cols, 1);
        q0.resize(cols);
        for (int c = 0; c < cols; c++) q0[c] = cstate[c / W];
        for (int s = 0; s < streams; s++) fin0[(size_t)s * W] = 0;
        HIP_TRY(hipMemcpyAsync(d_fin, fin0.data(), sizeof(int32_t) * cols, hipMemcpyHostToDevice, h->st));
        HIP_TRY(hipMemcpyAsync(d_q, q0.data(), sizeof(int32_t) * cols, hipMemcpyHostToDevice, h->st));
        HIP_TRY(hipMemcpyAsync(d_tab, con->next, sizeof(uint16_t) * 256 * (size_t)Q, hipMemcpyHostToDevice, h->st));
    }
    if (accept) { // rows 0 .. count - 1: selection i reads row count - 1 - i
        HIP_TRY(hipMemcpyAsync(d_acc, accept, (size_t)Q, hipMemcpyHostToDevice, h->st));
        HIP_TRY(hipMemcpyAsync(d_F, frows.data(), sizeof(uint32_t) * (size_t)count * fwords, hipMemcpyHostToDevice, h->st));
    }
    HIP_TRY(hipMemsetAsync(d_tp, 0, nd, h->st));
    HIP_TRY(hipMemsetAsync(d_tb, 0, nd, h->st));
    const Model m = model_of(h);
    RUN(K_PACK_U, pack_U(m.U, Ufwd, nullptr, N, h->st));

    BeamHeadArgs a{};
    a.Why = m.Why;
    a.by = m.by;
    a.H = H;
    a.C = Cs;
    a.Hr = H + n;
    a.Cr = Cs + n;
    a.prompts = d_prompts;
    a.off = d_off;
    a.x_next = xi;
    a.cost = d_cost;
    a.len = d_len;
    a.fin = d_fin;
    a.trace_parent = d_tp;
    a.trace_byte = d_tb;
    a.N = N;
    a.streams = streams;
    a.W = W;
    a.count = count;
    a.stop_byte = opt->stop_byte;
    a.ctab = d_tab;
    a.cstate = d_q;
    a.accept = d_acc;
    a.frows = d_F;
    a.fwords = fwords;
    const long long steps = (long long)max_len + count; // the longest stream's last selection is at step steps - 1
    for (long long t = 0; t < steps; t++) {
        hipError_t refused = hipSuccess;
        RUN(K_BEAM_HEAD, refused = beam_head(a, t, h->st));
        if (refused != hipSuccess) return head_refused("beam_search", "beam_head", refused);
        if (t + 1 == steps) break;
        if (int rc = step_columns(h, m, Ufwd, a.Hr, a.Cr, H, Cs, G, xi, cols)) return rc;
    }
    RUN(K_BEAM_BACKTRACK, beam_backtrack(d_tp, d_tb, d_len, d_out, streams, W, count, h->st));

    HIP_TRY(hipMemcpyAsync(out, d_out, nd, hipMemcpyDeviceToHost, h->st));
    HIP_TRY(hipMemcpyAsync(out_len, d_len, sizeof(int32_t) * cols, hipMemcpyDeviceToHost, h->st));
    HIP_TRY(hipMemcpyAsync(bits, d_cost, sizeof(double) * cols, hipMemcpyDeviceToHost, h->st));
    if (trace_parent) HIP_TRY(hipMemcpyAsync(trace_parent, d_tp, nd, hipMemcpyDeviceToHost, h->st));
    if (trace_byte) HIP_TRY(hipMemcpyAsync(trace_byte, d_tb, nd, hipMemcpyDeviceToHost, h->st));
    if (end_state) HIP_TRY(hipMemcpyAsync(end_state, d_q, sizeof(int32_t) * cols, hipMemcpyDeviceToHost, h->st));
    HIP_TRY(hipStreamSynchronize(h->st));
    return 0;
}

// Per-byte scores (include/lstm_hip.h): the generator's loop with score_head in gen_head's place.  Per
// step one score_head launch (byte t of every stream: logits, surprisal, entropy, rank, alternatives, the next input, final
// states) and one k_fwd_step; max length + 1 head launches, max length steps, no readback inside the loop.  A constraint is
// checked and every stream's text walked through it here, on the host, before anything is launched: the state each byte stands
// in is uploaded beside the text.  Only P of the handle is read; the working memory is gen_scratch.
int lstm_hip_score(lstm_hip_t *h, int32_t streams, const uint8_t *text, const uint64_t *text_off, const float *h0, const float *c0,
                   const lstm_hip_scoring *opt, const int32_t *start_state, const lstm_hip_scores *out, float *h_out,
                   float *c_out) {
    return lstm_hip_score_guided(h, streams, text, text_off, h0, c0, opt, start_state, out, h_out, c_out, nullptr);
}

// Guides, as in lstm_hip_generate_guided: per step one guide_logits launch ahead of score_head (a.gsum
// set: every scored byte is scored under the mixed logits, the constraint mask behind the mix) and one k_fwd_step per guide.  The
// guides' pieces are the last of the scratch layout: with gd NULL every offset, upload and launch is lstm_hip_score's.
int lstm_hip_score_guided(lstm_hip_t *h, int32_t streams, const uint8_t *text, const uint64_t *text_off, const float *h0,
                          const float *c0, const lstm_hip_scoring *opt, const int32_t *start_state, const lstm_hip_scores *out,
                          float *h_out, float *c_out, const lstm_hip_guidance *gd) {
    CHECK(h);
    if (!opt) return fail(LSTM_HIP_EINVAL, "score: null options");
    if (opt->size != sizeof(lstm_hip_scoring))
        return fail(LSTM_HIP_EINVAL, "score: options of %u bytes, expected %zu", opt->size, sizeof(lstm_hip_scoring));
    if (out && out->size != sizeof(lstm_hip_scores))
        return fail(LSTM_HIP_EINVAL, "score: outputs of %u bytes, expected %zu", out->size, sizeof(lstm_hip_scores));
    if (opt->first != 0 && opt->first != 1) return fail(LSTM_HIP_EINVAL, "score: first must be 0 or 1 (got %d)", opt->first);
    const int top_n = opt->top_n;
    if (top_n < 0 || top_n > 8) return fail(LSTM_HIP_EINVAL, "score: top_n must be in [0, 8] (got %d)", top_n);
    lstm_hip_scores o{};
    if (out) o = *out;
    if (top_n == 0 && (o.top_byte || o.top_bits)) return fail(LSTM_HIP_EINVAL, "score: top_byte / top_bits given with top_n = 0");
    const lstm_hip_constraint *con = opt->con;
    if (!con && (start_state || o.end_state)) return fail(LSTM_HIP_EINVAL, "score: start_state / end_state given without a constraint");
    if (streams < 1 || streams > 4096) return fail(LSTM_HIP_EINVAL, "score: streams must be in [1, 4096] (got %d)", streams);
    if (int rc = check_offsets("score", "text_off", text_off, streams)) return rc;
    const uint64_t total = text_off[streams];
    if (total > 0 && !text) return fail(LSTM_HIP_EINVAL, "score: null text with %llu bytes to score", (unsigned long long)total);
    const uint64_t max_len = longest(text_off, streams);
    const int N = h->cfg.N;
    if (N > 16384) return fail(LSTM_HIP_EINVAL, "score: hidden width %d above 16384", N);
    std::vector<int32_t> cstate;  // [streams] each stream's state: at its start, then after its text
    std::vector<uint16_t> ccount; // (the allowed counts are checked, not used)
    std::vector<uint16_t> qpos;   // [total] the state each byte stands in
    const int Q = con ? con->states : 0;
    if (con) {
        if (int rc = check_constraint("score", con, streams, start_state, cstate, ccount)) return rc;
        qpos.resize(total);
        if (int rc = walk_constraint("score", "byte", con, streams, text, text_off, cstate, qpos.data())) return rc;
    }
    Guides gs;
    if (gd)
        if (int rc = check_guidance("score", h, gd, gs)) return rc;
    const size_t n = (size_t)N * streams, nl = (size_t)h->N_log * streams, tot = (size_t)total;
    const bool keep = h_out || c_out;

    // (an output of a call without bytes is absent: nothing to zero, nothing to copy back, null to the head)
    float4 *Ufwd;
    float *H, *Cs, *G, *ho, *stage, *d_sur, *d_ent, *d_tbi;
    int32_t *xi;
    uint64_t *d_off;
    uint8_t *d_text, *d_rank, *d_tby;
    double *d_bits;
    uint16_t *d_tab, *d_q;
    Scratch mem;
    mem.piece(Ufwd, (size_t)N * N).piece(H, 2 * n).piece(Cs, 2 * n).piece(G, 4 * n).piece(ho, 2 * n, keep);
    mem.piece(stage, 2 * nl, h->padded()).piece(xi, streams);
    mem.piece(d_off, streams + 1).piece(d_text, tot).piece(d_bits, streams);
    mem.piece(d_sur, tot, o.surprisal && tot).piece(d_ent, tot, o.entropy && tot).piece(d_rank, tot, o.rank && tot);
    mem.piece(d_tby, tot * top_n, o.top_byte && tot).piece(d_tbi, tot * top_n, o.top_bits && tot);
    mem.piece(d_tab, 256 * (size_t)Q, con != nullptr).piece(d_q, tot, con != nullptr);
    guide_pieces(mem, gs, gd, streams);
    if (int rc = mem.commit(h)) return rc;

    // start state (padding rows zero), inputs, zeroed outputs (the entries of unscored bytes stay zero)
    if (int rc = upload_states(h, h0, c0, H, Cs, stage, streams)) return rc;
    HIP_TRY(hipMemcpyAsync(d_off, text_off, sizeof(uint64_t) * (streams + 1), hipMemcpyHostToDevice, h->st));
    if (tot) HIP_TRY(hipMemcpyAsync(d_text, text, tot, hipMemcpyHostToDevice, h->st));
    HIP_TRY(hipMemsetAsync(d_bits, 0, sizeof(double) * streams, h->st));
    if (d_sur) HIP_TRY(hipMemsetAsync(d_sur, 0, sizeof(float) * tot, h->st));
    if (d_ent) HIP_TRY(hipMemsetAsync(d_ent, 0, sizeof(float) * tot, h->st));
    if (d_rank) HIP_TRY(hipMemsetAsync(d_rank, 0, tot, h->st));
    if (d_tby) HIP_TRY(hipMemsetAsync(d_tby, 0, tot * top_n, h->st));
    if (d_tbi) HIP_TRY(hipMemsetAsync(d_tbi, 0, sizeof(float) * tot * top_n, h->st));
    if (con) {
        HIP_TRY(hipMemcpyAsync(d_tab, con->next, sizeof(uint16_t) * 256 * (size_t)Q, hipMemcpyHostToDevice, h->st));
        if (tot) HIP_TRY(hipMemcpyAsync(d_q, qpos.data(), sizeof(uint16_t) * tot, hipMemcpyHostToDevice, h->st));
    }
    const Model m = model_of(h);
    RUN(K_PACK_U, pack_U(m.U, Ufwd, nullptr, N, h->st));
    GuideLogitsArgs ga{};
    if (int rc = guides_begin(h, gs, gd, streams, ga)) return rc;
    ga.off = d_off;
    ga.scorer = 1;
    ga.first = opt->first;

    ScoreHeadArgs a{};
    a.Why = m.Why;
    a.by = m.by;
    a.text = d_text;
    a.off = d_off;
    a.surprisal = d_sur;
    a.entropy = d_ent;
    a.rank = d_rank;
    a.top_byte = d_tby;
    a.top_bits = d_tbi;
    a.bits = o.bits ? d_bits : nullptr;
    a.x_next = xi;
    a.h_out = ho;
    a.c_out = ho ? ho + n : nullptr;
    a.ctab = d_tab;
    a.qpos = d_q;
    a.N = N;
    a.streams = streams;
    a.first = opt->first;
    a.top_n = top_n;
    a.gsum = gs.gsum;
    a.wmain = gs.wmain;
    const bool stable = (h->cfg.flags & LSTM_HIP_STABLE_SOFTMAX) != 0;
    int cur = 0;
    for (uint64_t t = 0;; t++) {
        a.H = H + cur * n;
        a.C = Cs + cur * n;
        if (gs.count)
            if (int rc = guides_logits(h, "score", gs, ga, cur, (long long)t)) return rc;
        hipError_t refused = hipSuccess;
        RUN(K_SCORE_HEAD, refused = score_head(a, (long long)t, stable, h->st));
        if (refused != hipSuccess) return head_refused("score", "score_head", refused);
        if (t == max_len) break;
        if (int rc = step_columns(h, m, Ufwd, a.H, a.C, H + (cur ^ 1) * n, Cs + (cur ^ 1) * n, G, xi, streams)) return rc;
        if (int rc = guides_step(h, gs, cur, xi, streams)) return rc;
        cur ^= 1;
    }

    if (d_sur) HIP_TRY(hipMemcpyAsync(o.surprisal, d_sur, sizeof(float) * tot, hipMemcpyDeviceToHost, h->st));
    if (d_ent) HIP_TRY(hipMemcpyAsync(o.entropy, d_ent, sizeof(float) * tot, hipMemcpyDeviceToHost, h->st));
    if (d_rank) HIP_TRY(hipMemcpyAsync(o.rank, d_rank, tot, hipMemcpyDeviceToHost, h->st));
    if (d_tby) HIP_TRY(hipMemcpyAsync(o.top_byte, d_tby, tot * top_n, hipMemcpyDeviceToHost, h->st));
    if (d_tbi) HIP_TRY(hipMemcpyAsync(o.top_bits, d_tbi, sizeof(float) * tot * top_n, hipMemcpyDeviceToHost, h->st));
    if (o.bits) HIP_TRY(hipMemcpyAsync(o.bits, d_bits, sizeof(double) * streams, hipMemcpyDeviceToHost, h->st));
    if (int rc = download_states(h, h_out, c_out, a.h_out, a.c_out, stage, streams)) return rc;
    if (int rc = guides_finish(h, gs, gd, streams)) return rc;
    HIP_TRY(hipStreamSynchronize(h->st));
    if (o.end_state) std::copy(cstate.begin(), cstate.end(), o.end_state);
    return 0;
}

// Held-out bits of many texts (include/lstm_hip.h).  The schedule first: host only.  It is the
// schedule of the text windows too (lstm_hip_text_plan, section 3.18), which have `steps` = S - 1 rows where these have 128.
static int64_t text_plan(int32_t steps, int32_t lanes, int32_t streams, const uint64_t *off, int32_t *lane_of, int64_t *first_window,
                         std::vector<int32_t> *slot) { // slot (may be null): [windows][lanes], the stream a lane holds, -1 idle
    std::vector<std::pair<int32_t, int64_t>> placed(streams, {-1, -1});
    // lowest next free window, lowest lane on ties: a heap of (window, lane) pairs
    typedef std::pair<int64_t, int32_t> Free;
    std::vector<Free> heap;
    for (int32_t l = 0; l < lanes; l++) heap.push_back({0, l});
    const auto later = [](const Free &a, const Free &b) { return a > b; };
    std::make_heap(heap.begin(), heap.end(), later);
    int64_t windows = 0;
    for (int32_t s = 0; s < streams; s++) {
        const uint64_t len = off[s + 1] - off[s], n = len > 0 ? len - 1 : 0;
        if (n > 0) {
            std::pop_heap(heap.begin(), heap.end(), later);
            Free &f = heap.back();
            placed[s] = {f.second, f.first};
            f.first += (int64_t)((n + steps - 1) / steps);
            windows = std::max(windows, f.first);
            std::push_heap(heap.begin(), heap.end(), later);
        }
        if (lane_of) lane_of[s] = placed[s].first;
        if (first_window) first_window[s] = placed[s].second;
    }
    if (slot) {
        slot->assign((size_t)windows * lanes, -1);
        for (int32_t s = 0; s < streams; s++) {
            if (placed[s].first < 0) continue;
            const uint64_t n = off[s + 1] - off[s] - 1;
            const int64_t k = (int64_t)((n + steps - 1) / steps);
            for (int64_t w = placed[s].second; w < placed[s].second + k; w++) (*slot)[(size_t)w * lanes + placed[s].first] = s;
        }
    }
    return windows;
}
// both public plans, under the caller's name in a refusal
static int64_t checked_plan(const char *what, int32_t steps, int32_t lanes, int32_t streams, const uint64_t *text_off,
                            int32_t *lane_of, int64_t *first_window, std::vector<int32_t> *slot) {
    if (steps < 1) return fail(LSTM_HIP_EINVAL, "%s: steps must be >= 1 (got %d)", what, steps);
    if (lanes < 1 || lanes > 4096) return fail(LSTM_HIP_EINVAL, "%s: lanes must be in [1, 4096] (got %d)", what, lanes);
    if (streams < 1) return fail(LSTM_HIP_EINVAL, "%s: streams must be >= 1 (got %d)", what, streams);
    if (int rc = check_offsets(what, "text_off", text_off, streams)) return rc;
    return text_plan(steps, lanes, streams, text_off, lane_of, first_window, slot);
}

// the cached internal handle of lstm_hip_eval_texts and lstm_hip_embed_texts: remade when `lanes` changes
static int texts_handle(lstm_hip_t *h, int lanes) {
    HIP_TRY(hipStreamSynchronize(h->st));
    if (h->texts_h && h->texts_h->cfg.B != lanes) {
        (void)lstm_hip_destroy(h->texts_h);
        h->texts_h = nullptr;
    }
    if (!h->texts_h) {
        lstm_hip_config c = h->cfg; // (cfg.N is the parent's internal width, as for the B = 1 evaluator's handle)
        c.S = LSTM_HIP_EVAL_STEPS + 1;
        c.B = lanes;
        c.flags = (h->cfg.flags & (LSTM_HIP_FAST_MATH | LSTM_HIP_STABLE_SOFTMAX | LSTM_HIP_STEP_KERNELS)) | LSTM_HIP_NO_FUSED_GRADS;
        if (int rc = lstm_hip_create(&c, &h->texts_h)) return rc;
    }
    return 0;
}

int64_t lstm_hip_text_plan(int32_t steps, int32_t lanes, int32_t streams, const uint64_t *text_off, int32_t *lane_of,
                           int64_t *first_window) {
    return checked_plan("text_plan", steps, lanes, streams, text_off, lane_of, first_window, nullptr);
}
int64_t lstm_hip_eval_plan(int32_t lanes, int32_t streams, const uint64_t *text_off, int32_t *lane_of, int64_t *first_window) {
    return checked_plan("eval_plan", LSTM_HIP_EVAL_STEPS, lanes, streams, text_off, lane_of, first_window, nullptr);
}

// What lstm_hip_eval_texts and lstm_hip_embed_texts share: the checks, the plan, the internal handle, the pieces of the call's
// scratch that every lane launch reads, their uploads, and the device loop.  Per window: lane_window, the internal handle's
// unchanged do_forward, the caller's fold, all on the internal handle's stream; the uploads and the state copies at either
// end run on the parent's, as every inference call's do, with the parent's generator scratch as working memory.  The internal
// handle runs in the window loop's mode that skips the probability store (nothing reads them); its profiling is off, so the
// parent's kernel statistics do not move.  A call goes checks, (its own checks), plan, (its own pieces), upload, (its own
// fills on h->st), loop, (its downloads).
struct TextsRun {
    lstm_hip_t *h = nullptr;
    lstm_hip_ctx *e = nullptr; // the internal handle
    int32_t streams = 0;
    int lanes = 0, feed_last = 0;
    const uint8_t *text = nullptr;
    const uint64_t *text_off = nullptr;
    uint64_t total = 0;
    int64_t windows = 0;
    std::vector<int32_t> slot, lane_of; // [windows][lanes]; [streams]
    std::vector<int64_t> first;         // [streams]
    float *H0 = nullptr, *C0 = nullptr, *stage = nullptr;
    uint64_t *d_off = nullptr, *d_skip = nullptr;
    int64_t *d_first = nullptr;
    int32_t *d_slot = nullptr;
    uint8_t *d_text = nullptr;
    double *d_bits = nullptr;
    Scratch mem; // the call's pieces: the shared ones from plan(), the caller's own between plan() and upload()

    // the refusals both calls have, under the caller's name; chooses `lanes`
    int checks(lstm_hip_t *handle, const char *what, int32_t n_streams, const uint8_t *bytes, const uint64_t *off,
              const lstm_hip_eval_opt *opt) {
        CHECK(handle);
        if (opt && opt->size != sizeof(lstm_hip_eval_opt))
            return fail(LSTM_HIP_EINVAL, "%s: options of %u bytes, expected %zu", what, opt->size, sizeof(lstm_hip_eval_opt));
        if (opt && (opt->lanes < 0 || opt->lanes > 4096))
            return fail(LSTM_HIP_EINVAL, "%s: lanes must be in [0, 4096] (got %d)", what, opt->lanes);
        if (n_streams < 1) return fail(LSTM_HIP_EINVAL, "%s: streams must be >= 1 (got %d)", what, n_streams);
        if (int rc = check_offsets(what, "text_off", off, n_streams)) return rc;
        if (off[n_streams] > 0 && !bytes)
            return fail(LSTM_HIP_EINVAL, "%s: null text with %llu bytes to read", what, (unsigned long long)off[n_streams]);
        h = handle, streams = n_streams, text = bytes, text_off = off, total = off[n_streams];
        lanes = opt && opt->lanes > 0 ? opt->lanes : h->cfg.B;
        return 0;
    }
    // The plan (host only) -- with feed_last that of streams one byte longer: a stream of L bytes gets ceil(L / 128) windows,
    // an empty one no lane -- then the internal handle and the shared pieces.  `stage_cols`: the widest download of the call.
    int plan(int feed, size_t stage_cols) {
        feed_last = feed;
        std::vector<uint64_t> longer;
        for (int32_t s = 0; feed_last && s <= streams; s++) longer.push_back(text_off[s] + (uint64_t)s);
        lane_of.resize(streams), first.resize(streams);
        windows = text_plan(LSTM_HIP_EVAL_STEPS, lanes, streams, feed_last ? longer.data() : text_off, lane_of.data(), first.data(), &slot);
        if (int rc = texts_handle(h, lanes)) return rc;
        e = h->texts_h;
        const size_t n = (size_t)h->cfg.N * streams;
        mem.piece(H0, n).piece(C0, n).piece(stage, 2 * (size_t)h->N_log * stage_cols, h->padded());
        mem.piece(d_off, streams + 1).piece(d_skip, streams).piece(d_first, streams).piece(d_slot, slot.size());
        mem.piece(d_text, (size_t)total).piece(d_bits, streams);
        return 0;
    }
    // commits the scratch, brings the parameters, the start states and the tables to the device (on h->st) and fills `a`
    int upload(const float *h0, const float *c0, const uint64_t *skip, LaneArgs &a) {
        if (int rc = mem.commit(h)) return rc;
        HIP_TRY(hipMemcpyAsync(e->P, infer_block(h), sizeof(float) * h->pl.total, hipMemcpyDeviceToDevice, h->st));
        if (e->plan.bf16()) return fail(LSTM_HIP_ESTATE, "the internal lane handle is not fp32"); // (texts_handle: its only live flag is `packed`)
        e->img.params_written();
        if (int rc = upload_states(h, h0, c0, H0, C0, stage, streams)) return rc;
        HIP_TRY(hipMemcpyAsync(d_off, text_off, sizeof(uint64_t) * (streams + 1), hipMemcpyHostToDevice, h->st));
        if (skip) HIP_TRY(hipMemcpyAsync(d_skip, skip, sizeof(uint64_t) * streams, hipMemcpyHostToDevice, h->st));
        else HIP_TRY(hipMemsetAsync(d_skip, 0, sizeof(uint64_t) * streams, h->st));
        HIP_TRY(hipMemcpyAsync(d_first, first.data(), sizeof(int64_t) * streams, hipMemcpyHostToDevice, h->st));
        if (!slot.empty()) HIP_TRY(hipMemcpyAsync(d_slot, slot.data(), sizeof(int32_t) * slot.size(), hipMemcpyHostToDevice, h->st));
        if (total) HIP_TRY(hipMemcpyAsync(d_text, text, (size_t)total, hipMemcpyHostToDevice, h->st));
        HIP_TRY(hipMemsetAsync(d_bits, 0, sizeof(double) * streams, h->st));
        a.text = d_text;
        a.off = d_off;
        a.skip = d_skip;
        a.slot = d_slot;
        a.first = d_first;
        a.H0 = H0;
        a.C0 = C0;
        a.xi = e->xi;
        a.ti = e->ti;
        a.H = e->H;
        a.C = e->C;
        a.colloss = e->colloss;
        a.bits = d_bits;
        a.lanes = lanes;
        a.N = h->cfg.N;
        a.feed_last = feed_last;
        return 0;
    }
    // the device loop; `fold` launches window w's fold on e->st and returns its status.  elapsed_ms (may be null): the loop's
    // HIP-event time
    int loop(const LaneArgs &a, const std::function<int(int64_t)> &fold, float *elapsed_ms) {
        HIP_TRY(hipStreamSynchronize(h->st)); // (the host vectors are pageable: their copies are done; the loop is on e's stream)
        struct LoopMode { // the internal handle is back in its standalone mode on every return path
            lstm_hip_ctx *e;
            ~LoopMode() { e->in_loop = false, e->keep_outputs = true; }
        } loop_mode{e};
        e->in_loop = true;
        e->keep_outputs = false;
        if (elapsed_ms) HIP_TRY(hipEventRecord(e->evt0, e->st));
        for (int64_t w = 0; w < windows; w++) {
            lane_window(a, w, e->plan.n_cus, e->st);
            if (int rc = untimed_status("lane_window")) return rc;
            if (int rc = do_forward(e)) return rc;
            if (int rc = fold(w)) return rc;
        }
        if (elapsed_ms) {
            HIP_TRY(hipEventRecord(e->evt1, e->st));
            HIP_TRY(hipEventSynchronize(e->evt1));
            HIP_TRY(hipEventElapsedTime(elapsed_ms, e->evt0, e->evt1));
        }
        HIP_TRY(hipStreamSynchronize(e->st));
        return check_abort(e);
    }
};

// Held-out bits: the run with feed_last = 0 and eval_fold.
int lstm_hip_eval_texts(lstm_hip_t *h, int32_t streams, const uint8_t *text, const uint64_t *text_off, const float *h0, const float *c0,
                        const uint64_t *skip, const lstm_hip_eval_opt *opt, double *bits, float *surprisal, float *h_out,
                        float *c_out, float *elapsed_ms) {
    TextsRun r;
    if (int rc = r.checks(h, "eval_texts", streams, text, text_off, opt)) return rc;
    const size_t n = (size_t)h->cfg.N * streams, tot = (size_t)r.total;
    float *ho, *d_sur;
    if (int rc = r.plan(0, streams)) return rc;
    r.mem.piece(ho, 2 * n, h_out || c_out).piece(d_sur, tot, surprisal && tot);
    EvalArgs a{};
    if (int rc = r.upload(h0, c0, skip, a)) return rc;
    if (ho) { // a stream without a step never reaches the fold: its final state is its start state
        HIP_TRY(hipMemcpyAsync(ho, r.H0, sizeof(float) * n, hipMemcpyDeviceToDevice, h->st));
        HIP_TRY(hipMemcpyAsync(ho + n, r.C0, sizeof(float) * n, hipMemcpyDeviceToDevice, h->st));
    }
    if (d_sur) HIP_TRY(hipMemsetAsync(d_sur, 0, sizeof(float) * tot, h->st));
    a.sur = d_sur;
    a.Hout = h_out ? ho : nullptr;
    a.Cout = c_out ? ho + n : nullptr;
    const auto fold = [&](int64_t w) {
        eval_fold(a, w, r.e->plan.n_cus, r.e->st);
        return untimed_status("eval_fold");
    };
    if (int rc = r.loop(a, fold, elapsed_ms)) return rc;

    if (bits) HIP_TRY(hipMemcpyAsync(bits, r.d_bits, sizeof(double) * streams, hipMemcpyDeviceToHost, h->st));
    if (d_sur) HIP_TRY(hipMemcpyAsync(surprisal, d_sur, sizeof(float) * tot, hipMemcpyDeviceToHost, h->st));
    if (int rc = download_states(h, h_out, c_out, ho, ho ? ho + n : nullptr, r.stage, streams)) return rc;
    HIP_TRY(hipStreamSynchronize(h->st));
    return 0;
}

// Hidden states of many texts (include/lstm_hip.h): the run with feed_last = 1 (n = L steps: the last
// byte is fed) and embed_fold.  The outputs are blocks of internal-width columns in the call's scratch, [streams][N] per pool
// and source and [npick][N] per picked source, brought home through download_states like any state.
int lstm_hip_embed_texts(lstm_hip_t *h, int32_t streams, const uint8_t *text, const uint64_t *text_off, const float *h0, const float *c0,
                         const uint64_t *skip, const lstm_hip_eval_opt *opt, const uint64_t *pick, int64_t npick,
                         const lstm_hip_embedding *out, float *elapsed_ms) {
    TextsRun r;
    if (int rc = r.checks(h, "embed_texts", streams, text, text_off, opt)) return rc;
    if (!out) return fail(LSTM_HIP_EINVAL, "embed_texts: null out");
    if (out->size != sizeof(lstm_hip_embedding))
        return fail(LSTM_HIP_EINVAL, "embed_texts: outputs of %u bytes, expected %zu", out->size, sizeof(lstm_hip_embedding));
    if (npick < 0) return fail(LSTM_HIP_EINVAL, "embed_texts: npick must be >= 0 (got %lld)", (long long)npick);
    if (npick > 0 && !pick) return fail(LSTM_HIP_EINVAL, "embed_texts: null pick with npick = %lld", (long long)npick);
    for (int64_t k = 0; k < npick; k++) {
        if (pick[k] >= r.total)
            return fail(LSTM_HIP_EINVAL, "embed_texts: pick[%lld] = %llu is not below text_off[streams] = %llu", (long long)k,
                        (unsigned long long)pick[k], (unsigned long long)r.total);
        if (k > 0 && pick[k] <= pick[k - 1])
            return fail(LSTM_HIP_EINVAL, "embed_texts: pick must be strictly increasing (pick[%lld] = %llu after %llu)", (long long)k,
                        (unsigned long long)pick[k], (unsigned long long)pick[k - 1]);
    }
    const int pick_sources = (out->picked_h ? 1 : 0) + (out->picked_c ? 1 : 0);
    if (npick == 0 && pick_sources) return fail(LSTM_HIP_EINVAL, "embed_texts: picked_h / picked_c given with npick = 0");
    if (npick > 0 && !pick_sources) return fail(LSTM_HIP_EINVAL, "embed_texts: npick = %lld with neither picked_h nor picked_c", (long long)npick);
    const int N = h->cfg.N;
    const uint64_t pick_limit = (uint64_t)1 << 30;
    if ((uint64_t)npick > pick_limit / ((uint64_t)N * sizeof(float) * (pick_sources ? pick_sources : 1)))
        return fail(LSTM_HIP_EINVAL, "embed_texts: %lld picked positions of width %d from %d source(s) need more than %llu bytes",
                    (long long)npick, N, pick_sources, (unsigned long long)pick_limit);

    if (int rc = r.plan(1, std::max((size_t)streams, (size_t)npick))) return rc;

    // every pick as (lane, row, k), sorted by window; pick_at[w] .. pick_at[w + 1] are window w's
    std::vector<int64_t> pick_at(r.windows + 1, 0);
    std::vector<int32_t> table((size_t)npick * 3);
    {
        std::vector<int64_t> win(npick);
        int32_t s = 0;
        for (int64_t k = 0; k < npick; k++) { // (increasing picks: the stream index only moves forward)
            while (pick[k] >= text_off[s + 1]) s++;
            win[k] = r.first[s] + (int64_t)((pick[k] - text_off[s]) / LSTM_HIP_EVAL_STEPS);
            pick_at[win[k] + 1]++;
        }
        for (int64_t w = 0; w < r.windows; w++) pick_at[w + 1] += pick_at[w];
        std::vector<int64_t> next(pick_at.begin(), pick_at.end() - 1);
        s = 0;
        for (int64_t k = 0; k < npick; k++) {
            while (pick[k] >= text_off[s + 1]) s++;
            int32_t *t = &table[(size_t)next[win[k]]++ * 3];
            t[0] = r.lane_of[s];
            t[1] = (int32_t)((pick[k] - text_off[s]) % LSTM_HIP_EVAL_STEPS) + 1;
            t[2] = (int32_t)k;
        }
    }

    const size_t n = (size_t)N * streams, np = (size_t)N * npick;
    const bool want[2] = {out->mean_h || out->max_h || out->last_h, out->mean_c || out->max_c || out->last_c};
    float *pool[2], *picked[2];
    double *d_sum[2];
    int32_t *d_picks;
    for (int x = 0; x < 2; x++) r.mem.piece(d_sum[x], n, want[x]).piece(pool[x], 3 * n, want[x]); // mean | max | last
    r.mem.piece(picked[0], np, out->picked_h != nullptr).piece(picked[1], np, out->picked_c != nullptr);
    r.mem.piece(d_picks, table.size(), npick > 0);
    EmbedArgs a{};
    if (int rc = r.upload(h0, c0, skip, a)) return rc;
    for (int x = 0; x < 2; x++) { // a stream without a byte never reaches the fold: empty pools, last = its start state
        if (!want[x]) continue;
        HIP_TRY(hipMemsetAsync(pool[x], 0, sizeof(float) * 2 * n, h->st));
        HIP_TRY(hipMemcpyAsync(pool[x] + 2 * n, x ? r.C0 : r.H0, sizeof(float) * n, hipMemcpyDeviceToDevice, h->st));
    }
    if (npick) HIP_TRY(hipMemcpyAsync(d_picks, table.data(), sizeof(int32_t) * table.size(), hipMemcpyHostToDevice, h->st));
    for (int x = 0; x < 2; x++) {
        a.sum[x] = d_sum[x];
        a.mean[x] = pool[x];
        a.maxv[x] = want[x] ? pool[x] + n : nullptr;
        a.last[x] = want[x] ? pool[x] + 2 * n : nullptr;
        a.picked[x] = picked[x];
    }
    a.picks = d_picks;
    const auto fold = [&](int64_t w) {
        embed_fold(a, w, pick_at[w], pick_at[w + 1], r.e->plan.n_cus, r.e->st);
        return untimed_status("embed_fold");
    };
    if (int rc = r.loop(a, fold, elapsed_ms)) return rc;

    if (out->bits) HIP_TRY(hipMemcpyAsync(out->bits, r.d_bits, sizeof(double) * streams, hipMemcpyDeviceToHost, h->st));
    if (int rc = download_states(h, out->mean_h, out->mean_c, pool[0], pool[1], r.stage, streams)) return rc;
    if (int rc = download_states(h, out->max_h, out->max_c, a.maxv[0], a.maxv[1], r.stage, streams)) return rc;
    if (int rc = download_states(h, out->last_h, out->last_c, a.last[0], a.last[1], r.stage, streams)) return rc;
    if (npick)
        if (int rc = download_states(h, out->picked_h, out->picked_c, picked[0], picked[1], r.stage, (int)npick)) return rc;
    HIP_TRY(hipStreamSynchronize(h->st));
    if (out->count)
        for (int32_t s = 0; s < streams; s++) {
            const uint64_t L = text_off[s + 1] - text_off[s], k = skip ? skip[s] : 0;
            out->count[s] = k < L ? (int64_t)(L - k) : 0;
        }
    return 0;
}

// Both directions: per step one code_head launch and one k_fwd_step over all streams (the generator's loop), from the fp32
// master parameters P and a fragment image of U made for the call (the adaptive calls: remade for every block), in the
// handle's generator scratch memory.  Encoder: `text` in, the streams' codes (at lstm_hip_code_bound offsets) out; decoder:
// `code` at `code_off` in, `text` out.  A run is begun once, stepped over ranges of t that together cover [0, max_len) in
// order (the static calls: one range), and finished once; the coder state of every stream, x_next and the H / C ping-pong
// live on the device or in the run between ranges, so a pause between two ranges changes no code.
// The mixed calls (lstm_hip_encode_mixed / lstm_hip_decode_mixed) fill r.gs ahead of coder_begin: the
// guides' pieces, their logits zk, the streams' weights and the weight trace are then carved behind every piece of the unmixed
// run, and per step guide_logits (coder mode), code_head_mixed in code_head's place, and one k_fwd_step per guide behind the
// main model's.  With r.gs.count == 0 nothing of that is carved, uploaded or launched.
struct CoderRun {
    CodeHeadArgs a{};
    bool decode = false;
    int32_t streams = 0;
    uint64_t total = 0, max_len = 0, code_bytes = 0;
    std::vector<uint64_t> base; // each stream's code range on the device
    size_t n = 0;               // N * streams
    Model m{};
    float4 *Ufwd = nullptr;
    float *H = nullptr, *Cs = nullptr, *G = nullptr;
    double *bits_prev = nullptr, *block_bits = nullptr; // adaptive calls: per-stream bits at the last fold, per-block totals
    int cur = 0;
    Guides gs;                  // mixed calls: the guides (count == 0: an unmixed run)
    GuideLogitsArgs ga{};
    float *zk = nullptr;        // [streams][guides][256]
    float rate = 0.0f;
    std::vector<float> v0;      // the call's weights, once per stream
};
static int coder_begin(lstm_hip_t *h, CoderRun &r, bool decode, int32_t streams, const uint64_t *text_off, const uint8_t *text_in,
                       const uint8_t *code_in, const uint64_t *code_off_in, bool want_trace, int64_t n_block_bits,
                       const lstm_hip_guidance *gd = nullptr, bool want_w_trace = false) {
    const int N = h->cfg.N;
    r.decode = decode;
    r.streams = streams;
    r.total = text_off[streams];
    r.max_len = longest(text_off, streams);
    r.base.assign(streams + 1, 0);
    if (decode) r.base.assign(code_off_in, code_off_in + streams + 1);
    else
        for (int s = 0; s < streams; s++) r.base[s + 1] = r.base[s] + lstm_hip_code_bound(text_off[s + 1] - text_off[s]);
    r.code_bytes = r.base[streams];
    const uint64_t total = r.total, code_bytes = r.code_bytes;
    const size_t n = r.n = (size_t)N * streams;

    CodeHeadArgs &a = r.a;
    a = CodeHeadArgs{};
    uint64_t *d_toff, *d_base;
    double *d_bits;   // (the encoder's; carved and zeroed for the decoder too, which gets no pointer to them)
    uint32_t *d_trace;
    Scratch mem;
    mem.piece(r.Ufwd, (size_t)N * N).piece(r.H, 2 * n).piece(r.Cs, 2 * n).piece(r.G, 4 * n).piece(a.x_next, streams);
    mem.piece(d_toff, streams + 1).piece(d_base, streams + 1).piece(a.text, total).piece(a.code, code_bytes);
    mem.piece(a.state, streams).piece(a.code_len, streams).piece(d_bits, streams);
    mem.piece(d_trace, 3 * total, want_trace).piece(a.err, 1);
    mem.piece(r.bits_prev, streams, n_block_bits != 0).piece(r.block_bits, n_block_bits, n_block_bits != 0);
    const int G = r.gs.count;
    guide_pieces(mem, r.gs, gd, streams);
    mem.piece(r.zk, (size_t)256 * G * streams, G > 0).piece(a.v, (size_t)(1 + G) * streams, G > 0);
    mem.piece(a.w_trace, (size_t)(1 + G) * total, G > 0 && want_w_trace && !decode);
    if (int rc = mem.commit(h)) return rc;
    r.cur = 0;
    r.m = model_of(h);
    a.Why = r.m.Why;
    a.by = r.m.by;
    a.text_off = d_toff;
    a.code_base = d_base;
    a.bits = decode ? nullptr : d_bits;
    a.trace = decode ? nullptr : d_trace;
    a.N = N;
    a.streams = streams;
    a.decode = decode ? 1 : 0;

    HIP_TRY(hipMemsetAsync(r.H, 0, sizeof(float) * n, h->st)); // every stream starts from h = c = 0 (padding rows too)
    HIP_TRY(hipMemsetAsync(r.Cs, 0, sizeof(float) * n, h->st));
    HIP_TRY(hipMemcpyAsync(d_toff, text_off, sizeof(uint64_t) * (streams + 1), hipMemcpyHostToDevice, h->st));
    HIP_TRY(hipMemcpyAsync(d_base, r.base.data(), sizeof(uint64_t) * (streams + 1), hipMemcpyHostToDevice, h->st));
    if (!decode && total) HIP_TRY(hipMemcpyAsync(a.text, text_in, total, hipMemcpyHostToDevice, h->st));
    if (decode && code_bytes) HIP_TRY(hipMemcpyAsync(a.code, code_in, code_bytes, hipMemcpyHostToDevice, h->st));
    HIP_TRY(hipMemsetAsync(a.code_len, 0, sizeof(uint64_t) * streams, h->st)); // (empty streams: no code)
    HIP_TRY(hipMemsetAsync(d_bits, 0, sizeof(double) * streams, h->st));
    HIP_TRY(hipMemsetAsync(a.err, 0, sizeof(uint32_t), h->st));
    if (n_block_bits) {
        HIP_TRY(hipMemsetAsync(r.bits_prev, 0, sizeof(double) * streams, h->st));
        HIP_TRY(hipMemsetAsync(r.block_bits, 0, sizeof(double) * n_block_bits, h->st));
    }
    if (G) { // every guide from h = c = 0, its image of U; every stream's weights the call's
        r.ga = GuideLogitsArgs{};
        if (int rc = guides_begin(h, r.gs, gd, streams, r.ga)) return rc;
        r.ga.off = d_toff;
        r.ga.coder = 1;
        r.ga.zk = r.zk;
        a.zk = r.zk;
        a.nguides = G;
        a.rate = r.rate;
        r.v0.resize((size_t)(1 + G) * streams);
        for (int s = 0; s < streams; s++) {
            r.v0[(size_t)s * (1 + G)] = r.gs.wmain;
            for (int k = 0; k < G; k++) r.v0[(size_t)s * (1 + G) + 1 + k] = r.gs.r[k].w;
        }
        HIP_TRY(hipMemcpyAsync(a.v, r.v0.data(), sizeof(float) * r.v0.size(), hipMemcpyHostToDevice, h->st));
    }
    return 0;
}
// steps t0 .. t1-1 with the current P: the image of U is remade first, then per step code_head and (except behind the last
// byte of the longest stream) fwd_step on the byte just coded
static int coder_steps(lstm_hip_t *h, CoderRun &r, uint64_t t0, uint64_t t1) {
    if (t0 >= t1) return 0;
    const size_t n = r.n;
    RUN(K_PACK_U, pack_U(r.m.U, r.Ufwd, nullptr, h->cfg.N, h->st));
    for (long long t = (long long)t0; t < (long long)t1; t++) {
        r.a.H = r.H + r.cur * n;
        if (r.gs.count) {
            const char *what = r.decode ? "decode" : "encode";
            if (int rc = guides_logits(h, what, r.gs, r.ga, r.cur, t)) return rc;
            hipError_t refused = hipSuccess;
            RUN(K_CODE_HEAD_MIXED, refused = code_head_mixed(r.a, t, h->st));
            if (refused != hipSuccess) return head_refused(what, "code_head_mixed", refused);
        } else
            RUN(K_CODE_HEAD, code_head(r.a, t, h->st));
        if (t + 1 == (long long)r.max_len) break;
        if (int rc = step_columns(h, r.m, r.Ufwd, r.a.H, r.Cs + r.cur * n, r.H + (r.cur ^ 1) * n, r.Cs + (r.cur ^ 1) * n, r.G,
                                  r.a.x_next, r.streams))
            return rc;
        if (int rc = guides_step(h, r.gs, r.cur, r.a.x_next, r.streams)) return rc;
        r.cur ^= 1;
    }
    return 0;
}
static int coder_finish(lstm_hip_t *h, CoderRun &r, uint8_t *text_out, uint8_t *code_out, uint64_t *code_off_out, double *bits,
                        uint32_t *trace, double *block_bits, int64_t n_block_bits, float *w_out = nullptr, float *w_trace = nullptr) {
    const bool decode = r.decode;
    const int32_t streams = r.streams;
    const uint64_t total = r.total, code_bytes = r.code_bytes;
    const CodeHeadArgs &a = r.a;
    const char *what = decode ? "decode" : "encode";
    uint32_t err = 0;
    std::vector<uint64_t> len(streams);
    HIP_TRY(hipMemcpyAsync(&err, a.err, sizeof(uint32_t), hipMemcpyDeviceToHost, h->st));
    if (decode) {
        if (total) HIP_TRY(hipMemcpyAsync(text_out, a.text, total, hipMemcpyDeviceToHost, h->st));
    } else {
        HIP_TRY(hipMemcpyAsync(len.data(), a.code_len, sizeof(uint64_t) * streams, hipMemcpyDeviceToHost, h->st));
        if (code_bytes) HIP_TRY(hipMemcpyAsync(code_out, a.code, code_bytes, hipMemcpyDeviceToHost, h->st));
        if (bits) HIP_TRY(hipMemcpyAsync(bits, a.bits, sizeof(double) * streams, hipMemcpyDeviceToHost, h->st));
        if (trace && total) HIP_TRY(hipMemcpyAsync(trace, a.trace, sizeof(uint32_t) * 3 * total, hipMemcpyDeviceToHost, h->st));
        if (block_bits && n_block_bits)
            HIP_TRY(hipMemcpyAsync(block_bits, r.block_bits, sizeof(double) * n_block_bits, hipMemcpyDeviceToHost, h->st));
    }
    if (w_out) HIP_TRY(hipMemcpyAsync(w_out, a.v, sizeof(float) * (1 + r.gs.count) * streams, hipMemcpyDeviceToHost, h->st));
    if (w_trace && total)
        HIP_TRY(hipMemcpyAsync(w_trace, a.w_trace, sizeof(float) * (1 + r.gs.count) * total, hipMemcpyDeviceToHost, h->st));
    HIP_TRY(hipStreamSynchronize(h->st));
    if (err & CODE_ERR_TOTAL) return fail(LSTM_HIP_EINVAL, "%s: a frequency total passed 2^16 (the quantisation bound)", what);
    if (err & CODE_ERR_BOUND) return fail(LSTM_HIP_EINVAL, "%s: a code passed lstm_hip_code_bound", what);
    if (!decode) { // the codes back to back: move each down from its bound-sized range (memmove: ranges overlap in order)
        code_off_out[0] = 0;
        for (int s = 0; s < streams; s++) {
            if (len[s] > r.base[s + 1] - r.base[s]) return fail(LSTM_HIP_EINVAL, "encode: stream %d's code passed its bound", s);
            if (len[s]) memmove(code_out + code_off_out[s], code_out + r.base[s], len[s]);
            code_off_out[s + 1] = code_off_out[s] + len[s];
        }
    }
    return 0;
}
// the refusals the mixed calls add to the coders' own (include/lstm_hip.h); on success r holds the guides and the rate
static int mix_checks(lstm_hip_t *h, const char *what, const lstm_hip_guidance *gd, const lstm_hip_mix_coding *mx, const float *w_out,
                      const float *w_trace, CoderRun &r) {
    if (!gd) {
        if (mx) return fail(LSTM_HIP_EINVAL, "%s: mix coding given without guidance", what);
        if (w_out || w_trace) return fail(LSTM_HIP_EINVAL, "%s: w_out / w_trace given without guidance", what);
        return 0;
    }
    if (int rc = check_guidance(what, h, gd, r.gs)) return rc;
    for (int k = 0; k < gd->nguides; k++) {
        const lstm_hip_guide &u = gd->guides[k];
        if (u.h0 || u.c0 || u.h_out || u.c_out)
            return fail(LSTM_HIP_EINVAL, "%s: guide %d: h0, c0, h_out and c_out must be null (the coders start every model from zero)", what, k);
    }
    if (mx) {
        if (mx->size != sizeof(lstm_hip_mix_coding))
            return fail(LSTM_HIP_EINVAL, "%s: mix coding of %u bytes, expected %zu", what, mx->size, sizeof(lstm_hip_mix_coding));
        if (!std::isfinite(mx->rate) || mx->rate < 0.0) return fail(LSTM_HIP_EINVAL, "%s: rate must be finite and >= 0 (got %g)", what, mx->rate);
        r.rate = (float)mx->rate;
    }
    return 0;
}
static int run_coder(lstm_hip_t *h, bool decode, int32_t streams, const uint64_t *text_off, const uint8_t *text_in,
                     uint8_t *text_out, const uint8_t *code_in, const uint64_t *code_off_in, uint8_t *code_out,
                     uint64_t *code_off_out, double *bits, uint32_t *trace, const lstm_hip_guidance *gd = nullptr,
                     const lstm_hip_mix_coding *mx = nullptr, float *w_out = nullptr, float *w_trace = nullptr) {
    CoderRun r;
    if (int rc = mix_checks(h, decode ? "decode" : "encode", gd, mx, w_out, w_trace, r)) return rc;
    if (int rc = coder_begin(h, r, decode, streams, text_off, text_in, code_in, code_off_in, trace != nullptr, 0, gd, w_trace != nullptr))
        return rc;
    if (int rc = coder_steps(h, r, 0, r.max_len)) return rc;
    return coder_finish(h, r, text_out, code_out, code_off_out, bits, trace, nullptr, 0, w_out, w_trace);
}

int lstm_hip_encode(lstm_hip_t *h, int32_t streams, const uint8_t *text, const uint64_t *text_off, uint8_t *code,
                    uint64_t code_cap, uint64_t *code_off, double *bits, uint32_t *trace) {
    return lstm_hip_encode_mixed(h, streams, text, text_off, code, code_cap, code_off, bits, trace, nullptr, nullptr, nullptr, nullptr);
}

// The mixed coders.  The coders' own refusals first, then the guidance's and the mix coding's
// (mix_checks); with gd NULL every offset, upload and launch is lstm_hip_encode's / lstm_hip_decode's.
uint32_t lstm_hip_mix_coder_version(void) { return 1; }

int lstm_hip_encode_mixed(lstm_hip_t *h, int32_t streams, const uint8_t *text, const uint64_t *text_off, uint8_t *code,
                          uint64_t code_cap, uint64_t *code_off, double *bits, uint32_t *trace, const lstm_hip_guidance *gd,
                          const lstm_hip_mix_coding *mx, float *w_out, float *w_trace) {
    CHECK(h);
    if (streams < 1 || streams > 4096) return fail(LSTM_HIP_EINVAL, "encode: streams must be in [1, 4096] (got %d)", streams);
    if (int rc = check_offsets("encode", "text_off", text_off, streams)) return rc;
    if (!code_off) return fail(LSTM_HIP_EINVAL, "encode: null code_off");
    if (text_off[streams] > 0 && !text) return fail(LSTM_HIP_EINVAL, "encode: null text with %llu bytes to code", (unsigned long long)text_off[streams]);
    uint64_t need = 0;
    for (int s = 0; s < streams; s++) {
        const size_t b = lstm_hip_code_bound(text_off[s + 1] - text_off[s]);
        if (b == SIZE_MAX || need > UINT64_MAX - b) return fail(LSTM_HIP_EINVAL, "encode: text too long");
        need += b;
    }
    if (code_cap < need)
        return fail(LSTM_HIP_EINVAL, "encode: code_cap %llu is below the bound %llu (sum of lstm_hip_code_bound)",
                    (unsigned long long)code_cap, (unsigned long long)need);
    if (need > 0 && !code) return fail(LSTM_HIP_EINVAL, "encode: null code");
    if (h->cfg.N > 16384) return fail(LSTM_HIP_EINVAL, "encode: hidden width %d above 16384", h->cfg.N);
    return run_coder(h, false, streams, text_off, text, nullptr, nullptr, nullptr, code, code_off, bits, trace, gd, mx, w_out, w_trace);
}

int lstm_hip_decode(lstm_hip_t *h, int32_t streams, const uint8_t *code, const uint64_t *code_off, const uint64_t *text_off,
                    uint8_t *text) {
    return lstm_hip_decode_mixed(h, streams, code, code_off, text_off, text, nullptr, nullptr, nullptr);
}

int lstm_hip_decode_mixed(lstm_hip_t *h, int32_t streams, const uint8_t *code, const uint64_t *code_off, const uint64_t *text_off,
                          uint8_t *text, const lstm_hip_guidance *gd, const lstm_hip_mix_coding *mx, float *w_out) {
    CHECK(h);
    if (streams < 1 || streams > 4096) return fail(LSTM_HIP_EINVAL, "decode: streams must be in [1, 4096] (got %d)", streams);
    if (int rc = check_offsets("decode", "code_off", code_off, streams)) return rc;
    if (int rc = check_offsets("decode", "text_off", text_off, streams)) return rc;
    if (code_off[streams] > 0 && !code) return fail(LSTM_HIP_EINVAL, "decode: null code with %llu code bytes", (unsigned long long)code_off[streams]);
    if (text_off[streams] > 0 && !text) return fail(LSTM_HIP_EINVAL, "decode: null text with %llu bytes to decode", (unsigned long long)text_off[streams]);
    if (h->cfg.N > 16384) return fail(LSTM_HIP_EINVAL, "decode: hidden width %d above 16384", h->cfg.N);
    return run_coder(h, true, streams, text_off, nullptr, text, code, code_off, nullptr, nullptr, nullptr, nullptr, gd, mx, w_out, nullptr);
}

// ---- adaptive coding: the model trains on the bytes it has coded (include/lstm_hip.h)
uint32_t lstm_hip_adaptive_version(void) { return 1; }

int64_t lstm_hip_adaptive_blocks(int32_t S, int32_t B, const uint64_t *text_off) {
    if (S < 2 || B < 1) return fail(LSTM_HIP_EINVAL, "adaptive_blocks: need S >= 2 and B >= 1 (got %d, %d)", S, B);
    if (int rc = check_offsets("adaptive_blocks", "text_off", text_off, B)) return rc;
    uint64_t shortest = UINT64_MAX;
    for (int s = 0; s < B; s++) shortest = std::min<uint64_t>(shortest, text_off[s + 1] - text_off[s]);
    return (int64_t)(shortest / (uint64_t)(S - 1));
}

int lstm_hip_plan_identity(lstm_hip_t *h, char *buf, size_t cap) {
    if (!h || !buf || cap == 0) return fail(LSTM_HIP_EINVAL, "plan_identity: null handle or buffer");
    const EnginePlan &p = h->plan;
    const int n = snprintf(buf, cap, "np%d fwd%d bwd%d fused%d bc%d gp%d fc%d lc%d gc%d quad%d dusplit%d side%d dgt%d sw%d su%d", h->cfg.N,
                           (int)p.fwd, (int)p.bwd, (int)p.fused, p.bwd_cols, p.gpart_cols, p.fwd_cols, p.launch_cols, p.group_cols,
                           (int)p.adagrad_quad, (int)p.du_split, (int)p.side_stream, (int)p.direct_dgt, h->splits_dWhy, h->splits_dU);
    if (n < 0 || (size_t)n >= cap) return fail(LSTM_HIP_EINVAL, "plan_identity: the buffer needs %d bytes", n + 1);
    return 0;
}

// Both adaptive calls.  Per block: the code pass (coder_steps: the image of U remade from the current P, then the static
// coder's steps), block_window (the block's training window from the coder's text buffer, the carry, the bit fold), then one
// window of the training loop exactly as lstm_hip_train_windows runs it, without a slide riding in the update launch (the
// next block's bytes do not exist yet in the decoder).  The tail is coded only.
static int run_adaptive(lstm_hip_t *h, bool decode, const uint64_t *text_off, const uint8_t *text_in, uint8_t *text_out,
                        const uint8_t *code_in, const uint64_t *code_off_in, uint8_t *code_out, uint64_t *code_off_out, double lr,
                        double *bits, double *block_bits, uint32_t *trace) {
    const int S = h->cfg.S, B = h->cfg.B, N = h->cfg.N;
    const uint64_t L = (uint64_t)(S - 1);
    const int64_t n_blocks = lstm_hip_adaptive_blocks(S, B, text_off);
    if (n_blocks < 0) return (int)n_blocks;
    if (int rc = ensure_losses(h, n_blocks)) return rc;
    h->norms_n = -1;
    h->call_updates = 0;
    h->pre_slid = false;
    const bool clip = h->clip_max > 0.0;
    if (clip)
        if (int rc = ensure_norms(h, n_blocks)) return rc;
    // reset: empty window, zero states
    if (int rc = lstm_hip_reset_window(h)) return rc;
    HIP_TRY(hipMemsetAsync(h->H, 0, sizeof(float) * (size_t)S * N * B, h->st));
    HIP_TRY(hipMemsetAsync(h->C, 0, sizeof(float) * (size_t)S * N * B, h->st));
    CoderRun r;
    const int64_t n_bb = decode ? 0 : n_blocks + 1;
    if (int rc = coder_begin(h, r, decode, B, text_off, text_in, code_in, code_off_in, trace != nullptr, n_bb)) return rc;
    BlockWindowArgs w{};
    w.text = r.a.text, w.text_off = r.a.text_off;
    w.xi = h->xi, w.ti = h->ti, w.Xr = h->Xr, w.Tr = h->Tr, w.head = h->head;
    w.H = h->H, w.C = h->C;
    w.bits = r.a.bits, w.bits_prev = r.bits_prev;
    w.S = S, w.B = B, w.NB4 = N * B / 4;
    h->in_loop = true;
    LoopGuard guard{h};
    for (int64_t k = 0; k < n_blocks; k++) {
        int rc = 0;
        if ((rc = coder_steps(h, r, (uint64_t)k * L, (uint64_t)(k + 1) * L))) return rc;
        w.k = k, w.build = 1, w.block_bits = decode ? nullptr : r.block_bits + k;
        RUN(K_BLOCK_WINDOW, block_window(w, h->plan.n_cus, h->st));
        const bool own_loss = loop_window(h, k + 1 == n_blocks, h->d_losses + k);
        if ((rc = do_forward(h))) return rc;
        if (own_loss)
            RUN(K_LOSS, loss_reduce(loss_src(h), loss_steps(h), B, h->global_B, h->d_losses + k, h->dby_part, h->n_dby_parts,
                                    h->dP + h->pl.by, h->st, loss_scale(h)));
        h->dby_done = true;
        if ((rc = do_backward(h))) return rc;
        h->carry_slide = false;
        if ((rc = do_adagrad(h, lr, h->call_updates))) return rc;
    }
    if (int rc = coder_steps(h, r, (uint64_t)n_blocks * L, r.max_len)) return rc;
    if (!decode) {
        w.k = n_blocks, w.build = 0, w.block_bits = r.block_bits + n_blocks;
        RUN(K_BLOCK_WINDOW, block_window(w, h->plan.n_cus, h->st));
    }
    const int rc = coder_finish(h, r, text_out, code_out, code_off_out, bits, trace, block_bits, n_bb);
    if (int ab = check_abort(h)) return ab;
    if (rc) return rc;
    guard.completed = true;
    if (clip) h->norms_n = n_blocks;
    return 0;
}

static int adaptive_checks(lstm_hip_t *h, const char *what, double lr) {
    if (h->comm) return fail(LSTM_HIP_ESTATE, "%s: a handle with a communicator cannot code adaptively", what);
    if (h->infer_src == LSTM_HIP_SRC_AVERAGE) // (it codes with the model it trains: the setting cannot be honoured)
        return fail(LSTM_HIP_ESTATE, "%s: the inference source is LSTM_HIP_SRC_AVERAGE; adaptive coding reads the parameters it trains", what);
    if (h->soft_on) // (the decoder would need the teacher and the settings: the containers record neither)
        return fail(LSTM_HIP_ESTATE, "%s: soft targets are on (lstm_hip_set_soft_targets); the adaptive coders train on hard targets", what);
    if (h->wd_rate > 0.0) // (the containers record no mask: DESIGN.md section 3.15)
        return fail(LSTM_HIP_ESTATE, "%s: weight drop is on (lstm_hip_set_weight_drop); the adaptive coders train without it", what);
    if (h->acc_every > 1) // (the containers record no K)
        return fail(LSTM_HIP_ESTATE, "%s: gradient accumulation is on (lstm_hip_set_grad_accumulation); the adaptive coders update after every block", what);
    if (!std::isfinite(lr) || lr < 0.0) return fail(LSTM_HIP_EINVAL, "%s: learning_rate must be finite and >= 0 (got %g)", what, lr);
    if (h->cfg.N > 16384) return fail(LSTM_HIP_EINVAL, "%s: hidden width %d above 16384", what, h->cfg.N);
    if (h->cfg.B > 4096) return fail(LSTM_HIP_EINVAL, "%s: more than 4096 streams (B = %d)", what, h->cfg.B);
    return 0;
}

int lstm_hip_encode_adaptive(lstm_hip_t *h, const uint8_t *text, const uint64_t *text_off, double learning_rate, uint8_t *code,
                             uint64_t code_cap, uint64_t *code_off, double *bits, double *block_bits, uint32_t *trace) {
    CHECK(h);
    const char *what = "encode_adaptive";
    if (int rc = adaptive_checks(h, what, learning_rate)) return rc;
    const int32_t streams = h->cfg.B;
    if (int rc = check_offsets(what, "text_off", text_off, streams)) return rc;
    if (!code_off) return fail(LSTM_HIP_EINVAL, "%s: null code_off", what);
    if (text_off[streams] > 0 && !text) return fail(LSTM_HIP_EINVAL, "%s: null text with %llu bytes to code", what, (unsigned long long)text_off[streams]);
    uint64_t need = 0;
    for (int s = 0; s < streams; s++) {
        const size_t b = lstm_hip_code_bound(text_off[s + 1] - text_off[s]);
        if (b == SIZE_MAX || need > UINT64_MAX - b) return fail(LSTM_HIP_EINVAL, "%s: text too long", what);
        need += b;
    }
    if (code_cap < need)
        return fail(LSTM_HIP_EINVAL, "%s: code_cap %llu is below the bound %llu (sum of lstm_hip_code_bound)", what,
                    (unsigned long long)code_cap, (unsigned long long)need);
    if (need > 0 && !code) return fail(LSTM_HIP_EINVAL, "%s: null code", what);
    return run_adaptive(h, false, text_off, text, nullptr, nullptr, nullptr, code, code_off, learning_rate, bits, block_bits, trace);
}

int lstm_hip_decode_adaptive(lstm_hip_t *h, const uint8_t *code, const uint64_t *code_off, const uint64_t *text_off,
                             double learning_rate, uint8_t *text) {
    CHECK(h);
    const char *what = "decode_adaptive";
    if (int rc = adaptive_checks(h, what, learning_rate)) return rc;
    const int32_t streams = h->cfg.B;
    if (int rc = check_offsets(what, "code_off", code_off, streams)) return rc;
    if (int rc = check_offsets(what, "text_off", text_off, streams)) return rc;
    if (code_off[streams] > 0 && !code) return fail(LSTM_HIP_EINVAL, "%s: null code with %llu code bytes", what, (unsigned long long)code_off[streams]);
    if (text_off[streams] > 0 && !text) return fail(LSTM_HIP_EINVAL, "%s: null text with %llu bytes to decode", what, (unsigned long long)text_off[streams]);
    return run_adaptive(h, true, text_off, nullptr, text, code, code_off, nullptr, nullptr, learning_rate, nullptr, nullptr, nullptr);
}

// Training on separate texts (include/lstm_hip.h).  set: the texts, their offsets and the tables of
// the plan go to the device once and stay with the handle.  train: per window text_window (indices, rings, carry or zero
// state), the handle's own forward path with the softmax launch in its text form, text_fold (the streams' bits), then the
// adaptive train pass's sequence -- loss, backward, clip, update, no slide riding in the update launch.
// Weighted texts (lstm_hip_set_train_texts_weighted, section 3.20): a float per byte goes up with the texts; text_window then
// writes the window's weights beside ti and do_forward launches the softmax's weighted form.  Nothing else differs, and the
// unweighted set is the weighted one with weight = NULL.
static int drop_train_texts(lstm_hip_ctx *h) {
    HIP_TRY(hipStreamSynchronize(h->st));
    DeviceMem &m = h->own;
    TRY(m.release(h->tt_text));
    TRY(m.release(h->tt_off));
    TRY(m.release(h->tt_slot));
    TRY(m.release(h->tt_first));
    TRY(m.release(h->tt_bits));
    TRY(m.release(h->tt_weight));
    TRY(m.release(h->tt_wt));
    h->tt_streams = 0;
    h->tt_windows = h->tt_next = 0;
    return 0;
}
int lstm_hip_set_train_texts(lstm_hip_t *h, int32_t streams, const uint8_t *text, const uint64_t *text_off) {
    return lstm_hip_set_train_texts_weighted(h, streams, text, text_off, nullptr);
}
int lstm_hip_set_train_texts_weighted(lstm_hip_t *h, int32_t streams, const uint8_t *text, const uint64_t *text_off,
                                      const float *weight) {
    CHECK(h);
    if (streams == 0 && !text && !text_off && !weight) return drop_train_texts(h);
    std::vector<int32_t> slot;
    std::vector<int64_t> first(streams > 0 ? streams : 0);
    const int64_t windows = checked_plan("set_train_texts", h->cfg.S - 1, h->cfg.B, streams, text_off, nullptr, first.data(), &slot);
    if (windows < 0) return (int)windows;
    const uint64_t total = text_off[streams];
    if (total > 0 && !text) return fail(LSTM_HIP_EINVAL, "set_train_texts: null text with %llu bytes to read", (unsigned long long)total);
    if (weight)
        for (int32_t s = 0; s < streams; s++)
            for (uint64_t i = text_off[s]; i < text_off[s + 1]; i++)
                if (!(weight[i] >= 0.0f) || std::isinf(weight[i]))
                    return fail(LSTM_HIP_EINVAL, "set_train_texts_weighted: the weight of byte %llu of stream %d is %g; a weight must be finite and >= 0",
                                (unsigned long long)(i - text_off[s]), s, (double)weight[i]);
    if (int rc = drop_train_texts(h)) return rc;
    // (at least one element each, so that a set plan always has its five buffers)
    DeviceMem &m = h->own;
    TRY(m.alloc(h->tt_text, total ? total : 1, DeviceMem::kNoFill));
    TRY(m.alloc(h->tt_off, (size_t)streams + 1, DeviceMem::kNoFill));
    TRY(m.alloc(h->tt_slot, slot.empty() ? 1 : slot.size(), DeviceMem::kNoFill));
    TRY(m.alloc(h->tt_first, streams, DeviceMem::kNoFill));
    TRY(m.alloc(h->tt_bits, streams, 0));
    if (total) HIP_TRY(hipMemcpy(h->tt_text, text, total, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->tt_off, text_off, sizeof(uint64_t) * (streams + 1), hipMemcpyHostToDevice));
    if (!slot.empty()) HIP_TRY(hipMemcpy(h->tt_slot, slot.data(), sizeof(int32_t) * slot.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->tt_first, first.data(), sizeof(int64_t) * streams, hipMemcpyHostToDevice));
    if (weight) {
        TRY(m.alloc(h->tt_weight, total ? total : 1, DeviceMem::kNoFill));
        TRY(m.alloc(h->tt_wt, (size_t)h->cfg.S * h->cfg.B, 0));
        if (total) HIP_TRY(hipMemcpy(h->tt_weight, weight, sizeof(float) * total, hipMemcpyHostToDevice));
    }
    h->tt_streams = streams;
    h->tt_windows = windows;
    h->tt_next = 0;
    return 0;
}
int lstm_hip_get_train_texts(lstm_hip_t *h, int64_t *windows, int64_t *next) {
    if (!h) return fail(LSTM_HIP_EINVAL, "null handle");
    if (h->tt_streams == 0) return fail(LSTM_HIP_ESTATE, "get_train_texts before set_train_texts");
    if (windows) *windows = h->tt_windows;
    if (next) *next = h->tt_next;
    return 0;
}
int lstm_hip_get_train_texts_bits(lstm_hip_t *h, double *bits) {
    CHECK(h);
    if (h->tt_streams == 0) return fail(LSTM_HIP_ESTATE, "get_train_texts_bits before set_train_texts");
    if (!bits) return fail(LSTM_HIP_EINVAL, "get_train_texts_bits: null pointer");
    HIP_TRY(hipMemcpyAsync(bits, h->tt_bits, sizeof(double) * h->tt_streams, hipMemcpyDeviceToHost, h->st));
    HIP_TRY(hipStreamSynchronize(h->st));
    return 0;
}
int lstm_hip_train_text_windows(lstm_hip_t *h, int64_t count, double learning_rate, double *losses, float *elapsed_ms) {
    CHECK(h);
    if (h->tt_streams == 0) return fail(LSTM_HIP_ESTATE, "train_text_windows before set_train_texts");
    if (count < 0 || count > h->tt_windows - h->tt_next)
        return fail(LSTM_HIP_EINVAL, "train_text_windows: count %lld outside [0, %lld] (the plan has %lld windows, the next is %lld)",
                    (long long)count, (long long)(h->tt_windows - h->tt_next), (long long)h->tt_windows, (long long)h->tt_next);
    if (!std::isfinite(learning_rate) || learning_rate < 0.0)
        return fail(LSTM_HIP_EINVAL, "train_text_windows: learning_rate must be finite and >= 0 (got %g)", learning_rate);
    if (h->comm) return fail(LSTM_HIP_ESTATE, "train_text_windows: a handle with a communicator cannot train on separate texts");
    if (h->soft_on)
        return fail(LSTM_HIP_ESTATE, "train_text_windows: soft targets are on (lstm_hip_set_soft_targets); the text windows train on hard targets");
    if (h->loss_mode != LSTM_HIP_LOSS_ALL_STEPS_BITS)
        return fail(LSTM_HIP_ESTATE, "train_text_windows: the loss mode is %d; the text windows report LSTM_HIP_LOSS_ALL_STEPS_BITS only",
                    h->loss_mode);
    if (int rc = ensure_losses(h, count)) return rc;
    h->norms_n = -1;
    h->call_updates = 0;
    h->pre_slid = false;
    const bool clip = h->clip_max > 0.0;
    if (clip)
        if (int rc = ensure_norms(h, count)) return rc;
    const int B = h->cfg.B;
    TextWindowArgs a{};
    a.text = h->tt_text, a.off = h->tt_off, a.slot = h->tt_slot, a.first = h->tt_first;
    a.xi = h->xi, a.ti = h->ti, a.Xr = h->Xr, a.Tr = h->Tr, a.head = h->head;
    a.H = h->H, a.C = h->C;
    a.colloss = h->colloss, a.bits = h->tt_bits;
    a.S = h->cfg.S, a.B = B, a.N = h->cfg.N;
    a.weight = h->tt_weight, a.wt = h->tt_wt; // (both null on unweighted texts)
    if (elapsed_ms) HIP_TRY(hipEventRecord(h->evt0, h->st));
    h->in_loop = true;
    LoopGuard guard{h};
    struct TextMode { // the softmax launch is back in its own form on every return path
        lstm_hip_ctx *h;
        ~TextMode() { h->text_window = false; }
    } text_mode{h};
    h->text_window = true;
    for (int64_t i = 0; i < count; i++) {
        int rc = 0;
        RUN(K_TEXT_WINDOW, text_window(a, h->tt_next, h->plan.n_cus, h->st));
        const bool own_loss = loop_window(h, i + 1 == count, h->d_losses + i);
        if ((rc = do_forward(h))) return rc;
        RUN(K_TEXT_FOLD, text_fold(a, h->tt_next, h->plan.n_cus, h->st));
        if (own_loss)
            RUN(K_LOSS, loss_reduce(loss_src(h), loss_steps(h), B, h->global_B, h->d_losses + i, h->dby_part, h->n_dby_parts,
                                    h->dP + h->pl.by, h->st, loss_scale(h)));
        h->dby_done = true;
        if ((rc = do_backward(h))) return rc;
        h->carry_slide = false;
        if ((rc = do_adagrad(h, learning_rate, h->call_updates))) return rc;
        h->tt_next++;
    }
    if (elapsed_ms) {
        HIP_TRY(hipEventRecord(h->evt1, h->st));
        HIP_TRY(hipEventSynchronize(h->evt1));
        HIP_TRY(hipEventElapsedTime(elapsed_ms, h->evt0, h->evt1));
    }
    if (losses && count > 0)
        HIP_TRY(hipMemcpyAsync(h->h_losses, h->d_losses, sizeof(double) * count, hipMemcpyDeviceToHost, h->st));
    HIP_TRY(hipStreamSynchronize(h->st));
    if (losses && count > 0) std::memcpy(losses, h->h_losses, sizeof(double) * count);
    guard.completed = true;
    if (clip) h->norms_n = h->call_updates;
    return check_abort(h);
}

int lstm_hip_debug_stamps(lstm_hip_t *h, uint64_t *out, size_t count) {
    CHECK(h);
    if (!h->stamps) return fail(LSTM_HIP_ESTATE, "handle was not created with LSTM_HIP_DEBUG_STAMPS on a shape whose two-half forms carry stamps (fp32: hidden 512; bf16: any)");
    const size_t have = (size_t)4 * h->cfg.S * 16;
    HIP_TRY(hipMemcpyAsync(out, h->stamps, sizeof(uint64_t) * (count < have ? count : have), hipMemcpyDeviceToHost, h->st));
    HIP_TRY(hipStreamSynchronize(h->st));
    return 0;
}

int lstm_hip_synchronize(lstm_hip_t *h) {
    CHECK(h);
    HIP_TRY(hipStreamSynchronize(h->st));
    return check_abort(h);
}
int lstm_hip_set_profiling(lstm_hip_t *h, int32_t on) {
    if (!h) return fail(LSTM_HIP_EINVAL, "null handle");
    h->profiling = on != 0;
    return 0;
}
// the kernels' rows and, behind them, one row that is no kernel: "counter_resets", the times a recurrence cleared its hand-off
// counters (do_forward / do_backward), counted whether or not profiling is on; its time is 0
int lstm_hip_kernel_stat_count(lstm_hip_t *) { return K_COUNT + 1; }
int lstm_hip_kernel_stat(lstm_hip_t *h, int32_t idx, const char **name, int64_t *launches, double *total_ms) {
    if (!h || idx < 0 || idx > K_COUNT) return fail(LSTM_HIP_EINVAL, "kernel_stat: bad index %d", idx);
    if (idx == K_COUNT) {
        if (name) *name = "counter_resets";
        if (launches) *launches = h->counter_resets;
        if (total_ms) *total_ms = 0.0;
        return 0;
    }
    if (name) *name = kernel_name(idx);
    if (launches) *launches = h->launches[idx];
    if (total_ms) *total_ms = h->total_ms[idx];
    return 0;
}
int lstm_hip_reset_kernel_stats(lstm_hip_t *h) {
    if (!h) return fail(LSTM_HIP_EINVAL, "null handle");
    memset(h->launches, 0, sizeof(h->launches));
    memset(h->total_ms, 0, sizeof(h->total_ms));
    h->counter_resets = 0;
    return 0;
}

} // extern "C"
