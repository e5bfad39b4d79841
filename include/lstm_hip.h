/*
 * lstm_hip.h -- C ABI of the MI355X (gfx950) LSTM forward/BPTT/Adagrad path.
 *
 * This is the drop-in boundary for the hot path of krocki/Eigen-LSTM.  The reference has exactly
 * one host<->device seam: the twelve `#ifdef __GPU__` sites of
 * OV/lstm_eigen_class_CUDA/lstm.cc (50,107,156,192,273,316,328,335,362,374,379,389), which talk to
 * the device through cuParameters / cuLSTM<S> / cuda_adagrad and six copy helpers
 * (OV/lstm_eigen_class_CUDA/cu_lstm.h).  Every entry point below names the member it replaces
 * (OV/ = /root/reference/optimized-obsfuscated_versions).  Plain pointers and sizes only; no C++ or
 * torch types.  All matrices are column-major fp32, as Eigen's MatrixXf::data() is
 * (cu_matrix.cu:93-101 copies it verbatim).
 *
 * Differences from the reference seam, on purpose:
 *   - one-hot matrices x[t], target[t] (M x B floats each) cross the boundary as int32 indices
 *     [S x B]; index < 0 is the all-zero column (OV/lstm_eigen_opt/lstm.cc:122,125);
 *   - the five parameter tensors travel as ONE flat block [W | U | b | Why | by] (also the RCCL
 *     all-reduce payload);
 *   - errors are returned (0 = ok, <0 = LSTM_HIP_E*), never printed-and-ignored
 *     (cu_matrix.cu:16-19,159-162); lstm_hip_last_error() gives the text;
 *   - the whole i-loop body can run on the device (lstm_hip_train_windows) so nothing is copied
 *     per iteration (the reference moves 7*S matrices each way, lstm.cc:274,317,375).
 *
 * Thread-safety: a handle is used by one host thread at a time; different handles are independent.
 */
#ifndef LSTM_HIP_H_
#define LSTM_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSTM_HIP_OK 0
#define LSTM_HIP_EINVAL (-1)   /* bad argument / unsupported shape */
#define LSTM_HIP_EHIP (-2)     /* a HIP runtime call failed */
#define LSTM_HIP_ENODEV (-3)   /* no usable gfx950 device */
#define LSTM_HIP_ERCCL (-4)    /* RCCL missing or a collective failed */
#define LSTM_HIP_ESTATE (-5)   /* call sequence error (e.g. backward before forward) */

#define LSTM_HIP_VOCAB 256     /* M: raw bytes, R/lstm.cc:55 */

/* flags for lstm_hip_config.flags */
#define LSTM_HIP_FAST_MATH 1u      /* v_exp/v_rcp based sigmoid/tanh (the reference's --use_fast_math build,
                                      OV/lstm_eigen_class_CUDA/Makefile:53-66); default is libm-accurate */
                                   /* (bits 2u, 8u, 32u: flags of earlier versions, now ignored) */
#define LSTM_HIP_STEP_KERNELS 4u   /* one launch per timestep (baseline engine) instead of the persistent
                                      recurrence kernels */

#define LSTM_HIP_BF16_RECURRENCE 128u /* the bf16 MFMA path (BASELINE configs[4]): bf16 operands, fp32 accumulate, in the two
                                      recurrent products (U, and the h / dg hand-off) and in the four time-batched ones
                                      (Why*h, Why^T*dy, dy*h^T, dg*h^T); fp32 master weights, biases, elementwise math,
                                      dW/db/dby and Adagrad.  Needs N % 128 == 0, N <= 1024, B % 8 == 0 */
#define LSTM_HIP_NO_FUSED_GRADS 64u  /* compute dU/dW/db after the backward recurrence (GEMM + sorted segment sums)
                                      instead of accumulating them inside it */
#define LSTM_HIP_DEBUG_STAMPS 16u    /* diagnostic builds of both recurrences (N = 512, 8-column forms) that record
                                      s_memtime at marked points of every step; see lstm_hip_debug_stamps */
#define LSTM_HIP_PAD_HIDDEN 256u     /* accept any N >= 1 and run it at an internal width Np >= N whose extra hidden units
                                      have all-zero rows and columns in W, U, b and Why (exact: such a unit keeps c = h = 0
                                      and gets zero gradients).  Np depends on N and the flags only:
                                        fp32, N <= 64 or N > 1024:       N rounded up to 16
                                        fp32, 64 < N <= 1024, N % 64 = 0: N
                                        fp32, other 64 < N <= 1024:      the smallest of 128, 256, 512, 1024 >= N
                                        LSTM_HIP_BF16_RECURRENCE:        N rounded up to 128 (refused above 1024)
                                        LSTM_HIP_STEP_KERNELS:           N rounded up to 16
                                      Every call still takes and returns logical-N shapes; only the RCCL all-reduce
                                      payload is the padded block (lstm_hip_param_count(Np, M) floats). */
#define LSTM_HIP_STABLE_SOFTMAX 512u /* max-shifted output layer, for logits past expf's range (about 88).  Per column
                                      (one stream at one step), with z = Why*h + by and zmax = max_m z_m:
                                        p_m = expf(z_m - zmax) / s,  s = sum_m expf(z_m - zmax)
                                        surprisal = log2f(s) + (zmax - z_target) * log2(e)  (finite where p_target
                                                    underflows to 0; 0 for an empty target, as without the flag)
                                      dy = p - onehot, the loss modes, the /B and dby are defined on these as without
                                      the flag.  Training, lstm_hip_eval_bits, lstm_hip_sample and the temperature-1 draws
                                      and prompt bits of lstm_hip_generate all use it (tempered and greedy draws are
                                      unchanged).  Fixed at create; combines with every other flag.  Default: the
                                      reference's unshifted softmax (R/lstm.cc:195-204). */

typedef struct lstm_hip_ctx lstm_hip_t; /* opaque: cuParameters p,d,m + cuLSTM<S> in one object */

typedef struct lstm_hip_config {
    int32_t N;       /* hidden size: a multiple of 16, or any N >= 1 with LSTM_HIP_PAD_HIDDEN   R/lstm.cc:53 */
    int32_t M;       /* vocabulary, must be LSTM_HIP_VOCAB                R/lstm.cc:55 */
    int32_t S;       /* window columns; S-1 timesteps per window, S >= 2  R/lstm.cc:57 */
    int32_t B;       /* concurrent streams on THIS device                 OV/lstm_eigen_opt/lstm.cc:56 */
    int32_t device;  /* HIP device ordinal (reference: cudaSetDevice(4), lstm.cc:51) */
    uint32_t flags;  /* LSTM_HIP_* */
} lstm_hip_config;

/* ---- lifetime: cuParameters(M,N) x3 + cuLSTM<S>(M,N,B) ctor/dtor, cu_lstm.h:24-42,83-144;
 *      init_cublas/teardown_cublas, lstm.cc:50-54,389-391.  Parameters, gradients, Adagrad memory
 *      and all window state start zeroed (cuParameters::zero, cuLSTM::reset). */
int lstm_hip_create(const lstm_hip_config *cfg, lstm_hip_t **out);
int lstm_hip_destroy(lstm_hip_t *h);
const char *lstm_hip_last_error(void);
/* number of floats in the flat block: 4N*M + 4N*N + 4N + M*N + M (logical N: the size every call below takes) */
size_t lstm_hip_param_count(int32_t N, int32_t M);

/* ---- copy_parameters_to_device / copy_parameters_to_host, cu_lstm.h:307-325.
 *      `which`: 0 = parameters p, 1 = gradients d, 2 = Adagrad memory m (Adam: first moment), 3 = Adam's second moment
 *      (lstm_hip_set_optimizer).  Host block layout
 *      [W (4N x M) | U (4N x N) | b (4N) | Why (M x N) | by (M)], each column-major. */
int lstm_hip_set_params(lstm_hip_t *h, int which, const float *host_block);
int lstm_hip_get_params(lstm_hip_t *h, int which, float *host_block);

/* ---- copy_lstm_to_device / copy_lstm_to_host / copy_context_to_host, cu_lstm.h:337-396.
 *      State column t (0 <= t < S) of h and c, each N x B column-major.  Either pointer may be NULL. */
int lstm_hip_set_state(lstm_hip_t *h, int32_t t, const float *h_t, const float *c_t);
int lstm_hip_get_state(lstm_hip_t *h, int32_t t, float *h_t, float *c_t);
/* g[t] (4N x B, post-activation gates [i;o;f;u]) and probs[t] (M x B); t in [1,S).  NULL = skip.
 * For lock-step comparison (compare_lstm_states, cu_lstm.h:398-415). */
int lstm_hip_get_activations(lstm_hip_t *h, int32_t t, float *g_t, float *probs_t);

/* ---- copy_inputs_to_device, cu_lstm.h:364-377: the window's inputs and targets as indices,
 *      xi[t*B+b], ti[t*B+b], t in [0,S) (row 0 is never read, as in the reference). */
int lstm_hip_set_window(lstm_hip_t *h, const int32_t *xi, const int32_t *ti);
/* the same call with the reference's own operands: h[0], c[0] (N x B each, may be NULL = leave as is) and the dense one-hot
 * matrices x[t], target[t] (M x B each, column-major, t = 0..S-1 back to back: S*B columns of M floats).  Every column must
 * be all-zero or exactly one 1.0f among zeros (what the reference's encoder produces, R/lstm.cc:169-170,
 * OV/lstm_eigen_opt/lstm.cc:199-212); anything else is LSTM_HIP_EINVAL.  For bit-faithful lock-step tests against code
 * that holds the dense form. */
int lstm_hip_set_inputs_dense(lstm_hip_t *h, const float *h0, const float *c0, const float *x, const float *target);
/* the device-side part of the slide (OV/lstm_eigen_opt/lstm.cc:205-206): h[0] <- h[1], c[0] <- c[1] */
int lstm_hip_slide_state(lstm_hip_t *h);

/* ---- cuLSTM::forward, cu_lstm.h:162-201 (R/lstm.cc:173-201): t = 1..S-1 */
int lstm_hip_forward(lstm_hip_t *h);
/* ---- cuLSTM::calculate_loss, cu_lstm.h:203-215, with the root file's semantics (every step
 *      counts, R/lstm.cc:204-207; /B per OV/lstm_eigen_opt/lstm.cc:249): sum_t (sum_b -log2 p)/B */
int lstm_hip_loss(lstm_hip_t *h, double *loss_bits);
/* ---- cuLSTM::backward, cu_lstm.h:216-275 (R/lstm.cc:214-257): zero d, BPTT t = S-1..1 */
int lstm_hip_backward(lstm_hip_t *h);
/* ---- cuda_adagrad, cu_lstm.h:417-432 (R/lstm.cc:261-272): m += d.*d; p -= lr*d./sqrt(m+1e-10) */
int lstm_hip_adagrad(lstm_hip_t *h, double learning_rate);

/* ---- global-norm gradient clipping before every Adagrad step (lstm_hip_adagrad and each window of lstm_hip_train_windows)
 *   max_norm == 0      off (the default; nothing is computed, every path is the one without clipping)
 *   max_norm  > 0      norm = sqrt(sum of d^2 over the whole flat gradient block [dW|dU|db|dWhy|dby]), taken after the
 *                      all-reduce when there is a communicator; coef = max_norm / (norm + 1e-6) computed in double and
 *                      narrowed to float; when coef < 1 the step uses d' = d * coef (fp32) in place of d:
 *                      m += d'^2; p -= lr * d' / sqrt(m + 1e-10).  +INFINITY: measure only, never scale.
 *                      A non-finite norm is recorded as is and the step is unscaled (it behaves as without clipping).
 *   negative or NaN    LSTM_HIP_EINVAL
 * The squares are summed in double in one fixed order over flat-block indices, so the norm depends
 * only on the values of the summed block: bit-identical across engines' fold and plain paths and across ranks.  A padded
 * handle (LSTM_HIP_PAD_HIDDEN) sums its padded block, whose padding entries are 0.  The gradient block (lstm_hip_get_params
 * which=1) keeps the unclipped d.  Per handle, may change between calls, not part of checkpoints. */
int lstm_hip_set_grad_clip(lstm_hip_t *h, double max_norm);
/* the pre-clip norms of the Adagrad steps of the last lstm_hip_adagrad (1) or lstm_hip_train_windows (count) call,
 * oldest first; n <= that number (else LSTM_HIP_EINVAL); LSTM_HIP_ESTATE when clipping was off for that call.  Under
 * gradient accumulation (below) a call records one norm per UPDATE it made, possibly none. */
int lstm_hip_get_grad_norms(lstm_hip_t *h, double *norms, int64_t n);

/* ---- gradient accumulation: one update per `every` training windows
 *   every == 1   off (the default): no block, no counter, no launch; mean must still be 0 or 1
 *   every >= 2   on; mean = 0 keeps the sum of the windows' gradients, mean = 1 divides it by every
 *   anything else is LSTM_HIP_EINVAL, the message names the number and the handle stays usable.
 * A micro-window is every place an update is made today: lstm_hip_adagrad, each window of lstm_hip_train_windows and of
 * lstm_hip_train_text_windows.  Let g be the window's gradient block, summed from its pieces in the order the handle uses
 * without accumulation.  The handle keeps an fp32 block acc and a count pending in 0 .. every - 1:
 *   pending + 1 < every    acc = g when pending == 0 (an exact copy), else acc = acc + g (one fp32 add per element);
 *                          pending += 1.  No update: parameters, optimizer state and step count, averaging counts, the
 *                          weight-drop index t and every image of the weights stay as they are, and the call's learning rate
 *                          is not read.  lstm_hip_get_params(which = 1) returns this window's own g.
 *   pending + 1 == every   d = acc + g; with mean, d = d * (float)(1.0 / every): a second, separately rounded fp32 operation
 *                          with the factor computed in double on the host, no fused multiply-add.  d goes to the gradient
 *                          block (which = 1 returns it, unclipped) and the update runs on d exactly as a plain window's runs
 *                          on its gradient: the clip norm is taken on d, the step uses this call's learning rate, Adam's t,
 *                          the averaging count `seen` and the weight-drop index t advance by one.  pending = 0.
 * (NumPy's (acc + g) * np.float32(1.0 / every) on float32 arrays is bit for bit the same.)  Non-finite values propagate as
 * they are.  acc and pending live with the handle across calls: how a run is cut into lstm_hip_train_windows,
 * lstm_hip_train_text_windows and lstm_hip_adagrad calls shows in no result.  Losses, the teacher's KL and the text windows'
 * per-stream bits stay per window; lstm_hip_get_grad_norms returns one norm per update.  Under weight drop one mask lasts
 * the `every` windows of a cycle.  A LSTM_HIP_PAD_HIDDEN handle keeps acc at the internal width with zero padding.
 * State: a different (every, mean) pair, off included, discards what is pending (pending = 0); the same pair again keeps it.
 * lstm_hip_get_grad_accumulator / lstm_hip_set_grad_accumulator move acc as lstm_hip_get_params / lstm_hip_set_params move
 * their blocks (logical-N flat block; with pending == 0 get returns the zero block: nothing is summed); set needs
 * 0 <= pending < every (else LSTM_HIP_EINVAL) and exists for resuming, in this order: lstm_hip_set_grad_accumulation,
 * lstm_hip_set_grad_accumulator.  Both answer LSTM_HIP_ESTATE while accumulation is off; the four answer LSTM_HIP_EINVAL for
 * a null pointer.  Accumulation runs on one device: turning it on with a communicator on the handle, and
 * lstm_hip_comm_init while it is on, are LSTM_HIP_ESTATE; so are the adaptive coders while it is on (their containers
 * record no `every`).  Per handle, may change between calls, not part of the engine plan; a handle that never turns it on
 * makes the launches it made before this call existed. */
int lstm_hip_set_grad_accumulation(lstm_hip_t *h, int32_t every, int32_t mean);
int lstm_hip_get_grad_accumulation(lstm_hip_t *h, int32_t *every, int32_t *mean, int32_t *pending);
int lstm_hip_get_grad_accumulator(lstm_hip_t *h, float *host_block);        /* logical-N flat block, as get_params */
int lstm_hip_set_grad_accumulator(lstm_hip_t *h, const float *host_block, int32_t pending);

/* ---- the update rule of lstm_hip_adagrad and of every window of lstm_hip_train_windows (the name is kept for the seam)
 *   LSTM_HIP_OPT_ADAGRAD  the default above; beta1, beta2, eps and weight_decay must all be 0
 *   LSTM_HIP_OPT_ADAM     Adam with decoupled weight decay (torch.optim.AdamW, single-tensor form; weight_decay 0: plain
 *                         Adam); needs 0 <= beta1 < 1, 0 <= beta2 < 1, eps > 0, weight_decay >= 0, all finite.
 *                         At step number t (1-based, counted per handle), with d' = d * coef when clipping scales the step:
 *                           p <- p * (1 - lr*wd)                                 (only when wd > 0)
 *                           m <- m + (1 - beta1) * (d' - m)
 *                           v <- beta2 * v + (1 - beta2) * d'^2
 *                           p <- p - (lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 *                         The per-step scalars (lr / (1 - beta1^t), sqrt(1 - beta2^t), 1 - lr*wd, 1 - beta1, beta2,
 *                         1 - beta2, eps) are computed in double on the host and narrowed to float; the elementwise work,
 *                         m and v are fp32.  The decay covers the whole flat block, biases included.  Every step counts,
 *                         lr = 0 steps included (t advances, m and v are updated).
 * Anything else is LSTM_HIP_EINVAL.  A new kind zeroes the optimizer state (which = 2, and 3 for Adam) and the step count;
 * the same kind again keeps both and takes the new numbers (e.g. a new weight decay mid-run).  State blocks of
 * lstm_hip_set_params / lstm_hip_get_params: which = 2 is Adagrad's memory or Adam's first moment m, which = 3 Adam's
 * second moment v (LSTM_HIP_ESTATE on a handle that is not on Adam).  A padded handle keeps m and v at the padded width
 * with zero padding, as the memory.  With a communicator every rank applies the same step, with the same t, to the
 * all-reduced gradient.  The step counter advances once per update launched, for either kind; in one train_windows call
 * every window has its own t.  steps >= 0 for set. */
#define LSTM_HIP_OPT_ADAGRAD 0
#define LSTM_HIP_OPT_ADAM 1
int lstm_hip_set_optimizer(lstm_hip_t *h, int32_t kind, double beta1, double beta2, double eps, double weight_decay);
int lstm_hip_get_optimizer_steps(lstm_hip_t *h, int64_t *steps);
int lstm_hip_set_optimizer_steps(lstm_hip_t *h, int64_t steps);

/* ---- a running average of the weights over the trajectory, and inference from it
 *   LSTM_HIP_AVG_OFF      the default: no block, no counters, no launch; decay must be 0
 *   LSTM_HIP_AVG_EMA      exponential moving average; needs 0 <= decay < 1, finite
 *   LSTM_HIP_AVG_UNIFORM  the uniform running mean of the averaged iterates (SWA); decay must be 0
 *   every >= 1 for all three.  Anything else, an unknown kind and NaN included, is LSTM_HIP_EINVAL; the message says which
 *   number, and the handle stays usable.
 * Which updates count: every update the handle launches, the rule of the optimizer step counter -- lstm_hip_adagrad, each
 * window of lstm_hip_train_windows, each train pass of the adaptive coders; lr = 0 updates too.  With averaging on, after
 * each update seen += 1, and the update is DUE when seen % every == 0.  At a due update n += 1 and the average block a is
 * updated from the parameters p AFTER that update, per element of the whole flat block [W|U|b|Why|by]:
 *     n == 1   a = p                   an exact copy, no arithmetic: neither kind needs a bias correction
 *     n  > 1   a = a + w * (p - a)     fp32, three separately rounded operations, no fused multiply-add
 *              EMA: w = (float)(1.0 - decay);  UNIFORM: w = (float)(1.0 / (double)n);  both computed in double on the host
 * (NumPy's a + w * (p - a) on float32 arrays is bit for bit the same.)  Non-finite values propagate as they are.  The average
 * is written by one launch of its own on the handle's stream, after the update launch and only at due updates: nothing is
 * read back, nothing waits, and how lstm_hip_train_windows calls are cut into chunks does not show.  A handle that never
 * turns averaging on makes the launches it made before this call existed.  With a communicator every rank applies the same
 * rule to the same parameters; nothing is exchanged.  A LSTM_HIP_PAD_HIDDEN handle keeps the average at the internal width
 * with zero padding (0 in p, and written as 0 by lstm_hip_set_average, as lstm_hip_set_params does).
 * State: a new kind allocates the block if needed, zeroes it, sets seen = n = 0 and puts the inference source back to
 * LSTM_HIP_SRC_PARAMS; the same kind again keeps the block and both counters and takes the new decay and every;
 * LSTM_HIP_AVG_OFF drops averaging.  Per handle, may change between calls, not part of the engine plan.
 * lstm_hip_get_average / lstm_hip_set_average move the block as lstm_hip_get_params / lstm_hip_set_params move theirs
 * (logical-N flat block; with n == 0 get returns the zero block).  The average is not a fifth `which` block: which = 4 stays
 * LSTM_HIP_EINVAL there.  lstm_hip_set_averaging_counts needs 0 <= n <= seen (else LSTM_HIP_EINVAL; n = 0 while the inference
 * source is the average: LSTM_HIP_ESTATE); it exists for resuming, in this order: lstm_hip_set_averaging,
 * lstm_hip_set_average, lstm_hip_set_averaging_counts.  These four answer LSTM_HIP_ESTATE on a handle without averaging,
 * LSTM_HIP_EINVAL for a null pointer. */
#define LSTM_HIP_AVG_OFF 0
#define LSTM_HIP_AVG_EMA 1
#define LSTM_HIP_AVG_UNIFORM 2
int lstm_hip_set_averaging(lstm_hip_t *h, int32_t kind, double decay, int32_t every);
int lstm_hip_get_average(lstm_hip_t *h, float *host_block);        /* logical-N flat block, as get_params */
int lstm_hip_set_average(lstm_hip_t *h, const float *host_block);
int lstm_hip_get_averaging_counts(lstm_hip_t *h, int64_t *seen, int64_t *n);
int lstm_hip_set_averaging_counts(lstm_hip_t *h, int64_t seen, int64_t n);
/* which fp32 block lstm_hip_eval_bits, lstm_hip_sample, lstm_hip_generate*, lstm_hip_beam_search*, lstm_hip_score,
 * lstm_hip_encode and lstm_hip_decode read: the parameters (the default) or the average.  With LSTM_HIP_SRC_AVERAGE they take
 * W, b, Why and by from the average and pack their image of U from it, so every result is bit for bit what a second handle
 * of the same configuration gives after lstm_hip_set_params(0, the average).  Training never reads the source: parameters,
 * optimizer state and losses are those of a handle without it.  LSTM_HIP_SRC_AVERAGE is LSTM_HIP_ESTATE while averaging is
 * off or n == 0 (a zero model is never what the caller meant); the adaptive coders answer LSTM_HIP_ESTATE while the source
 * is the average (they code with the model they train); an unknown source is LSTM_HIP_EINVAL.  The source stays until it is
 * set again, averaging is turned off or a new kind is chosen. */
#define LSTM_HIP_SRC_PARAMS 0
#define LSTM_HIP_SRC_AVERAGE 1
int lstm_hip_set_inference_source(lstm_hip_t *h, int32_t source);

/* ---- weight drop: DropConnect on the hidden-to-hidden matrix U, one mask per training window
 * rate == 0 is off (the default); 0 < rate < 1 is on; anything else (negative, >= 1, NaN, infinite) is LSTM_HIP_EINVAL, the
 * message names the number and the handle stays usable.
 *
 * Numbering.  Element (r, k) of the logical 4N x N matrix U, r = g * N + j with the gates g in the order i, o, f, u, has the
 * number e = r + 4N * k, N being the handle's logical N: independent of padding and of the create flags, so fp32, bf16 and
 * LSTM_HIP_PAD_HIDDEN handles of one logical N share their masks.
 * Random word.  Philox4x32-10 with counter (c0, c1, c2, c3) = (low 32, high 32 bits of e >> 2, low 32, high 32 bits of t) and
 * key (k0, k1) = (low 32, high 32 bits of seed); round multipliers 0xD2511F53 (M0, for c0) and 0xCD9E8D57 (M1, for c2), key
 * increments 0x9E3779B9 and 0xBB67AE85; per round c <- (hi(M1*c2) ^ c1 ^ k0, lo(M1*c2), hi(M0*c0) ^ c3 ^ k1, lo(M0*c0)), then
 * the key is bumped; ten rounds.  The word of element e is output word e & 3.
 * Keep.  keep(e) <=> word >= thr, thr = (uint32) floor(rate * 2^32) computed in double on the host.
 * Scale.  s = (float)(1.0 / (1.0 - rate)), computed in double on the host and narrowed.
 *
 * Every recurrence of a training window (lstm_hip_forward / lstm_hip_backward, each window of lstm_hip_train_windows) reads
 * Ue, Ue_e = keep(e) ? U_e * s (one fp32 multiply) : +0.0f.  After the dU product the gradient block holds
 * dU_e = keep(e) ? dUe_e * s : +0.0f, the gradient with respect to U itself: lstm_hip_get_params(which = 1) returns it, the
 * clip norm is taken on it and the all-reduce sums it.  W, b, Why, by and their gradients are untouched.
 * The mask index t advances by one with every update the handle launches while weight drop is on (the rule of the optimizer
 * step counter: lstm_hip_adagrad, each window of lstm_hip_train_windows, lr = 0 too); a forward and a backward pass between
 * two updates use one mask.  set takes (rate, seed, t) together, get returns them; resuming is set with the saved t.
 *
 * Everything that is not a training window reads the unmasked parameters with no rescaling (inverted dropout):
 * lstm_hip_eval_bits, lstm_hip_sample, lstm_hip_generate*, lstm_hip_beam_search*, lstm_hip_score, lstm_hip_encode,
 * lstm_hip_decode, the running average and lstm_hip_get_params(0).
 * lstm_hip_set_weight_drop drops the forward pass: lstm_hip_backward after it is LSTM_HIP_ESTATE until a new
 * lstm_hip_forward.  The adaptive coders answer LSTM_HIP_ESTATE while weight drop is on (their containers record no mask); a
 * handle whose plan runs the dU product in halves (LSTM_HIP_DU_SPLIT) refuses set with LSTM_HIP_ESTATE.  With a communicator
 * every rank must be given the same (rate, seed, t); nothing is exchanged.  Per handle, may change between calls, not part of
 * the engine plan; a handle that never turns it on makes the launches it made before this call existed.
 *
 * lstm_hip_weight_drop_mask needs no device and no handle: keep[r + 4N * k] = 1 where element (r, k) is kept, else 0
 * (4N * N bytes; rate 0 keeps everything).  It runs the text the device runs. */
int lstm_hip_set_weight_drop(lstm_hip_t *h, double rate, uint64_t seed, uint64_t t);
int lstm_hip_get_weight_drop(lstm_hip_t *h, double *rate, uint64_t *seed, uint64_t *t);
int lstm_hip_weight_drop_mask(int32_t N, double rate, uint64_t seed, uint64_t t, uint8_t *keep);

/* ---- soft targets: label smoothing and distillation from a teacher
 * Per column (one stream at one step, target byte k, k < 0 for an empty target), with z = Why h + by the student's logits and
 * p their softmax in the handle's own mode (unshifted, or max-shifted under LSTM_HIP_STABLE_SOFTMAX):
 *   r    = (1 - eps) e_k + eps / 256 for k >= 0;  r = 0 for k < 0 (no smoothing mass: the hard term is dy = probs there)
 *   q    = softmax(z_T / tau), p_tau = softmax(z / tau), both max-shifted; z_T the teacher's logits of the same column.
 *          At tau = 1 p_tau is p itself, with no second softmax
 *   dy   = alpha (p - r) + (1 - alpha) tau (p_tau - q)     (without a teacher the second term is absent)
 * the gradient, in nats, of alpha CE(r, p) + (1 - alpha) tau^2 KL(q || p_tau).  The teacher's term applies to every column,
 * those with an empty target included.  dby = rowsum(dy).  The probabilities, the surprisals and every reported loss stay the
 * hard-target figures of p, so losses compare between runs with and without soft targets.
 * alpha, 1 - alpha, tau, 1 / tau, 1 - eps and eps / 256 are computed in double on the host and narrowed; the elementwise work
 * is fp32.  Results are held to tolerances, not to bits -- except when the feature is off: teacher NULL with opt NULL or
 * (alpha, tau, eps) = (1, 1, 0) leaves a handle that makes exactly the launches it made before this call existed.
 *
 * The teacher is a handle of the caller's with the same S, B and device; any N and any create flags.  It is borrowed: its
 * window, states and logit block are overwritten, its parameters (which = 0) only read, its inference source and average
 * ignored.  A forward pass of the student (lstm_hip_forward, each window of lstm_hip_train_windows) copies the student's
 * window inputs to the teacher, runs the teacher's forward recurrence and Why H product in the forms of the teacher's plan,
 * without its softmax launch, and then the student's forward pass, all on the student's stream: the two handles' recurrences
 * are never in flight together.  In lstm_hip_train_windows the teacher slides as the student does (its own column carry_col
 * becomes its column 0 before every window); in the single-window calls its column 0 is what the caller left there.
 * lstm_hip_slide_state and lstm_hip_set_state on the student never touch the teacher.  lstm_hip_backward on the teacher after
 * such a pass is LSTM_HIP_ESTATE.  When a call of the student that ran a forward pass returns, the teacher's window is the
 * student's last window as a whole, inputs AND targets, as if given to it by lstm_hip_set_window: lstm_hip_get_window on the
 * teacher returns it, and the teacher's own next lstm_hip_train_windows slides on from it with the teacher's own text and
 * cursors, which a student never touches.  (A teacher that is to go on training on its own text gets its window back from
 * its caller with lstm_hip_set_window.)
 *
 * Teacher KL.  kl = sum_m q_m (log2 q_m - log2 p_tau,m) per column, in log-sum-exp form, 0 where q_m is 0; per window
 * sum_t (sum_b kl) / B_global, summed as the window loss is, without the tau^2 factor.  lstm_hip_get_teacher_kl returns the
 * figures of the last lstm_hip_forward (1) or lstm_hip_train_windows (count), oldest first; n <= that number (else
 * LSTM_HIP_EINVAL); LSTM_HIP_ESTATE without a teacher.  They stay on the device until asked for.
 *
 * Refusals (the handle stays usable, nothing is launched).  LSTM_HIP_EINVAL: a wrong size, alpha outside [0, 1], tau <= 0 or
 * not finite, eps outside [0, 1), NaN anywhere, alpha != 1 or tau != 1 without a teacher, teacher == h, a teacher that has a
 * teacher (or a student that is one), a teacher whose S, B or device differ.  LSTM_HIP_ESTATE: a communicator on the student;
 * lstm_hip_train_text_windows and the adaptive coders while soft targets are on; a student forward while the teacher has
 * weight drop on; lstm_hip_destroy(teacher) while a student holds it (destroying or re-setting the student releases it).
 * Per handle, may change between calls, not part of the engine plan or of checkpoints.  A set drops the forward pass:
 * lstm_hip_backward is LSTM_HIP_ESTATE until a new lstm_hip_forward. */
typedef struct lstm_hip_soft_targets {
    uint32_t size;        /* sizeof(lstm_hip_soft_targets); anything else: LSTM_HIP_EINVAL */
    double alpha;         /* weight of the hard-target term, 0..1; must be 1 without a teacher */
    double temperature;   /* tau > 0 of the teacher term; must be 1 without a teacher */
    double smoothing;     /* eps in [0, 1): label smoothing of the hard target */
} lstm_hip_soft_targets;
int lstm_hip_set_soft_targets(lstm_hip_t *h, lstm_hip_t *teacher /* may be NULL */,
                              const lstm_hip_soft_targets *opt /* NULL with teacher NULL: off */);
int lstm_hip_get_soft_targets(lstm_hip_t *h, lstm_hip_t **teacher, lstm_hip_soft_targets *opt);
int lstm_hip_get_teacher_kl(lstm_hip_t *h, double *kl_bits, int64_t n);

/* ---- data-parallel exchange (new; the reference is single-device).  One SUM all-reduce of the
 *      flat gradient block per window over RCCL; every rank then applies the identical Adagrad step.
 *      With LSTM_HIP_PAD_HIDDEN the payload is the padded block (Np from N and the flags, so every
 *      rank of a job has the same layout). */
#define LSTM_HIP_UNIQUE_ID_BYTES 128
int lstm_hip_comm_unique_id(uint8_t id[LSTM_HIP_UNIQUE_ID_BYTES]);
int lstm_hip_comm_init(lstm_hip_t *h, const uint8_t id[LSTM_HIP_UNIQUE_ID_BYTES], int32_t nranks, int32_t rank);
int lstm_hip_allreduce_grads(lstm_hip_t *h);

/* ---- the whole i-loop on the device (OV/lstm_eigen_opt/lstm.cc:186-318 without the host hops).
 *      set_text uploads the corpus once (rawread, R/lstm.cc:382-420); set_cursors the B read
 *      positions (opt:140-144); reset_window clears x/target to the all-zero columns (opt:122,125).
 *      train_windows runs `count` iterations of: event=text[pos]; pos++ (wrap to S); slide;
 *      forward; loss; backward; [all-reduce]; Adagrad.  losses (may be NULL) receives `count`
 *      per-window losses (what the reference adds to epoch_loss); for ranks of a communicator
 *      that is the local sum over this rank's streams divided by the GLOBAL batch.
 *      elapsed_ms (may be NULL) receives the HIP-event time of the loop on the handle's stream.
 *      After the call the handle holds the LAST window: its states, gates, probabilities and gradient block.  (The windows
 *      before it need not have stored their probabilities and summed gradient: should the call, or an adaptive coding
 *      call, end with an error, lstm_hip_get_activations' probs and lstm_hip_get_params(which = 1) answer LSTM_HIP_ESTATE
 *      until a forward / backward pass has filled them again.) */
int lstm_hip_set_text(lstm_hip_t *h, const uint8_t *text, size_t len);
int lstm_hip_set_cursors(lstm_hip_t *h, const uint64_t *pos);
int lstm_hip_get_cursors(lstm_hip_t *h, uint64_t *pos);
int lstm_hip_reset_window(lstm_hip_t *h);
int lstm_hip_get_window(lstm_hip_t *h, int32_t *xi, int32_t *ti);
int lstm_hip_train_windows(lstm_hip_t *h, int64_t count, double learning_rate, double *losses, float *elapsed_ms);
/* window stride variants (OV/lstm_eigen_class_batch/lstm_segment.cc:110,130,183-187): train_windows advances every
 * stream by `stride` bytes per iteration (default 1, the root file) and takes the carry h[0],c[0] from column
 * `carry_col` of the previous window (default 1; the segment variant uses stride = S/2, carry_col = S/2 - 1). */
int lstm_hip_set_stride(lstm_hip_t *h, int32_t stride, int32_t carry_col);
/* global batch the loss is divided by (defaults to B; set by the host when streams are sharded) */
int lstm_hip_set_global_batch(lstm_hip_t *h, int32_t global_B);
/* what lstm_hip_loss / train_windows report:
 *   ALL_STEPS_BITS  the sum over all S-1 steps of -log2 p(target) / B (R/lstm.cc:204-207; the default)
 *   LAST_STEP_NATS  step S-1 only, natural log (the CPU class of that variant: forward_loss,
 *                   OV/lstm_eigen_class_CUDA/lstm.h:200-221)
 *   LAST_STEP_BITS  step S-1 only, -log2, / B: exactly cuLSTM::calculate_loss, the boundary member lstm_hip_loss replaces
 *                   (OV/lstm_eigen_class_CUDA/cu_lstm.h:203-215 with kernel_elementwise_neglog, cu_kernels.cu:211-225)
 * The gradients do not change: that variant's backward still uses dy of every step (lstm.h:299-302, cu_lstm.h:216-300). */
#define LSTM_HIP_LOSS_ALL_STEPS_BITS 0
#define LSTM_HIP_LOSS_LAST_STEP_NATS 1
#define LSTM_HIP_LOSS_LAST_STEP_BITS 2
int lstm_hip_set_loss_mode(lstm_hip_t *h, int32_t mode);

/* ---- held-out evaluator and sampler on the device (OV/lstm_eigen_class_CUDA/lstm.cc:661-720,
 *      578-659; R/lstm.cc:293-356).  eval: bits/char of `text` from h = c = 0.  sample: `count`
 *      bytes from state (h0,c0) (N floats each, in/out) using the caller's uniform draws u[i].
 *      Limit: a handle on the per-step engine (every width without a persistent recurrence, so every N > 1024) runs
 *      both in one workgroup with (6 Np + 256) * 4 bytes of LDS, Np the internal width.  Where that exceeds the
 *      device's opt-in limit per workgroup (160 KB on gfx950, which holds Np <= 6784) both return LSTM_HIP_EINVAL with a message
 *      naming N, before anything runs; the handle stays usable.  A launch the runtime refuses is LSTM_HIP_EHIP. */
int lstm_hip_eval_bits(lstm_hip_t *h, const uint8_t *text, size_t len, double *bits_per_char);
int lstm_hip_sample(lstm_hip_t *h, float *h0, float *c0, const double *u, int32_t count, uint8_t *out);
/* ---- batched, prompted sampling and per-text scoring (the loops of R/lstm.cc:293-356 and
 *      OV/lstm_eigen_class_CUDA/lstm.cc:578-720 over many independent streams at once).  Per stream s:
 *        start   state column s of h0 / c0 (N x streams each; NULL = zeros, test()'s reset_std = 0)
 *        prompt  prompts[prompt_off[s] .. prompt_off[s+1]) fed as inputs (prompts and prompt_off may both be NULL:
 *                no prompts); bits[s] (may be NULL) = sum over prompt positions j = 1..L-1 of -log2 p(prompt[j]) at
 *                temperature 1, so bits[s] / (L-1) is the text's lstm_hip_eval_bits from a zero start
 *        sample  then `count` bytes, byte i drawn from the current h and fed back as the next input (as lstm_hip_sample):
 *                with z = Why*h + by, temperature 1: p = expf(z) / sum (unshifted; max-shifted with
 *                LSTM_HIP_STABLE_SOFTMAX, which also scores prompts in log-sum-exp form); other temperature > 0:
 *                p ~ expf((z - max z) / temperature); 0 (and any temperature below FLT_MIN, its limit): argmax z,
 *                lowest index on ties.  The byte is the first m with
 *                u < cdf[m] (sequential float sum), 0 if none; the draw is u[i*streams + s] (u may be NULL only for
 *                temperature 0) and the byte goes to out[i*streams + s]
 *        final   h_out / c_out (N x streams each, may be NULL) receive the state after the stream's last input
 *      N is the logical N of the handle.  Computed from the fp32 parameters whatever the precision flags
 *      (LSTM_HIP_FAST_MATH applies); nothing else of the handle is read or changed (gradients, Adagrad memory, window,
 *      cursors, carry).  LSTM_HIP_EINVAL: streams outside 1..4096, count < 0, offsets not starting at 0 or decreasing,
 *      temperature negative or not finite, u missing with temperature > 0 and count > 0, out missing with count > 0. */
int lstm_hip_generate(lstm_hip_t *h, int32_t streams, const uint8_t *prompts, const uint64_t *prompt_off,
                      const float *h0, const float *c0, double temperature, const double *u, int32_t count,
                      uint8_t *out, double *bits, float *h_out, float *c_out);
/* ---- the same call with sampling controls.  Everything lstm_hip_generate documents holds: prompts,
 *      scoring, the order the draws are consumed in, final states, what of the handle is read, the refusals.  With top_k 0 or
 *      256, top_p 1 and stop_byte -1 the call is bit for bit lstm_hip_generate(..., opt->temperature, ...), which is a thin
 *      caller of this function.
 *        filter  per drawn byte, after temperature; greedy draws (temperature below FLT_MIN) and prompt scoring ignore it.
 *                z: the stream's 256 logits; p: the normalised terms of the CDF walk above (in the mode the temperature and
 *                LSTM_HIP_STABLE_SOFTMAX select).
 *                  1. rank_m = #{i : z_i > z_m} + #{i < m : z_i == z_m} (z descending, index ascending: top_k = 1 is
 *                     greedy decoding, lowest index on ties)
 *                  2. keep_k = top_k if 1..255, else 256
 *                  3. keep_p = 256 if top_p == 1; else walk ranks r = 0, 1, .. adding p[rank r] into one float:
 *                     keep_p = r + 1 at the first r where the sum >= (float)top_p, 256 if it never is
 *                  4. keep = min(keep_k, keep_p) >= 1
 *                  5. p'_m = p_m where rank_m < keep, else 0; s' = the sequential float sum of p' in index order;
 *                     p''_m = p'_m / s'
 *                  6. the byte is the first m with u < cdf[m] (sequential float sum of p''); if u passes every edge, the
 *                     largest kept index (a filtered draw is always a kept byte; unfiltered draws keep byte 0 there)
 *                kept[i*streams + s] (may be NULL) = keep for a filtered draw, 256 for an unfiltered one, 1 for a greedy
 *                one, 0 for positions after the stream has stopped.
 *                Without LSTM_HIP_STABLE_SOFTMAX, expf(z) can overflow at temperature 1: the byte is then unspecified (but a
 *                byte, and nothing faults).
 *        stop    stream s ends with its first DRAWN byte equal to stop_byte, at draw i (prompt bytes never stop it):
 *                out_len[s] (may be NULL) = i + 1, or count if it never comes; out[j*streams + s] = 0 for j >= out_len[s].
 *                The stop byte is still fed as an input: h_out / c_out are the state after it (the state after the
 *                stream's last input, with the stream's own length).  Draw i uses u[i*streams + s] as ever, so a stopped
 *                run is the prefix of the unstopped run with the same draws.
 *                The call still runs all max prompt length + count steps: stopped streams idle, no result is read back
 *                inside the loop and the loop does not end early.
 *      LSTM_HIP_EINVAL (the handle stays usable), beside lstm_hip_generate's: opt NULL or opt->size != sizeof(lstm_hip_sampling),
 *      top_k outside 0..256, top_p NaN, <= 0 or > 1, stop_byte outside -1..255. */
typedef struct lstm_hip_sampling {
    uint32_t size;        /* sizeof(lstm_hip_sampling); anything else: LSTM_HIP_EINVAL */
    double   temperature; /* as lstm_hip_generate */
    int32_t  top_k;       /* 0 or 256: off; 1..255: keep the k most likely bytes */
    double   top_p;       /* 1.0: off; 0 < top_p < 1: keep the smallest most-likely-first prefix whose mass reaches top_p */
    int32_t  stop_byte;   /* -1: off; 0..255: a stream ends with the first DRAWN byte equal to it */
} lstm_hip_sampling;
int lstm_hip_generate_ex(lstm_hip_t *h, int32_t streams, const uint8_t *prompts, const uint64_t *prompt_off,
                         const float *h0, const float *c0, const lstm_hip_sampling *opt, const double *u, int32_t count,
                         uint8_t *out, double *bits, float *h_out, float *c_out,
                         int32_t *out_len /* [streams], may be NULL */, uint16_t *kept /* [count*streams], may be NULL */);
/* ---- the same call under a constraint: a byte-level DFA decides, per stream, which bytes may come next (DESIGN.md section
 *      3.10).  Everything lstm_hip_generate_ex documents holds, and it is a thin caller of this function with con = NULL,
 *      start_state = end_state = NULL: that call makes the launches it made before this function existed.
 *        table   con->next[q*256 + b], con->states = Q states (1..4096): the state after byte b in state q (a value < Q), or
 *                0xFFFF: byte b is forbidden in state q.  A_q is the number of allowed bytes of state q.  There are no
 *                accepting states: the caller reads the final state (lstm_hip_generate_accepting, below, has them).
 *        prompt  q starts at start_state[s] (NULL: 0) and is advanced over the stream's prompt bytes on the host, before
 *                anything is launched; a prompt byte that is forbidden where it stands is LSTM_HIP_EINVAL (the message names
 *                the stream and the byte's offset in its prompt).  Prompt scoring (bits) ignores the constraint: it stays the
 *                text's evaluation bits.
 *        draw    z'_m = z_m where next[q][m] is allowed, -inf otherwise.  Rules 1-6 above run on z' (and on p formed from z':
 *                max, expf and the normalising sum see the masked logits), with keep = min(keep_k, keep_p, A_q), and a
 *                constrained draw is ALWAYS a filtered draw, also with top_k and top_p off: its terms are divided by the
 *                index-order float sum of the kept terms, and if u passes every edge the byte is the largest kept index.
 *                Greedy draws take the argmax of z', lowest index on ties.  kept = keep (<= A_q), 1 for a greedy draw.
 *        advance q <- next[q][x].  Should x be forbidden where it stands (possible only with non-finite parameters or an
 *                overflowing expf), the byte written and fed is the lowest allowed byte of q instead: out is always accepted
 *                by the table and q never leaves it.
 *        stop    as above; a stop byte that is forbidden never comes.
 *        final   end_state[s] (may be NULL) = q after the stream's last drawn byte, the state after its prompt if it drew
 *                none.  A second call with h0 / c0 = h_out / c_out, no prompt, start_state = end_state and the remaining
 *                draws gives the bytes and states of the one long call, bit for bit.
 *      LSTM_HIP_EINVAL (the handle stays usable, the message says which), beside lstm_hip_generate_ex's: start_state or
 *      end_state given with con NULL; con->size != sizeof(lstm_hip_constraint); states outside 1..4096; next NULL; an entry
 *      that is neither < states nor 0xFFFF; a start state outside 0..states-1; a state that can be reached from some stream's
 *      start state and has no allowed byte (breadth-first from the start states: unreachable rows may be empty); a prompt
 *      byte the table rejects.  The coders and lstm_hip_sample take no constraint (beam search does: see
 *      lstm_hip_beam_search_constrained). */
typedef struct lstm_hip_constraint {
    uint32_t size;        /* sizeof(lstm_hip_constraint); anything else: LSTM_HIP_EINVAL */
    int32_t  states;      /* Q: 1..4096 */
    const uint16_t *next; /* [Q*256]: next state, or 0xFFFF = forbidden */
} lstm_hip_constraint;
int lstm_hip_generate_constrained(lstm_hip_t *h, int32_t streams, const uint8_t *prompts, const uint64_t *prompt_off,
                                  const float *h0, const float *c0, const lstm_hip_sampling *opt, const double *u, int32_t count,
                                  uint8_t *out, double *bits, float *h_out, float *c_out, int32_t *out_len, uint16_t *kept,
                                  const lstm_hip_constraint *con, const int32_t *start_state /* [streams], may be NULL: all 0 */,
                                  int32_t *end_state /* [streams], may be NULL */);
/* Two tables for it; neither needs a device or a handle.
 * lstm_hip_dfa_utf8 returns 8 and, if next is not NULL, fills 8*256 entries with the automaton of well-formed UTF-8 (no
 * overlong forms, no surrogates, nothing above U+10FFFF).  The numbering is part of the contract; state 0 is the start state and
 * the only character boundary, so a stream whose end_state is 0 ended on a whole character.
 *      state 0: 00-7F -> 0, C2-DF -> 1, E0 -> 3, E1-EC -> 2, ED -> 4, EE-EF -> 2, F0 -> 6, F1-F3 -> 5, F4 -> 7
 *      state 1: 80-BF -> 0      state 2: 80-BF -> 1      state 3: A0-BF -> 1      state 4: 80-9F -> 1
 *      state 5: 80-BF -> 2      state 6: 90-BF -> 2      state 7: 80-8F -> 2      everything else is forbidden
 * (allowed bytes per state: 179, 64, 64, 32, 32, 64, 48, 16.)
 * lstm_hip_dfa_restrict forbids every transition on a byte b with allow[b] == 0 in a table of `states` states, then
 * repeatedly forbids the transitions into states that have no allowed byte left, until nothing changes.  State numbers do not
 * change.  Returns 0, or LSTM_HIP_EINVAL when state 0 ends up with no allowed byte (or the table is not one: NULL, states
 * outside 1..4096, an entry that is neither a state nor 0xFFFF). */
int32_t lstm_hip_dfa_utf8(uint16_t *next);
int lstm_hip_dfa_restrict(uint16_t *next, int32_t states, const uint8_t allow[256]);
/* ---- a byte regular expression compiled to such a table.  Host only: no handle, no device.
 *      Returns the number of states Q, 1..4096.  With next == NULL && accept == NULL it only returns Q and ignores cap;
 *      otherwise cap >= Q is required, next takes Q*256 entries (a next state, or 0xFFFF) and accept Q flags (1: accepting).
 *      Every failure returns LSTM_HIP_EINVAL; lstm_hip_last_error() says what is wrong and at which byte of the pattern, and
 *      *error_pos (may be NULL) gets that byte offset, or -1 for a failure without a position: too many states, an empty
 *      language, a stop-byte conflict, cap too small.
 *        language  a match is ALWAYS a whole-string match; the pattern is bytes, with the meaning Python's re.fullmatch gives a
 *                  bytes pattern without flags, for this subset:
 *                    literals     any byte other than \ . [ ] ( ) | * + ? { } ^ $ stands for itself, bytes >= 0x80 included:
 *                                 UTF-8 text in a pattern is its byte sequence, and A QUANTIFIER BINDS THE LAST BYTE, as in
 *                                 Python: group a multi-byte character before repeating it, (?:\xC3\xA9)+.
 *                    .            any byte except 0x0A
 *                    escapes      \n \r \t \f \v \xHH; \d \D \w \W \s \S with their ASCII meaning (\w = [A-Za-z0-9_], \s =
 *                                 [ \t\n\r\f\v], the upper-case forms their complements over 0..255); a backslash before an
 *                                 ASCII punctuation byte is that byte; before any other byte it is refused
 *                    classes      [...] and [^...] of single bytes, ranges a-z and the escapes above (class escapes included,
 *                                 though not as a range end); a - that comes first or last is a literal; ] and [ must be
 *                                 escaped; a raw byte >= 0x80 is refused (write \xHH); [^...] is the complement over 0..255
 *                    groups       ( ) and (?: ), both only grouping, nested at most 200 deep; every other (? form is refused
 *                    alternation  | ; empty alternatives are allowed, and the empty pattern matches the empty string
 *                    quantifiers  * + ? {m} {m,} {m,n} {,n} with m <= n <= 4095.  A quantifier directly behind a quantifier
 *                                 is refused (lazy and possessive forms, a**: group first), and so is a { that does not start
 *                                 a well-formed quantifier (stricter than Python)
 *                    anchors      ^ and $ are refused: there is nothing to anchor
 *        result    the MINIMAL automaton of the language, trimmed: every state can be reached from state 0 and can reach an
 *                  accepting state.  State 0 is the start state; states are numbered breadth-first from it, the bytes of a
 *                  state visited in ascending order, so two patterns with the same language (a|b and [ab]) give byte-identical
 *                  tables.  A pattern that matches nothing, or whose automaton has more than 4096 states, is refused.
 *        limits    the construction is bounded, so a pattern whose automaton explodes fails quickly instead of exhausting
 *                  memory: at most 2^20 nodes of the unrolled pattern (a bounded repeat is copies of its operand), 32768
 *                  states and 2^27 node visits of the subset construction before minimisation.  Past any of them:
 *                  LSTM_HIP_EINVAL, "too many states".
 *        stop_byte -1: the table of the language L itself, accept = L's accepting states.  Such a table can hold accepting
 *                  states whose rows are empty; the table checks of the calls that take it apply.
 *                  0..255: the table of L followed by the stop byte.  If the trimmed automaton of L has a transition on the
 *                  stop byte the call fails ("the pattern can match the stop byte": a stream ends at its first drawn stop
 *                  byte).  Otherwise every accepting state of L gets a transition on the stop byte into one new final state,
 *                  the only accepting state, whose row allows the stop byte alone, back to itself: no reachable row is empty,
 *                  and the generator, the scorer and beam search take the table as it is.
 * lstm_hip_dfa_intersect builds the product of two tables from (0, 0): a byte is allowed iff both allow it, a product state
 * accepts iff both components do (a NULL accept array: every state accepts).  The product goes through the same trimming,
 * minimisation and numbering, with the same two-call sizing; the product may have at most 32768 states before minimisation.
 * LSTM_HIP_EINVAL: more than 4096 states, an empty language, cap too small, or a table that is not one (NULL, states outside
 * 1..4096, an entry that is neither a state nor 0xFFFF).  --utf8 --regex of lstm_generate is this call with the UTF-8 table
 * and accept = {0}. */
int32_t lstm_hip_dfa_regex(const uint8_t *pattern, size_t len, int32_t stop_byte /* -1: none */, uint16_t *next, uint8_t *accept,
                           int32_t cap, int32_t *error_pos /* may be NULL */);
int32_t lstm_hip_dfa_intersect(const uint16_t *a, int32_t qa, const uint8_t *acc_a /* may be NULL */, const uint16_t *b, int32_t qb,
                               const uint8_t *acc_b /* may be NULL */, uint16_t *next, uint8_t *accept, int32_t cap);
/* ---- beam search: per stream the W = opt->beams most likely continuations of its prompt that the
 *      search finds, with their costs in bits.  Prompts, prompt_off, h0 / c0 (N x streams; NULL = zeros) are those of
 *      lstm_hip_generate.  Stream s is fed its prompt of length L (nothing is scored during the prompt) and makes selection
 *      i = t - L at steps t = L .. L+count-1.  It keeps W slots; all start from the stream's start state, slot 0 with cost 0
 *      and slots 1..W-1 with cost +inf, so the first selection expands slot 0 only.
 *        cost       of extending live slot j by byte m: z = Why*h_j + by summed as lstm_hip_generate sums it (sequentially in
 *                   k, separate multiply and add); zmax = max z; s = the sequential float sum, in index order, of
 *                   expf(z_k - zmax); c_m = log2f(s) + (zmax - z_m) * 1.44269504088896341f in float (the surprisal of the
 *                   LSTM_HIP_STABLE_SOFTMAX prompt scorer: ALWAYS max-shifted, whatever that flag says).  The candidate
 *                   costs the double cost_j + (double)c_m.  Only the fp32 parameters are read (a bf16 handle searches as an
 *                   fp32 one); LSTM_HIP_FAST_MATH applies to the recurrence only, as in lstm_hip_generate.
 *        finished   a slot is finished by its first SELECTED byte equal to stop_byte.  A finished slot offers exactly one
 *                   candidate: itself, cost unchanged, byte 0, no new input.
 *        selection  of all candidates of the stream, the first W in this order are selected: cost ascending (NaN taken as
 *                   +inf), then parent slot ascending, then z descending, then byte ascending; new slot r is the r-th of
 *                   them.  (Ordering by z inside one parent makes beams = 1 exactly greedy decoding, lowest index on ties.)
 *        records    trace_parent[i*streams*W + s*W + r] and trace_byte[..] (both may be NULL): the slot that new slot r
 *                   extends and the byte.  The slot's length is its parent's + 1 for a live parent, unchanged for a finished
 *                   one; it is finished when the selected byte is stop_byte.  A live slot's byte is its next input (the stop
 *                   byte is still fed, though no output depends on it); a finished slot gets no input.  States follow parents.
 *        results    per stream the final slots in rank order r = 0..W-1; hypothesis r is found by walking the back-pointers
 *                   from the last selection.  out[(s*W + r)*count + i] holds its bytes and is 0 from out_len[s*W + r] on;
 *                   out_len includes the stop byte; bits[s*W + r] is the cost (raw cost order: no length normalisation).
 *      No final states are returned: feed prompt + hypothesis to lstm_hip_generate with count 0 to continue from one.  The
 *      loop runs max L + count steps with no readback and no early exit.  Nothing of the handle but P is read or written,
 *      as for lstm_hip_generate.  With count 0 nothing is selected: out_len = 0 and bits = the start costs, where given.
 *      With non-finite parameters the hypotheses are unspecified, but they are bytes and every index stays in its table.
 *      LSTM_HIP_EINVAL (the handle stays usable): opt NULL or opt->size != sizeof(lstm_hip_beam), beams outside 1..32,
 *      streams < 1 or streams * beams > 4096, internal hidden width * beams > 16384, count < 0, stop_byte outside -1..255,
 *      offsets not starting at 0 or decreasing, prompts without offsets or offsets without prompts, out, out_len or bits
 *      NULL with count > 0.  LSTM_HIP_EHIP: the device refused the kernel's LDS request. */
typedef struct lstm_hip_beam {
    uint32_t size;      /* sizeof(lstm_hip_beam); anything else: LSTM_HIP_EINVAL */
    int32_t  beams;     /* W: 1..32 hypotheses kept per stream */
    int32_t  stop_byte; /* -1: off; 0..255: a hypothesis is finished by its first SELECTED byte equal to it */
} lstm_hip_beam;
int lstm_hip_beam_search(lstm_hip_t *h, int32_t streams, const uint8_t *prompts, const uint64_t *prompt_off,
                         const float *h0, const float *c0, const lstm_hip_beam *opt, int32_t count,
                         uint8_t *out      /* [streams][W][count] */,
                         int32_t *out_len  /* [streams*W] */,
                         double  *bits     /* [streams*W] */,
                         uint8_t *trace_parent /* [count][streams*W], may be NULL */,
                         uint8_t *trace_byte   /* [count][streams*W], may be NULL */);
/* ---- beam search under a constraint, with accepting states: per stream the most likely
 *      continuations THAT THE TABLE ACCEPTS.  lstm_hip_beam_search is a thin caller of this function with bc = start_state =
 *      end_state = NULL, and that call makes the launches it made before this function existed.  Everything
 *      lstm_hip_beam_search documents holds under a constraint, except:
 *        states     every slot carries a state q of bc->con (the table of lstm_hip_generate_constrained).  The stream's state
 *                   starts at start_state[s] (NULL: 0) and is advanced over the stream's prompt on the host before anything is
 *                   launched; a prompt byte forbidden where it stands is LSTM_HIP_EINVAL (the message names the stream and the
 *                   offset).  All W slots start in the resulting state q0.  A live slot extended by byte m moves to
 *                   next[q][m]; a finished slot keeps its state; states follow parents like h and c.  end_state[s*W + r] (may
 *                   be NULL) is the state of final slot r.
 *        absent     slots 1..W-1 start FINISHED: cost +inf, length 0, state q0 (in the unconstrained call they start live
 *                   with cost +inf).  They offer themselves as any finished slot does and are selected only when fewer than W
 *                   other candidates exist, so a hypothesis with bits = +inf and out_len = 0 is "no such hypothesis": a table
 *                   that allows fewer than W strings returns fewer.  Every live slot offers at least one candidate (deadline)
 *                   and every finished slot exactly one, so a selection always finds W.
 *        cost       z'_m = z_m where next[q][m] is allowed, -inf otherwise; zmax, the sequential float sum of
 *                   expf(z'_k - zmax) and the surprisal are taken on z'.  A forbidden term adds 0.0f, so the sum is the one
 *                   over the allowed bytes in index order: this is the max-shifted surprisal lstm_hip_score computes under
 *                   the same table, and a hypothesis's bits is, bit for bit, the double sum in text order of the surprisal[]
 *                   entries a LSTM_HIP_STABLE_SOFTMAX handle's lstm_hip_score(con) gives its bytes.  The deadline removes
 *                   candidates; it never changes a cost.
 *        deadline   only with bc->accept.  acc(q) = accept[q] != 0.  F[0][q] = acc(q); for R >= 1, F[R][q] = OR over the
 *                   allowed bytes b of q of: acc(next[q][b]) if b is the stop byte, F[R-1][next[q][b]] otherwise ("from q an
 *                   accepted end is reached by exactly R more bytes, or fewer when the last is the stop byte").  At selection
 *                   i, with R = count - i, candidate (slot j, byte m) EXISTS iff slot j is live, nx = next[q_j][m] is allowed,
 *                   and acc(nx) if m is the stop byte, F[R-1][nx] otherwise.  Candidates that do not exist are not offered.
 *                   F[count][q0] is checked, and the rule keeps F[R][q] true for every live slot, so it always offers a
 *                   candidate.  Hence every hypothesis with finite bits ends in an accepting state: finished by a stop byte
 *                   into one, or holding exactly count bytes and standing in one.  With accept = NULL every state accepts, no
 *                   table is built or read and there is no deadline (a stop byte may then end a hypothesis anywhere).
 *                   Building F is host work before the first launch: at most count * (transitions between distinct states)
 *                   steps, and only copies once two rows in sequence are equal (for the UTF-8 table: from row 4 on).
 *        order      among the candidates that exist, the four-key order of lstm_hip_beam_search.
 *        count 0    out_len = 0, bits = the start costs, end_state = q0 for every slot; with accept, q0 must be accepting.
 *      LSTM_HIP_EINVAL (the handle stays usable, the message says which), beside those of lstm_hip_beam_search: start_state
 *      or end_state given with bc NULL; bc->size != sizeof(lstm_hip_beam_constraint); bc->con NULL; every table refusal of
 *      lstm_hip_generate_constrained; a prompt byte the table rejects; with accept: F[count][q0] false for some stream (the
 *      message names it: "no accepted string of `count` bytes or fewer ending in the stop byte"), or (count + 1) * states
 *      above 2^28. */
typedef struct lstm_hip_beam_constraint {
    uint32_t size;                    /* sizeof(lstm_hip_beam_constraint); anything else: LSTM_HIP_EINVAL */
    const lstm_hip_constraint *con;   /* the table, as lstm_hip_generate_constrained takes it; required */
    const uint8_t *accept;            /* [con->states], nonzero = accepting; NULL: every state accepts */
} lstm_hip_beam_constraint;
int lstm_hip_beam_search_constrained(lstm_hip_t *h, int32_t streams, const uint8_t *prompts, const uint64_t *prompt_off,
                                     const float *h0, const float *c0, const lstm_hip_beam *opt, int32_t count,
                                     uint8_t *out, int32_t *out_len, double *bits, uint8_t *trace_parent, uint8_t *trace_byte,
                                     const lstm_hip_beam_constraint *bc /* NULL: exactly lstm_hip_beam_search */,
                                     const int32_t *start_state /* [streams], may be NULL: all 0 */,
                                     int32_t *end_state /* [streams*W], may be NULL */);
/* ---- sampling with accepting states: lstm_hip_generate_constrained with the deadline rule of beam
 *      search, so that every stream ends on a whole accepted string and never in the middle of a pattern.
 *      lstm_hip_generate_constrained is a thin caller of this function, and two cases are exactly the earlier calls, with the
 *      launches and the bits they had before this function existed: bc == NULL is lstm_hip_generate_ex, and bc->accept == NULL
 *      is lstm_hip_generate_constrained(bc->con).  With bc->accept everything lstm_hip_generate_constrained documents holds,
 *      except:
 *        table F   as in lstm_hip_beam_search_constrained, with opt->stop_byte: acc(q) = accept[q] != 0; F[0][q] = acc(q);
 *                  F[R][q] = OR over the allowed bytes b of q of acc(next[q][b]) if b is the stop byte, F[R-1][next[q][b]]
 *                  otherwise.  It is built on the host before the first launch.
 *        exists    at draw i of stream s, with R = count - i, q the stream's state and nx = next[q][m], byte m EXISTS iff nx is
 *                  allowed and: acc(nx) if m is the stop byte, F[R-1][nx] otherwise.  E is the number of existing bytes;
 *                  E >= 1 at every draw of every stream, because F[count][q0] is checked and the rule keeps F[R][q] true.
 *        draw      z'_m = z_m where m exists, -inf otherwise; everything said of z' holds with E in place of A_q: rank, max,
 *                  expf and the normalising sum see the mask, a tempered draw is a filtered draw with keep = min(keep_k,
 *                  keep_p, E), greedy takes the argmax of z'.  A byte that does not exist and was chosen all the same
 *                  (non-finite logits only) is replaced by the lowest EXISTING byte.  Prompt scoring ignores all of this.
 *        end       a stream ends with its first drawn stop byte, which now exists only where it leads into an accepting state;
 *                  a stream that never draws it holds exactly count bytes and stands in an accepting state.  So
 *                  acc(end_state[s]) holds for every stream, always, also with non-finite parameters.
 *        chaining  two calls in sequence are NOT the one long call any more: each call has its own deadline, so the first
 *                  call ends every stream in an accepting state where the long call would only have passed through.
 *        count 0   nothing is drawn; every stream's state after its prompt must be accepting.
 *      LSTM_HIP_EINVAL (the handle stays usable, nothing is launched), beside those of lstm_hip_generate_constrained:
 *      bc->size != sizeof(lstm_hip_beam_constraint); bc->con NULL; F[count][q0] false for some stream (the message names it:
 *      "no accepted string of `count` bytes or fewer ending in the stop byte"; with count 0: q0 not accepting); (count + 1) *
 *      states above 2^28. */
int lstm_hip_generate_accepting(lstm_hip_t *h, int32_t streams, const uint8_t *prompts, const uint64_t *prompt_off,
                                const float *h0, const float *c0, const lstm_hip_sampling *opt, const double *u, int32_t count,
                                uint8_t *out, double *bits, float *h_out, float *c_out, int32_t *out_len, uint16_t *kept,
                                const lstm_hip_beam_constraint *bc /* NULL: exactly lstm_hip_generate_ex */,
                                const int32_t *start_state /* [streams], may be NULL: all 0 */,
                                int32_t *end_state /* [streams], may be NULL */);
/* ---- the same call with logit processors: an additive bias, min-p, and the no-repeat n-gram rule,
 *      applied on the device inside the step loop, with no readback.  lstm_hip_generate_accepting is a thin caller of this
 *      function with lp = NULL, and two cases are exactly that call, with its scratch offsets, uploads, kernel instantiations
 *      and bytes: lp == NULL, and a block with everything off (bias NULL, min_p 0, no_repeat 0).  Everything
 *      lstm_hip_generate_accepting documents holds, except what follows.  Only DRAWN bytes are processed: prompt scoring
 *      (bits) ignores all of it, as it ignores a constraint.  Per drawn byte of stream s, from z_m = Why*h + by summed as ever:
 *        1 bias      z_m <- z_m + bias[m], one float add.  Greedy draws see it too.
 *        2 valid     V_m: the table allows byte m (with accept: byte m EXISTS under the deadline); without a table every m.
 *        3 ban       T = history[s] ++ prompt[s] ++ the bytes drawn so far, len = |T|, n = no_repeat.  If len >= n - 1, suf is
 *                    the last n - 1 bytes of T and B_m holds iff some j with j + n - 1 < len has T[j .. j+n-1) == suf and
 *                    T[j+n-1] == m (n = 1 bans every byte that occurs in T); otherwise B is empty.  This is the
 *                    no_repeat_ngram_size rule of the usual toolkits, on bytes.  The history is never fed and never scored.
 *                    COST: the device scans T at every draw (256 positions at a time per stream, up to n - 1 byte compares
 *                    each): linear in len per draw, quadratic over a call; hence the 65536-byte limit below.
 *        4 survive   S = #{m : V_m and not B_m}.  If S == 0 the ban is DROPPED FOR THIS DRAW (B <- empty, S = #V): the table
 *                    always wins, and the guarantees of lstm_hip_generate_constrained and lstm_hip_generate_accepting (out is
 *                    accepted, the end state accepts) hold unchanged.  z'_m = z_m where V_m and not B_m, -inf otherwise.
 *        5 filter    rank, max, expf and the normalising sum see z'.  Rules 1-6 of lstm_hip_generate_ex apply with one more
 *                    cap: thr = (float)min_p * sorted[0] (one float multiply; sorted: the normalised terms in rank order),
 *                    keep_m = the first rank r with sorted[r] < thr, 256 if there is none (>= 1), and
 *                    keep = min(keep_k, keep_p, keep_m, S).  The owner lane takes the nucleus walk FIRST, bounded by keep_k and
 *                    S as before, and the min-p walk SECOND, over the ranks the nucleus walk kept (the minimum is the same).
 *        6 draw      a draw with any processor on is ALWAYS a filtered draw, as a constrained one is: the kept terms are divided
 *                    by their index-order float sum, past every edge the byte is the largest kept index, kept = keep.  Greedy
 *                    draws take the argmax of z', lowest index on ties, kept = 1; they ignore min_p.
 *        7 replace   a chosen byte that is no survivor (non-finite logits only) gives way to the lowest surviving byte.
 *        chaining    without accept, a second call with h0 / c0 = h_out / c_out, start_state = end_state, no prompt and
 *                    history[s] = the first call's history ++ prompt ++ drawn bytes gives the bytes and states of the one long
 *                    call, bit for bit.
 *      Beam search, the scorer, the coders and lstm_hip_sample take no processors.
 *      LSTM_HIP_EINVAL (the handle stays usable, nothing is launched, the message says which), beside those of
 *      lstm_hip_generate_accepting: lp->size wrong; a bias entry that is NaN or infinite (to ban a byte, restrict a table:
 *      lstm_hip_dfa_restrict); min_p NaN, negative or above 1; no_repeat outside 0..64; history without history_off or
 *      history_off without history; history_off not starting at 0 or decreasing; history given with no_repeat 0; with
 *      no_repeat > 0, the longest (history + prompt) + count above 65536. */
typedef struct lstm_hip_logit_processors {
    uint32_t size;               /* sizeof(lstm_hip_logit_processors); anything else: LSTM_HIP_EINVAL */
    const float *bias;           /* [256] added to the logits of every drawn byte, or NULL: none */
    double   min_p;              /* 0: off; 0 < min_p <= 1 */
    int32_t  no_repeat;          /* 0: off; n in 1..64: no n-gram of a stream's text occurs twice */
    const uint8_t  *history;     /* bytes that precede each stream's prompt for the n-gram rule only, or NULL */
    const uint64_t *history_off; /* [streams + 1]; NULL with history NULL */
} lstm_hip_logit_processors;
int lstm_hip_generate_processed(lstm_hip_t *h, int32_t streams, const uint8_t *prompts, const uint64_t *prompt_off,
                                const float *h0, const float *c0, const lstm_hip_sampling *opt, const double *u, int32_t count,
                                uint8_t *out, double *bits, float *h_out, float *c_out, int32_t *out_len, uint16_t *kept,
                                const lstm_hip_beam_constraint *bc, const int32_t *start_state, int32_t *end_state,
                                const lstm_hip_logit_processors *lp /* NULL: exactly lstm_hip_generate_accepting */);
/* ---- guided generation and scoring: a log-linear mix of the logits of several models that are fed
 *      the same bytes, each carrying its own recurrent state: z' = a*z + SUM_k b_k*z^k.  (1+g, -g) with a smaller model is
 *      contrastive decoding, with the same model on another context it is guidance with a negative context, and weights that
 *      sum to 1 are the geometric mean of an ensemble.  lstm_hip_generate_processed and lstm_hip_score are thin callers of the
 *      two functions below with gd = NULL, and that case is exactly the earlier call, with its scratch offsets, uploads,
 *      launches and bytes.  Everything lstm_hip_generate_processed / lstm_hip_score document holds, except what follows.
 *        feeding    every guide is fed the inputs the main model is fed, in the same steps: the prompt bytes, then the drawn
 *                   bytes; for the scorer the text.  Each guide advances its own state from its own h0 / c0 (N_k x streams, N_k
 *                   the guide's logical N; NULL = zeros) through its own W, U, b.  The block its
 *                   lstm_hip_set_inference_source names is read, its LSTM_HIP_FAST_MATH applies to its recurrence, weight drop is
 *                   never applied.  A guide is only read, nothing of it is written: model == h is allowed (the same weights with
 *                   a second state: the guidance case), and so is the same handle in two guides.
 *        logits     z^k_m = Why_k*h_k + by_k summed as lstm_hip_generate sums it (sequentially in the hidden index, multiply and
 *                   add separately rounded, by added last): bit for bit what guide k's own call computes from that state.
 *        mixing     g_m = b_1*z^1_m, then g_m = g_m + b_k*z^k_m for k = 2.. in index order, then z_m <- a*z_m + g_m.  Every
 *                   weight is narrowed to float on the host; every multiply and every add is one fp32 operation, no contraction.
 *        generator  mixing is step 0 of the processors' list, ahead of the bias.  Only DRAWN bytes are mixed, greedy draws see
 *                   it; prompt bits ignore it, as they ignore the processors and the table.  A guided draw is a processed draw
 *                   (always filtered, kept = keep).  Tables, accepting states, the n-gram rule, min-p, top-k / top-p and the
 *                   replace rules then run on the mixed logits unchanged; out is still always accepted by the table.
 *        stopping   a stream that has stopped idles in every guide too.  guide.h_out / c_out is the guide's state after the
 *                   stream's last input, the stop byte included: the rule of the main h_out.
 *        chaining   (generator) a second call that passes every model's h_out / c_out as its h0 / c0, start_state = end_state
 *                   and the history as lstm_hip_generate_processed hands it over gives the one long call, bit for bit.
 *        scorer     every scored byte is scored under the mixed logits: surprisal, entropy, rank, top bytes and top bits, and
 *                   bits are defined on z' exactly as they are on z.  The constraint mask comes after the mix.  With first = 1
 *                   byte 0 sees every guide's start state.  Chaining in pieces holds with the guides' states handed over too.
 *        ordering   all launches go on the main handle's stream.  Where model != h the call first makes that stream wait on an
 *                   event recorded on the guide's stream, so work the caller queued on the guide is finished.  The call ends
 *                   synchronised.  A guide may not be used by another host thread during the call.
 *        cost       per step one more launch for all guides together (their logits and the mix) and one recurrence step per guide;
 *                   the guides' images of U, states and the sum live in the MAIN handle's working memory.
 *      Beam search, the adaptive coders, lstm_hip_sample, lstm_hip_eval_texts and lstm_hip_embed_texts take no guides; the
 *      static coders take them through lstm_hip_encode_mixed / lstm_hip_decode_mixed (below).
 *      LSTM_HIP_EINVAL (the handle stays usable, nothing is launched; the message names the guide's index), beside those of the
 *      unguided call, which come first: gd->size wrong; nguides outside 1..LSTM_HIP_MAX_GUIDES; guides NULL; main_weight or a
 *      weight NaN or infinite; a NULL model; a guide on another device; a guide whose internal width is above 16384.
 *      LSTM_HIP_EHIP: the device refused the LDS request of the guides' kernel (nothing of that step is launched). */
#define LSTM_HIP_MAX_GUIDES 4
typedef struct lstm_hip_guide {
    lstm_hip_t *model;          /* any handle on the same device, any N and flags; MAY BE h ITSELF */
    double weight;              /* b_k: finite; negative and 0 allowed */
    const float *h0, *c0;       /* N_k x streams (the guide's logical N), NULL = zeros */
    float *h_out, *c_out;       /* N_k x streams, may be NULL: the guide's state after the stream's last input */
} lstm_hip_guide;
typedef struct lstm_hip_guidance {
    uint32_t size;              /* sizeof(lstm_hip_guidance); anything else: LSTM_HIP_EINVAL */
    double main_weight;         /* a: finite */
    int32_t nguides;            /* 1..LSTM_HIP_MAX_GUIDES */
    const lstm_hip_guide *guides;
} lstm_hip_guidance;
int lstm_hip_generate_guided(lstm_hip_t *h, int32_t streams, const uint8_t *prompts, const uint64_t *prompt_off,
                             const float *h0, const float *c0, const lstm_hip_sampling *opt, const double *u, int32_t count,
                             uint8_t *out, double *bits, float *h_out, float *c_out, int32_t *out_len, uint16_t *kept,
                             const lstm_hip_beam_constraint *bc, const int32_t *start_state, int32_t *end_state,
                             const lstm_hip_logit_processors *lp,
                             const lstm_hip_guidance *gd /* NULL: exactly lstm_hip_generate_processed */);
/* ---- per-byte scores: what the model thinks of every byte of given texts.  Stream s is
 *      text[text_off[s] .. text_off[s+1]), 1 <= streams <= 4096; empty streams are allowed (no entries, h_out = the start
 *      state).  h0 / c0 / h_out / c_out are N x streams as in lstm_hip_generate (NULL = zeros / not wanted); h_out is the
 *      state after the stream's last byte.  Per-position outputs are indexed like text: byte j of stream s is entry
 *      text_off[s] + j; an unscored byte (j = 0 with first = 0) has all-zero entries.
 *        rule       byte j, value x, is scored on the state after inputs 0..j-1 (the start state for j = 0).
 *                   z = Why*h + by summed as lstm_hip_generate sums it.  With con: z_m = -inf where next[q][m] is forbidden, q
 *                   the state byte j stands in (start_state[s] advanced over bytes 0..j-1); everything below sees the mask.
 *                   Without LSTM_HIP_STABLE_SOFTMAX: e_m = expf(z_m), s = the sequential float sum of e in index order,
 *                   p_m = e_m / s, surprisal(b) = -log2f(p_b).  With it: e_m = expf(z_m - max z), s and p as before,
 *                   surprisal(b) = log2f(s) + (max z - z_b) * 1.44269504088896341f.
 *        surprisal  surprisal(x).  bits[s] adds (double)surprisal in text order: with first = 0 and no constraint these are the
 *                   additions of lstm_hip_generate's prompt bits, so the two agree bit for bit.
 *        entropy    -(sequential float sum in index order of p_m * log2f(p_m), a term being 0 where p_m is not above 0).
 *        rank       #{i : z_i > z_x} + #{i < x : z_i == z_x}: rule 1 of lstm_hip_generate_ex; 0 = the model's first guess.
 *        top        top_byte[.. * top_n + r] is the byte of rank r < top_n, top_bits its surprisal.  Under a constraint the
 *                   ranks from A_q on are the forbidden bytes in index order, with +inf bits.
 *        chaining   a text scored in pieces -- every call after the first with first = 1, h0 / c0 = the h_out / c_out and
 *                   start_state = the end_state of the call before -- gives the entries of the one long call, bit for bit.
 *        end_state  the state after the stream's last byte (start_state[s] for an empty stream).
 *      Without LSTM_HIP_STABLE_SOFTMAX expf may overflow: the float outputs of that position are then unspecified, ranks and
 *      bytes are still in 0..255 and nothing faults.  Only the fp32 parameters are read (a bf16 handle scores as an fp32 one;
 *      LSTM_HIP_FAST_MATH applies to the recurrence only); gradients, optimizer state, window, cursors and carry are untouched.
 *      The loop runs max length + 1 head launches and max length recurrence steps, with no readback inside it.
 *      LSTM_HIP_EINVAL (the handle stays usable): opt NULL, opt->size or out->size wrong, first not 0 or 1, top_n outside 0..8,
 *      top_byte or top_bits given with top_n = 0, start_state or end_state given with con NULL, streams outside 1..4096,
 *      offsets missing, not starting at 0 or decreasing, text NULL with bytes to score, the table refusals of
 *      lstm_hip_generate_constrained, a byte its table rejects (the message names the stream and the offset).
 *      LSTM_HIP_EHIP: the device refused the kernel's LDS request. */
typedef struct lstm_hip_scoring {
    uint32_t size;      /* sizeof(lstm_hip_scoring); anything else: LSTM_HIP_EINVAL */
    int32_t  first;     /* 0: byte 0 of a stream is an input only (as the prompt bits of lstm_hip_generate);
                           1: it is scored too, from the stream's start state */
    int32_t  top_n;     /* 0..8: alternatives recorded per scored byte */
    const lstm_hip_constraint *con;  /* may be NULL */
} lstm_hip_scoring;
typedef struct lstm_hip_scores {     /* outputs; every pointer may be NULL.  total = text_off[streams] */
    uint32_t size;      /* sizeof(lstm_hip_scores); anything else: LSTM_HIP_EINVAL */
    float   *surprisal;  /* [total]          bits of the byte that stands at that position of `text` */
    float   *entropy;    /* [total]          bits, of the distribution that byte was scored under */
    uint8_t *rank;       /* [total]          0 = the byte was the model's first guess */
    uint8_t *top_byte;   /* [total * top_n]  the bytes of rank 0..top_n-1 */
    float   *top_bits;   /* [total * top_n]  their surprisals */
    double  *bits;       /* [streams]        sum of the stream's surprisals */
    int32_t *end_state;  /* [streams]        only with con */
} lstm_hip_scores;
int lstm_hip_score(lstm_hip_t *h, int32_t streams, const uint8_t *text, const uint64_t *text_off, const float *h0,
                   const float *c0, const lstm_hip_scoring *opt,
                   const int32_t *start_state /* [streams], may be NULL: all 0; only with con */,
                   const lstm_hip_scores *out /* may be NULL: nothing but h_out / c_out is wanted */, float *h_out,
                   float *c_out);
/* the same call under a mix with other models: the block, the rule and the refusals stand at lstm_hip_generate_guided */
int lstm_hip_score_guided(lstm_hip_t *h, int32_t streams, const uint8_t *text, const uint64_t *text_off, const float *h0,
                          const float *c0, const lstm_hip_scoring *opt, const int32_t *start_state, const lstm_hip_scores *out,
                          float *h_out, float *c_out, const lstm_hip_guidance *gd /* NULL: exactly lstm_hip_score */);

/* ---- held-out bits of many texts at the trainer's forward speed: the training window's forward
 *      path (recurrence, time-batched Why*H, softmax launch) run forward-only, on a cached internal handle of
 *      `lanes` columns and LSTM_HIP_EVAL_STEPS steps, in a device loop with no readback.  Stream s is
 *      text[text_off[s] .. text_off[s+1]) with L bytes, streams >= 1; h0 / c0 / h_out / c_out are N x streams as in
 *      lstm_hip_generate (NULL = zeros / not wanted).
 *        rule       a stream has n = max(L - 1, 0) steps; step j (0-based) feeds byte j and scores byte j + 1 on the state
 *                   after inputs 0..j.  Byte 0 is never scored (as lstm_hip_eval_bits, and first = 0 of lstm_hip_score); the
 *                   last byte is scored but never fed.  Bytes j + 1 < skip[s] are fed but not scored (warm-up); skip 0 and
 *                   skip 1 mean the same.  The arithmetic is a training window's: the handle's forward recurrence in fp32,
 *                   z = Why*h for all steps of a window in one product, the softmax launch's surprisal.
 *        surprisal  indexed like text, as lstm_hip_score's: entry text_off[s] + i belongs to byte i of stream s and is the
 *                   float the softmax launch wrote for it, -log2f(p), or the log-sum-exp form under LSTM_HIP_STABLE_SOFTMAX;
 *                   0.0f for every unscored byte (byte 0, bytes below skip[s]).
 *        bits       bits[s] adds (double)surprisal over the stream's scored bytes in text order.
 *        h_out      the state after the stream's last FED byte, byte L - 2 (for L <= 1 the start state).  This is NOT
 *                   lstm_hip_score's "state after the last byte": the last byte has not been fed.
 *        chaining   a text evaluated in pieces: the next piece starts with byte L - 1 of this one AGAIN (pieces overlap by
 *                   one byte) and takes h0 / c0 = this piece's h_out / c_out.
 *        plan       lstm_hip_eval_plan, host only (no handle, no device), is the schedule the call runs.  Window k of a stream
 *                   holds its steps 128k .. 128k + 127 in rows 1..128 (both indices -1 past the end); a stream needs
 *                   ceil(n / 128) windows; one with n = 0 gets no lane (lane_of = first_window = -1).  Streams are placed in
 *                   index order, each on the lane whose next free window is lowest (lowest lane on ties), in consecutive
 *                   windows there.  Column 0 of a stream's first window is its h0 / c0 column, column 0 of every later window
 *                   column 128 of that lane's window before; an idle lane has empty rows.  Returns the number of windows
 *                   (the largest next free window, >= 0); LSTM_HIP_EINVAL for lanes outside 1..4096, streams < 1, offsets
 *                   missing, not starting at 0 or decreasing.  lane_of / first_window: [streams], either may be NULL.
 *      opt NULL or lanes = 0: the handle's B lanes.  The internal handle has the parent's internal width and its
 *      LSTM_HIP_FAST_MATH, LSTM_HIP_STABLE_SOFTMAX and LSTM_HIP_STEP_KERNELS, is always fp32 (a bf16 handle evaluates from its
 *      fp32 parameters, like every inference call), is remade when `lanes` changes and freed with the handle.  Per window: one
 *      launch that builds the window, the forward path (a width on the per-step engine: one launch per step), one launch that
 *      folds the surprisals.  The block lstm_hip_set_inference_source names is copied in at every call; weight drop is never
 *      applied.  Nothing else of the handle is read and nothing is written: parameters, gradients, optimizer state and counts,
 *      window, rings, cursors, carry, averaging and weight-drop state, clip norms and kernel statistics stay as they were.
 *      elapsed_ms (may be NULL): HIP-event time of the device loop.
 *      LSTM_HIP_EINVAL (the handle stays usable, nothing is launched): opt->size wrong, lanes outside 0..4096, streams < 1,
 *      offsets missing, not starting at 0 or decreasing, text NULL with bytes to read. */
#define LSTM_HIP_EVAL_STEPS 128          /* steps per evaluation window */
typedef struct lstm_hip_eval_opt {
    uint32_t size;   /* sizeof(lstm_hip_eval_opt); anything else: LSTM_HIP_EINVAL */
    int32_t  lanes;  /* streams evaluated side by side; 0: the handle's B; else 1..4096 */
} lstm_hip_eval_opt;
int64_t lstm_hip_eval_plan(int32_t lanes, int32_t streams, const uint64_t *text_off, int32_t *lane_of, int64_t *first_window);
int lstm_hip_eval_texts(lstm_hip_t *h, int32_t streams, const uint8_t *text, const uint64_t *text_off,
                        const float *h0, const float *c0,        /* N x streams, NULL = zeros */
                        const uint64_t *skip,                    /* [streams], NULL = none */
                        const lstm_hip_eval_opt *opt,            /* NULL: lanes = the handle's B */
                        double *bits,                            /* [streams], may be NULL */
                        float *surprisal,                        /* [text_off[streams]], may be NULL */
                        float *h_out, float *c_out,              /* N x streams, may be NULL */
                        float *elapsed_ms);                      /* may be NULL */

/* ---- hidden states of many texts: pooled, last and picked positions.  lstm_hip_eval_texts' engine
 *      -- the same cached internal handle, the same device loop without readback, the same arithmetic (the handle's forward
 *      recurrence in fp32, from the fp32 block lstm_hip_set_inference_source names; weight drop is never applied) -- read for
 *      what the model computed, not for what it predicted.  Stream s is text[text_off[s] .. text_off[s+1]) with L bytes;
 *      h0 / c0 / skip / opt are lstm_hip_eval_texts'.
 *        rule       a stream has n = L steps, NOT lstm_hip_eval_texts' L - 1: there the last byte is scored and never fed, and
 *                   an embedding must have seen the whole text.  Step j feeds byte j; its target is byte j + 1 where
 *                   j + 1 < L and j + 1 >= skip[s], else the step has no target.  "Position i" is the state after inputs
 *                   0..i, indexed like text: text_off[s] + i.
 *        last_*     position L - 1; for L = 0 the start state.  skip does not affect it.
 *        pool       positions max(skip[s], 0) .. L - 1; count[s] is their number, max(L - skip[s], 0).
 *        mean_*     (double) of every pooled float is added in text order into one double per element, carried across the
 *                   stream's windows in device memory; the result is (float)(sum / (double)count).
 *        max_*      the largest pooled value, exactly one of the floats.
 *                   An empty pool gives mean = max = +0.0f.  With non-finite states which value comes out is unspecified;
 *                   nothing faults.
 *        picked_*   pick[0 .. npick) are positions, strictly increasing; column k of picked_h / picked_c (N x npick) is the
 *                   state at position pick[k], whether or not it lies below skip.
 *        bits       lstm_hip_eval_texts' figure for the same stream and skip within its tolerance (not bit-equal: the
 *                   placement differs by the extra step).
 *        plan       the schedule is lstm_hip_text_plan(128, lanes, streams, off') with off'[s] = text_off[s] + s: every stream
 *                   counted one byte longer, which gives n = L from the planner's n = L' - 1.  Window k of a stream holds its
 *                   positions 128k .. 128k + 127 in rows 1..128; column 0 and later windows follow lstm_hip_eval_texts; a
 *                   stream with L = 0 gets no lane, its outputs are written before the loop (last = start state, count 0).
 *      Every pointer of `out` may be NULL (not wanted).  All state outputs are N x streams (picked: N x npick), column s =
 *      stream s, as h_out elsewhere.  Per window: one launch that builds the window, the forward path, one launch that folds
 *      pools, picks, last states and bits; the two launches have no kernel statistics row.  What of the handle is touched is
 *      lstm_hip_eval_texts' paragraph word for word: the block the inference source names is copied in at every call, nothing
 *      else is read and nothing is written.  elapsed_ms (may be NULL): HIP-event time of the device loop.
 *      LSTM_HIP_EINVAL (the handle stays usable, nothing is launched): everything lstm_hip_eval_texts refuses, in its words
 *      under the name embed_texts; out NULL or of the wrong size; npick < 0; pick NULL with npick > 0; a pick >=
 *      text_off[streams] or not above the one before it; picked_* given with npick == 0, or npick > 0 with neither given; a
 *      picked block (internal width x npick x 4 bytes x sources) above 1 GiB. */
typedef struct lstm_hip_embedding {   /* outputs; every pointer may be NULL */
    uint32_t size;                    /* sizeof(lstm_hip_embedding); anything else: LSTM_HIP_EINVAL */
    float   *mean_h, *max_h, *last_h; /* N x streams each */
    float   *mean_c, *max_c, *last_c; /* the same of the cell state */
    int64_t *count;                   /* [streams] pooled positions */
    double  *bits;                    /* [streams] as lstm_hip_eval_texts' bits */
    float   *picked_h, *picked_c;     /* N x npick */
} lstm_hip_embedding;
int lstm_hip_embed_texts(lstm_hip_t *h, int32_t streams, const uint8_t *text, const uint64_t *text_off,
                         const float *h0, const float *c0,        /* N x streams, NULL = zeros */
                         const uint64_t *skip,                    /* [streams], NULL = none */
                         const lstm_hip_eval_opt *opt,            /* NULL: lanes = the handle's B */
                         const uint64_t *pick, int64_t npick,     /* may be NULL / 0 */
                         const lstm_hip_embedding *out, float *elapsed_ms);

/* ---- training on separate texts, each from its zero state: the trio set_text / set_cursors /
 *      train_windows for texts.  Stream s is text[text_off[s] .. text_off[s+1]) with L bytes; a stream has
 *      n = max(L - 1, 0) steps, step j feeds byte j and has byte j + 1 as its target.
 *        plan       lstm_hip_text_plan, host only (no handle, no device), is lstm_hip_eval_plan's rule with `steps` (>= 1) rows
 *                   per window in place of 128: window k of a stream holds its steps k*steps .. k*steps + steps - 1 in rows
 *                   1..steps; a stream needs ceil(n / steps) windows; one with n = 0 gets no lane (lane_of = first_window =
 *                   -1).  Streams are placed in index order, each on the lane whose next free window is lowest (lowest lane on
 *                   ties), in consecutive windows there.  Returns the number of windows; LSTM_HIP_EINVAL for steps < 1 and
 *                   for everything lstm_hip_eval_plan refuses.  lstm_hip_eval_plan(...) is lstm_hip_text_plan(128, ...).
 *        set        lstm_hip_set_train_texts uploads the texts, the offsets and the tables of
 *                   lstm_hip_text_plan(S - 1, B, ...), zeroes the per-stream bits and sets next = 0.  The memory stays with
 *                   the handle; a second set replaces the first; streams = 0 with both pointers NULL drops it.
 *                   lstm_hip_get_train_texts returns the plan's length and the next window to run (either may be NULL).
 *        train      lstm_hip_train_text_windows runs windows next .. next + count - 1 of the plan, one update each; how a
 *                   plan is cut into calls shows in no result.  Per window:
 *                     window    one launch for all B lanes.  Row t (1..S-1) of a lane that holds step j of its stream gets
 *                               xi = byte j, ti = byte j + 1 (row 0 holds the step before row 1's where the text has one, as
 *                               a slid window does; it is never read); every other row -- past a text's end, an idle lane -- gets xi = -1 and no target
 *                               (ti = -1).  Column 0 of H and C is zero for a lane that starts a text in this window and for
 *                               an idle lane; for a lane that continues its text it is column S-1 of the handle's state,
 *                               read where lstm_hip_train_windows reads its carry (a call in between that rewrites that
 *                               column changes the result, as it would there).  The ring form of the window and its head are
 *                               written too, so a later lstm_hip_train_windows or lstm_hip_get_window sees a whole window.
 *                     forward   the handle's own training forward path on the engine its plan chose, weight drop included
 *                               when it is on.
 *                     targets   a column with ti < 0 gets dy = 0 and a surprisal of 0 HERE (in every other call it gets
 *                               dy = probs, the reference's rule).  For a row past a text's end dy = 0 and the gradients
 *                               arriving from later rows are 0 by induction from the window's end, so the row adds exactly
 *                               zero to every gradient, on every backward form.
 *                     loss      losses[i] (may be NULL) is the LSTM_HIP_LOSS_ALL_STEPS_BITS figure of the window: rows without
 *                               a target add 0, the sum is still divided by the global batch.  Each stream's surprisals are
 *                               added in double, in text order, into its entry of the bits block:
 *                               lstm_hip_get_train_texts_bits returns the [streams] prequential bits, every byte scored
 *                               under the parameters its window had before its update.
 *                     update    backward, clip if set, the handle's optimizer step, exactly as the adaptive train pass runs
 *                               them: Adam's t, the averaging counts and the weight-drop index advance once per window, and
 *                               with clipping on lstm_hip_get_grad_norms afterwards returns the call's `count` norms.
 *                   After the call the handle holds the last window (states, gates, probabilities, gradient block), as after
 *                   lstm_hip_train_windows.  Text, cursors, stride and loss mode are neither read nor written.
 *                   elapsed_ms (may be NULL): HIP-event time of the device loop.
 *      Refusals (the handle stays usable, nothing is launched).  LSTM_HIP_ESTATE: no texts set (train, get, bits); a
 *      communicator on the handle (every rank would have to run the same number of windows); a loss mode other than
 *      LSTM_HIP_LOSS_ALL_STEPS_BITS.  LSTM_HIP_EINVAL: count < 0 or past the plan's end; learning_rate negative or not
 *      finite; for set: streams < 1, more than 4096 lanes (B), offsets missing, not starting at 0 or decreasing, text NULL
 *      with bytes to read.
 *
 *      Weights per byte: completion-only training, importance weights.
 *      lstm_hip_set_train_texts_weighted is lstm_hip_set_train_texts with a float per byte: weight[text_off[s] + i] is the
 *      weight of byte i of stream s AS A TARGET, so the weight of step j (feeds byte j, target byte j + 1) is entry j + 1,
 *      indexed like the surprisal output of lstm_hip_eval_texts.  Byte 0 of a stream is never a target: its entry is
 *      validated and never used.  The weights are uploaded once with the texts and stay with the handle.
 *      lstm_hip_set_train_texts(h, ...) is this call with weight = NULL, which is the unweighted set above: its launches and
 *      its bytes.  streams = 0 with all three pointers NULL drops the texts; a second set replaces the first, weighted or
 *      not; plan, placement, next = 0 and the zeroed bits are the same.  With weights set a window is everything above, and
 *        dy         a column with a target k and the weight w gets dy = w * (p - e_k): one fp32 multiply per element behind
 *                   the subtraction.  A column with w == 0 gets dy = +0.0f in every element and a surprisal of 0.0f BY
 *                   SELECTION, not by multiplication, so a context byte whose p is NaN or inf poisons nothing.  A column
 *                   without a target (ti < 0) is as above: dy = 0, surprisal 0.  A byte of weight 0 inside a text is NOT a
 *                   text's end: its row adds nothing of its own, and the gradients of the later rows flow back through its
 *                   state -- it is context.
 *        loss       the column's figure is w * surprisal, one fp32 multiply of the float the unweighted window writes
 *                   (-log2f(p_k), or the log-sum-exp form under LSTM_HIP_STABLE_SOFTMAX).  losses[i] and
 *                   lstm_hip_get_train_texts_bits are therefore the WEIGHTED figures, folded by the same launches in the
 *                   same order; nothing is divided by the weights' sum (callers divide).  The probabilities
 *                   (lstm_hip_get_activations) stay the plain p.
 *        identity   w == 1.0f everywhere gives the unweighted call's bytes: a multiply by 1 is exact.
 *        gradients  dby = rowsum(dy), dWhy, the clip norm and the update see the weighted dy; nothing else changes.  A window
 *                   whose weights are all 0 still runs one update (the counters advance); with Adagrad its parameters and
 *                   memory come out byte-identical.
 *      The softmax launch of a weighted window has its own statistics row, softmax_loss_dy_weighted (softmax_loss_dy_text
 *      stays 0).  The window's weights are scratch: they show in no later call.
 *      Refused with LSTM_HIP_EINVAL, nothing launched, a previous set kept: an entry of weight[0 .. text_off[streams]) that
 *      is negative, NaN or infinite (the message names the stream and the byte's offset in it), and everything
 *      lstm_hip_set_train_texts refuses, in its words.  lstm_hip_train_text_windows refuses what it refuses above. */
int64_t lstm_hip_text_plan(int32_t steps, int32_t lanes, int32_t streams, const uint64_t *text_off, int32_t *lane_of,
                           int64_t *first_window);
int lstm_hip_set_train_texts(lstm_hip_t *h, int32_t streams, const uint8_t *text, const uint64_t *text_off);
int lstm_hip_set_train_texts_weighted(lstm_hip_t *h, int32_t streams, const uint8_t *text, const uint64_t *text_off,
                                      const float *weight /* [text_off[streams]], indexed like text; NULL: unweighted */);
int lstm_hip_get_train_texts(lstm_hip_t *h, int64_t *windows, int64_t *next);   /* plan length, next window to run */
int lstm_hip_train_text_windows(lstm_hip_t *h, int64_t count, double learning_rate, double *losses, float *elapsed_ms);
int lstm_hip_get_train_texts_bits(lstm_hip_t *h, double *bits /* [streams] */);

/* ---- arithmetic coding of bytes with the model.  Stream s is text[text_off[s] .. text_off[s+1]),
 *      1 <= streams <= 4096, each coded on its own from h = c = 0 (empty streams allowed: their code is empty).
 *        which bytes   EVERY byte, the first one included: byte j is coded with the distribution of the state after inputs
 *                      0..j-1 (for j = 0 the zero state, so z = by).  Unlike lstm_hip_eval_bits and the prompt bits of
 *                      lstm_hip_generate, which never score byte 0.
 *        distribution  z = Why*h + by summed as lstm_hip_generate sums it (sequentially in k, no contraction), then
 *                      p_m = expf(z_m - max z) / sum_k expf(z_k - max z): ALWAYS max-shifted, whatever
 *                      LSTM_HIP_STABLE_SOFTMAX says.  Only the fp32 parameters are read (a bf16 handle codes as an fp32 one);
 *                      LSTM_HIP_FAST_MATH applies to the recurrence as in lstm_hip_generate.
 *        quantisation  q_m = 1 + (uint32)(p_m * 65024.0f) (truncated), T = sum_m q_m (256 <= T <= 65281 < 2^16),
 *                      cum_m = sum_{k<m} q_k.  Every byte keeps q >= 1, so any input can be coded.
 *        coder         the carryless 32-bit range coder (Subbotin: TOP = 2^24, BOT = 2^16), 4-byte flush; a code never
 *                      rewrites a byte it has written.  The decoder reads 0 for every byte past the end of its stream's
 *                      code and never reads outside it.
 *      code_bound(len) = 0 for len = 0, else 3*len + 4: the proven worst case of a stream's code (SIZE_MAX on overflow).
 *      A code decodes only with the same coder version (lstm_hip_coder_version, bumped whenever the logits, the softmax,
 *      the quantisation or the coder change), the same parameters and the same LSTM_HIP_FAST_MATH setting.
 *      Nothing of the handle is read or written except P (as lstm_hip_generate): gradients, optimizer state and step count,
 *      window, cursors, carry, loss mode and clip setting stay as they are.  Working memory stays with the handle.
 *      LSTM_HIP_EINVAL: streams outside 1..4096, offsets missing, not starting at 0 or decreasing, a null buffer where bytes
 *      are due, code_cap below the bound; and (never expected) a frequency total above 2^16 or a code past its bound on
 *      the device, in which case the call fails instead of returning a corrupt code. */
uint32_t lstm_hip_coder_version(void);
size_t lstm_hip_code_bound(uint64_t len);
/* code: code_cap >= sum_s lstm_hip_code_bound(len_s) bytes; the codes are written back to back and code_off[0..streams]
 * (out) delimits them.  bits (may be NULL): per stream, sum over its bytes of -log2(q/T) in double (the ideal length under
 * the quantised model).  trace (may be NULL): 3 uint32 per coded byte, in text order: cum, freq (= q), total (= T). */
int lstm_hip_encode(lstm_hip_t *h, int32_t streams, const uint8_t *text, const uint64_t *text_off, uint8_t *code,
                    uint64_t code_cap, uint64_t *code_off, double *bits, uint32_t *trace);
/* code[code_off[s] .. code_off[s+1]) is stream s's code; text_off gives each stream's decoded length (the lengths belong to
 * the container, not to the code) and where it goes in text.  A truncated code decodes to the requested length. */
int lstm_hip_decode(lstm_hip_t *h, int32_t streams, const uint8_t *code, const uint64_t *code_off, const uint64_t *text_off,
                    uint8_t *text);

/* ---- mixed coding: the static coder on a log-linear mix of several models' logits, the mixing
 *      weights fixed or learned online, per stream, from the bytes already coded.  Models 0..G are the main handle (index 0)
 *      and the G guides of gd in index order, G = 1..LSTM_HIP_MAX_GUIDES.  Everything lstm_hip_encode / lstm_hip_decode
 *      document holds, except what follows.
 *        states    every model starts every stream from h = c = 0 and is fed the coded bytes, each through its own W, U, b
 *                  in the same steps, exactly as the guides of lstm_hip_score_guided are fed: the block a guide's
 *                  lstm_hip_set_inference_source names is read, its LSTM_HIP_FAST_MATH applies to its recurrence, weight drop
 *                  never applies.  Nothing of a guide is written; model == h is allowed.
 *        logits    byte j of a stream is coded under z^k = Why_k*h_k + by_k of the states after inputs 0..j-1, each summed as
 *                  every head sums it (sequentially in the hidden index, multiply and add separately rounded, by added last).
 *        weights   a stream carries v[0..G], float, initialised to ((float)main_weight, (float)weight_1, .., (float)weight_G).
 *        mix       g_m = v_1*z^1_m, then g_m = g_m + v_k*z^k_m for k = 2.. in index order, then z'_m = v_0*z^0_m + g_m.  Every
 *                  multiply and every add is one fp32 operation, no contraction.
 *        table     exactly lstm_hip_encode's, built on z': p_m = expf(z'_m - max z') / s with s summed in index order,
 *                  q_m = 1 + (uint32)(p_m * 65024.0f), T = sum_m q_m, cum_m = sum_{k<m} q_k; the same coder, flush and
 *                  lstm_hip_code_bound.  Weights that have become NaN or infinite give the flat table (every q = 1) on both
 *                  sides, never a corrupt code.
 *        learning  (rate > 0) after byte x of the stream has been coded or decoded, the stream's last byte included:
 *                    d_m    = (float)q_m / (float)T - (m == x ? 1.0f : 0.0f)
 *                    grad_k = SUM_m d_m * z^k_m      the sequential float sum in index order of separately rounded products
 *                    v_k   <- v_k - (float)rate * grad_k              for k = 0..G, one multiply and one subtraction
 *                  d is the gradient of the byte's code length (in nats) under the QUANTISED table with respect to z', so
 *                  nothing transcendental enters the update and the decoder holds everything it needs when it needs it.
 *                  rate == 0 skips the update: v stays the call's weights, and the call is a fixed log-linear mix.
 *      gd == NULL: mx, w_out and w_trace must be NULL too, and the call is lstm_hip_encode / lstm_hip_decode exactly, with its
 *      scratch offsets, launches and bytes (those two are thin callers of the functions below).  mx == NULL with gd: rate 0.
 *      w_out (may be NULL): [streams][1+G], every stream's weights after its last byte (the call's weights for an empty
 *      stream); the decoder's equal the encoder's bit for bit.  w_trace (encoder, may be NULL): [total][1+G], the weights each
 *      byte was coded under, in text order; row 0 of a stream is the call's weights.  bits and trace are those of the mix.
 *      A code decodes only with the same lstm_hip_coder_version AND lstm_hip_mix_coder_version (bumped whenever the mix, the
 *      update or their order change a code), the same parameters and LSTM_HIP_FAST_MATH setting of every model in the same
 *      order, the same weights and the same rate.  The adaptive coders take no guides.
 *      LSTM_HIP_EINVAL (nothing is launched), after everything lstm_hip_encode / lstm_hip_decode refuse, in their words:
 *      everything a guidance block is refused for (lstm_hip_score_guided); a guide with a non-NULL h0, c0, h_out or c_out (the
 *      coders start every model from zero); mx->size wrong; rate negative, NaN or infinite; mx, w_out or w_trace without gd.
 *      LSTM_HIP_EHIP: the device refused an LDS request of the guides' kernel or of the mixed head (nothing of that step is
 *      launched). */
typedef struct lstm_hip_mix_coding {
    uint32_t size;              /* sizeof(lstm_hip_mix_coding); anything else: LSTM_HIP_EINVAL */
    double rate;                /* >= 0, finite; 0: fixed weights */
} lstm_hip_mix_coding;
uint32_t lstm_hip_mix_coder_version(void);
int lstm_hip_encode_mixed(lstm_hip_t *h, int32_t streams, const uint8_t *text, const uint64_t *text_off, uint8_t *code,
                          uint64_t code_cap, uint64_t *code_off, double *bits, uint32_t *trace, const lstm_hip_guidance *gd,
                          const lstm_hip_mix_coding *mx, float *w_out /* [streams][1+G], may be NULL */,
                          float *w_trace /* [total][1+G], may be NULL */);
int lstm_hip_decode_mixed(lstm_hip_t *h, int32_t streams, const uint8_t *code, const uint64_t *code_off, const uint64_t *text_off,
                          uint8_t *text, const lstm_hip_guidance *gd, const lstm_hip_mix_coding *mx,
                          float *w_out /* [streams][1+G], may be NULL */);

/* ---- adaptive coding: no checkpoint, the model trains on the bytes it has coded.  The handle's B
 *      streams are the coder's streams: stream s is text[text_off[s] .. text_off[s+1]), s < cfg.B (at most 4096).  With
 *      L = S - 1 and n_blocks = floor(min_s len_s / L) (lstm_hip_adaptive_blocks) both calls run this schedule:
 *        reset       window to empty columns, every state column of H and C to zero, coder state (h, c) of every stream to zero
 *        block k     code pass: bytes [kL, (k+1)L) of every stream, one step at a time, with the CURRENT fp32 parameters:
 *                    exactly lstm_hip_encode's rule per step (distribution, quantisation, coder; then the recurrence step on
 *                    the byte), the coder's (h, c) and range coder state carried over from block k-1; the image of U the
 *                    step kernel reads is remade from the parameters first.
 *                    train pass: one training window on those same bytes, exactly what lstm_hip_train_windows(1, lr) does
 *                    on a handle with lstm_hip_set_stride(S-1, S-1) whose cursors stood at text_off[s] + kL: window row t
 *                    holds target byte kL+t-1 and input byte kL+t-2 of the stream (empty before the stream's start), h[0],
 *                    c[0] <- column S-1, forward, loss, backward, clip if set, the handle's optimizer step with its own
 *                    step count.  The train pass runs on the engine the handle's plan chose.
 *        tail        the remaining bytes of every stream, coded, not trained on
 *        flush       4 bytes per non-empty stream, as lstm_hip_encode
 *      The decoder trains on the bytes it has decoded and so holds the encoder's parameters at every step, PROVIDED it starts
 *      from an identical handle: same config and flags, parameters, optimizer kind / numbers / state / step count, clip
 *      setting, learning_rate, and the same engine plan on the same kind of device (lstm_hip_plan_identity, the device's
 *      name and CU count: they decide the order of the training sums).  A code decodes only with the same
 *      lstm_hip_coder_version AND lstm_hip_adaptive_version (bumped when the schedule or anything it calls changes a code).
 *      The coder's (h, c) and the trainer's carry are two separate states.  Parameters that have gone non-finite keep
 *      coding (q = 1 for NaN), so a diverged run still round-trips; it stops compressing.
 *      Unlike the static calls these CHANGE the handle: parameters, gradients, optimizer state and step count, window, rings
 *      and carry are those of the last train pass (the model after the call is the adapted one).  The stride, loss mode,
 *      text and cursors set by the caller are neither read nor written: they stay as they are.  With clipping on,
 *      lstm_hip_get_grad_norms afterwards returns the n_blocks pre-clip norms of the call's train passes.
 *      code_cap, the offsets' checks and the device error bits are those of lstm_hip_encode / lstm_hip_decode;
 *      learning_rate must be finite and >= 0 (0 still runs the train pass); a handle with a communicator is LSTM_HIP_ESTATE.
 *      A truncated or damaged code decodes to the requested lengths; from the block after the first wrong byte on the decoder
 *      trains on other bytes than the encoder did, so every stream may differ from there (a container's checksum catches it). */
uint32_t lstm_hip_adaptive_version(void);
/* n_blocks of the schedule above; needs no device.  < 0 (LSTM_HIP_EINVAL): S < 2, B < 1, offsets missing, not starting at
 * 0 or decreasing */
int64_t lstm_hip_adaptive_blocks(int32_t S, int32_t B, const uint64_t *text_off);
/* bits (may be NULL): per stream, as lstm_hip_encode.  block_bits (may be NULL): n_blocks + 1 doubles, the ideal bits of all
 * streams in each block's code pass, the last one the tail's.  trace (may be NULL): as lstm_hip_encode. */
int lstm_hip_encode_adaptive(lstm_hip_t *h, const uint8_t *text, const uint64_t *text_off, double learning_rate,
                             uint8_t *code, uint64_t code_cap, uint64_t *code_off, double *bits, double *block_bits,
                             uint32_t *trace);
int lstm_hip_decode_adaptive(lstm_hip_t *h, const uint8_t *code, const uint64_t *code_off, const uint64_t *text_off,
                             double learning_rate, uint8_t *text);
/* a short text naming everything of the handle's engine plan that decides the order of a training window's sums (internal
 * width, the form of each recurrence, column grouping, split counts): two handles train to the same bits only when it, the
 * device name and the CU count agree.  cap >= 128 is enough. */
int lstm_hip_plan_identity(lstm_hip_t *h, char *buf, size_t cap);

/* ---- measurement.  With profiling on, every kernel launch is bracketed by HIP events on the
 *      handle's stream and per-kernel totals accumulate. */
int lstm_hip_synchronize(lstm_hip_t *h);
/* [forward, backward][2 workgroups][S][16] shader-clock stamps of the last window (LSTM_HIP_DEBUG_STAMPS handles only;
 * slot meanings: persistent.hip, FSTAMP / BSTAMP) */
int lstm_hip_debug_stamps(lstm_hip_t *h, uint64_t *out, size_t count);
int lstm_hip_set_profiling(lstm_hip_t *h, int32_t on);
/* rows 0 .. count-1; the last row, "counter_resets", is no kernel: its launches are the times a persistent recurrence
 * cleared its hand-off counters (every 2^26 launches, or LSTM_HIP_EPOCH_LIMIT), counted with profiling on or off, time 0 */
int lstm_hip_kernel_stat_count(lstm_hip_t *h);
int lstm_hip_kernel_stat(lstm_hip_t *h, int32_t idx, const char **name, int64_t *launches, double *total_ms);
int lstm_hip_reset_kernel_stats(lstm_hip_t *h);
/* device facts for the bench line: name (<= 63 chars), CU count, clock MHz */
int lstm_hip_device_info(int32_t device, char name[64], int32_t *cus, int32_t *clock_mhz);

#ifdef __cplusplus
}
#endif
#endif /* LSTM_HIP_H_ */
