// code_head.inc -- k_code_head and the range coder's device helpers (lstm_hip_encode / lstm_hip_decode).
// Included by kernels.hip inside namespace lstmk, at the place this text stood, and by the host emulations under tests/
// (tests/device_shim.h supplies the device words there).  Not a translation unit of its own.
// ------------------------------------------------------------------------------------------------
// code_head: one step of the model-driven range coder (lstm_hip_encode / lstm_hip_decode; DESIGN.md section 3.6).  Per
// stream s with more than t bytes, byte t is coded with the distribution of the state after t inputs:
//   z = Why*h + by        k_gen_head's sum: sequential in k, separate multiply and add, the same SB grouping rule
//   p_m = expf(z_m - max z) / s,  s = sum_m expf(z_m - max z) in index order (always max-shifted)
//   q_m = 1 + (uint32)(p_m * 65024.0f),  cum_m = sum_{k<m} q_k (exclusive scan over the 256 threads),  T = cum_256
// then the stream's owner lane runs one step of the carryless range coder (Subbotin; rc_* below) on (cum_x, q_x, T).
// The float work depends only on the stream's h, so the encoder (x = the text byte) and the decoder (x found in cum) see
// the same table at every step; `decode` is a runtime argument of one instantiation per SB.
// ------------------------------------------------------------------------------------------------
constexpr uint32_t RC_TOP = 1u << 24, RC_BOT = 1u << CODER_TOTAL_BITS;
constexpr int RC_MAX_SHIFTS = 3; // bytes one coding step can move (DESIGN.md section 3.6); a fourth is an error, never a loop
__device__ __forceinline__ void rc_put(const CodeHeadArgs &a, int s, CoderState &c, uint32_t byte) {
    const uint64_t beg = a.code_base[s], cap = a.code_base[s + 1] - beg;
    if (c.pos < cap) a.code[beg + c.pos] = (uint8_t)byte;
    else atomicOr(a.err, CODE_ERR_BOUND);
    c.pos++;
}
__device__ __forceinline__ uint32_t rc_get(const CodeHeadArgs &a, int s, CoderState &c) {
    const uint64_t beg = a.code_base[s], cap = a.code_base[s + 1] - beg;
    const uint32_t byte = c.pos < cap ? a.code[beg + c.pos] : 0u; // past the end of the stream's code: 0
    c.pos++;
    return byte;
}
// after low += cum * r; range = freq * r: shift out (encoder) or in (decoder) every settled top byte
__device__ __forceinline__ void rc_normalize(const CodeHeadArgs &a, int s, CoderState &c) {
    for (int n = 0;; n++) {
        if ((c.low ^ (c.low + c.range)) >= RC_TOP) { // top bytes differ
            if (c.range >= RC_BOT) break;
            c.range = (0u - c.low) & (RC_BOT - 1); // the carryless cut: end the interval at the next multiple of 2^16
        }
        if (n == RC_MAX_SHIFTS) {
            atomicOr(a.err, CODE_ERR_BOUND);
            break;
        }
        if (a.decode) c.code = (c.code << 8) | rc_get(a, s, c);
        else rc_put(a, s, c, c.low >> 24);
        c.low <<= 8;
        c.range <<= 8;
    }
}
// the coder step of one owner thread per stream, spread over the four waves (every other thread returns at once); PUBLISH:
// the byte coded or decoded goes to x_out[j] as well, for the threads that wait behind the step
template <int SB, bool PUBLISH>
__device__ __forceinline__ void code_owner_step(const CodeHeadArgs &a, const uint32_t (*tab)[260], int s0, int lane, int wave, long long t,
                                                uint32_t *x_out) {
    const int j = lane * 4 + wave;
    if (j >= SB || s0 + j >= a.streams) return;
    const int s = s0 + j;
    const uint64_t beg = a.text_off[s], len = a.text_off[s + 1] - beg;
    if ((unsigned long long)t >= len) {
        a.x_next[s] = -1;
        return;
    }
    CoderState c;
    if (t == 0) {
        c.low = 0;
        c.range = 0xFFFFFFFFu;
        c.code = 0;
        c.pad = 0;
        c.pos = 0;
        if (a.decode)
            for (int i = 0; i < 4; i++) c.code = (c.code << 8) | rc_get(a, s, c);
    } else
        c = a.state[s];
    const uint32_t T = tab[j][256];
    int x = a.decode ? 0 : a.text[beg + t];
    if (T > RC_BOT) atomicOr(a.err, CODE_ERR_TOTAL); // (cannot happen, DESIGN.md section 3.6; the call fails)
    else {
        c.range /= T; // >= 1: range >= 2^16 >= T after every normalisation
        if (a.decode) {
            uint32_t v = (c.code - c.low) / c.range;
            if (v >= T) v = T - 1; // (a damaged or truncated code: still some byte, never outside the table)
            int lo = 0, hi = 256; // tab[j][lo] <= v < tab[j][hi]; cum is strictly increasing (every q >= 1)
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (tab[j][mid] <= v) lo = mid;
                else hi = mid;
            }
            x = lo;
        }
        const uint32_t cum = tab[j][x], freq = tab[j][x + 1] - cum;
        c.low += cum * c.range;
        c.range *= freq;
        rc_normalize(a, s, c);
        if (a.decode) a.text[beg + t] = (uint8_t)x;
        else {
            if (a.trace) {
                uint32_t *tr = a.trace + 3 * (size_t)(beg + t);
                tr[0] = cum;
                tr[1] = freq;
                tr[2] = T;
            }
            if (a.bits) a.bits[s] += -log2((double)freq / (double)T);
            if ((unsigned long long)t + 1 == len) { // flush: the four bytes of low
                for (int i = 0; i < 4; i++) {
                    rc_put(a, s, c, c.low >> 24);
                    c.low <<= 8;
                }
                a.code_len[s] = c.pos;
            }
        }
    }
    a.state[s] = c;
    a.x_next[s] = x;
    if constexpr (PUBLISH) x_out[j] = (uint32_t)x;
}
// MIX (code_head_mixed; lstm_hip_encode_mixed / lstm_hip_decode_mixed, DESIGN.md section 3.25): the table is built on the mix
//   z' = v_0 * z^0 + g,   g = v_1 * z^1, then g = g + v_k * z^k in index order (one multiply, one add, each rounded)
// of the main model's logits z^0 and the guides' z^k (a.zk, written by k_guide_logits ahead of this launch) under the stream's
// own weights v (a.v).  With rate != 0 the weights then take one step on the byte x just coded, from what both sides hold:
//   d_m = (float)q_m / (float)T - (m == x ? 1.0f : 0.0f),   grad_k = sum_m d_m * z^k_m,   v_k = v_k - rate * grad_k
// the sum sequential in m, every product rounded on its own.  Thread m stages its logit of every member behind hs
// (zs: [SB][1 + G][257] floats, the odd stride keeps the summing threads on different banks), the owner lane publishes x
// through s_wave, thread m then writes d_m over the dead table, and one thread per (stream, model) pair sums that pair.  No
// thread returns before the last barrier: the owner's step is a call here, not the end of the kernel.
template <int SB, bool MIX = false>
__global__ __launch_bounds__(256) void k_code_head(CodeHeadArgs a, long long t) {
    HEAD_DYNAMIC_LDS(float, hs); // [N][SB]; MIX: then zs
    __shared__ uint32_t tab[SB][260]; // the logits, then expf terms (as float), then cum_0 .. cum_256
    __shared__ float s_zmax[SB], s_sum[SB];
    __shared__ uint32_t s_wave[4][SB];
    const int m = threadIdx.x, N = a.N, s0 = blockIdx.x * SB, lane = m & 63, wave = m >> 6;
    bool act[SB]; // (the same in every thread)
    bool need = false;
    [[maybe_unused]] uint32_t qm[SB]; // MIX: q_m of every stream, kept for the update
#pragma unroll
    for (int j = 0; j < SB; j++) {
        const int s = s0 + j;
        act[j] = s < a.streams && (unsigned long long)t < a.text_off[s + 1] - a.text_off[s];
        need |= act[j];
    }
    if (need) { // (uniform)
        float *ps = reinterpret_cast<float *>(&tab[0][0]);
        for (int i = m; i < N * SB; i += 256) {
            const int k = i / SB, j = i - k * SB;
            hs[i] = s0 + j < a.streams ? a.H[(size_t)(s0 + j) * N + k] : 0.0f;
        }
        __syncthreads();
        float y[SB];
#pragma unroll
        for (int j = 0; j < SB; j++) y[j] = 0.0f;
        for (int k0 = 0; k0 < N; k0 += 16) { // as k_gen_head: 16 loads in flight, the additions in k order
            float wv[16];
#pragma unroll
            for (int i = 0; i < 16; i++) wv[i] = a.Why[(size_t)(k0 + i) * 256 + m];
#pragma unroll
            for (int i = 0; i < 16; i++)
#pragma unroll
                for (int j = 0; j < SB; j++) y[j] += wv[i] * hs[(k0 + i) * SB + j];
        }
        const float bym = a.by[m];
#pragma unroll
        for (int j = 0; j < SB; j++) {
            y[j] = y[j] + bym; // the logit z
            if constexpr (MIX)
                if (act[j]) { // the members to zs; z becomes the mix under the stream's weights
                    const int G = a.nguides;
                    const size_t s = (size_t)(s0 + j);
                    const float *vj = a.v + s * (G + 1);
                    float *zj = hs + (size_t)N * SB + (size_t)j * (G + 1) * 257;
                    zj[m] = y[j];
                    float g = 0.0f;
                    for (int k = 1; k <= G; k++) {
                        const float zk = a.zk[(s * G + (k - 1)) * 256 + m];
                        zj[k * 257 + m] = zk;
                        const float term = vj[k] * zk;
                        g = k == 1 ? term : g + term;
                    }
                    y[j] = vj[0] * y[j] + g;
                }
            ps[j * 260 + m] = y[j];
        }
        __syncthreads();
        const bool own = m < SB && s0 + m < a.streams && (unsigned long long)t < a.text_off[s0 + m + 1] - a.text_off[s0 + m];
        if (own) { // max z of stream m (every order gives the same max)
            float best = ps[m * 260];
            for (int i = 1; i < 256; i++)
                if (ps[m * 260 + i] > best) best = ps[m * 260 + i];
            s_zmax[m] = best;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < SB; j++)
            if (act[j]) ps[j * 260 + m] = expf(y[j] - s_zmax[j]);
        __syncthreads();
        if (own) {
            float s = 0.0f;
            for (int i = 0; i < 256; i++) s += ps[m * 260 + i];
            s_sum[m] = s;
        }
        __syncthreads();
        // quantise; exclusive integer scan of q over the 256 threads (wave scan, then the wave totals through LDS)
        uint32_t q[SB], incl[SB];
#pragma unroll
        for (int j = 0; j < SB; j++) {
            const float v = ps[j * 260 + m] / s_sum[j] * 65024.0f; // p_m * 65024, in [0, 65024] (NaN: q = 1)
            q[j] = act[j] ? 1u + (v >= 1.0f ? (uint32_t)v : 0u) : 1u;
            int x = (int)q[j];
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int o = __shfl_up(x, d, 64);
                if (lane >= d) x += o;
            }
            incl[j] = (uint32_t)x;
        }
        if (lane == 63)
#pragma unroll
            for (int j = 0; j < SB; j++) s_wave[wave][j] = incl[j];
        __syncthreads(); // (also: every read of the expf terms is done)
#pragma unroll
        for (int j = 0; j < SB; j++) {
            uint32_t before = 0;
            for (int w = 0; w < wave; w++) before += s_wave[w][j];
            tab[j][m] = before + incl[j] - q[j];
            if (m == 255) tab[j][256] = before + incl[j];
            if constexpr (MIX) qm[j] = q[j];
        }
        __syncthreads();
    }
    code_owner_step<SB, MIX>(a, tab, s0, lane, wave, t, &s_wave[0][0]);
    if constexpr (MIX) {
        if (!need) return; // (uniform)
        __syncthreads(); // (also: every owner is done with the table)
        const int G1 = a.nguides + 1;
        float *ds = reinterpret_cast<float *>(&tab[0][0]);
        if (a.rate != 0.0f) { // (uniform)
#pragma unroll
            for (int j = 0; j < SB; j++)
                if (act[j]) {
                    const float T = (float)tab[j][256]; // (entry 256 is not overwritten)
                    ds[j * 260 + m] = (float)qm[j] / T - (m == (int)s_wave[0][j] ? 1.0f : 0.0f);
                }
            __syncthreads();
        }
        if (m < SB * G1) { // one thread per (stream, model) pair
            const int j = m / G1, k = m - j * G1, s = s0 + j;
            if (s < a.streams && (unsigned long long)t < a.text_off[s + 1] - a.text_off[s]) {
                const float v = a.v[(size_t)s * G1 + k];
                if (a.w_trace) a.w_trace[(size_t)(a.text_off[s] + t) * G1 + k] = v;
                if (a.rate != 0.0f) {
                    const float *zj = hs + (size_t)N * SB + (size_t)m * 257;
                    float grad = 0.0f;
                    for (int i = 0; i < 256; i++) grad += ds[j * 260 + i] * zj[i];
                    a.v[(size_t)s * G1 + k] = v - a.rate * grad;
                }
            }
        }
    }
}
