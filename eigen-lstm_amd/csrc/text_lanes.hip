// text_lanes.hip -- lane_window, eval_fold, embed_fold: the launches lstm_hip_eval_texts and lstm_hip_embed_texts put around
// the forward path (kernels.h; DESIGN.md sections 3.17 and 3.23).  A file of its own, apart from the training window's kernels.
//
// A stream sits on one lane and a lane holds one stream per window, so every element is independent and no two workgroups
// touch the same stream's element: grid-stride loops over lanes x rows for the indices, over lanes x N / 4 for the state
// columns in float4 (N % 16 == 0 and every column starts on a 16-byte boundary), and over the lanes for the bits, whose
// additions per stream are sequential in text order: one thread, one window after the other on the stream.
#include "kernels.h"

#include <algorithm>

namespace lstmk {

__global__ __launch_bounds__(256) void k_lane_window(LaneArgs a, long long w) {
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x, nth = (long long)gridDim.x * 256;
    const int32_t *slot = a.slot + w * a.lanes;
    for (long long i = tid; i < (long long)EVAL_STEPS * a.lanes; i += nth) {
        const int r = (int)(i / a.lanes), l = (int)(i - (long long)r * a.lanes); // row r + 1 of the window
        const int s = slot[l];
        int xv = -1, tv = -1;
        if (s >= 0) {
            const uint64_t o = a.off[s], len = a.off[s + 1] - o;
            const uint64_t j = (uint64_t)(w - a.first[s]) * EVAL_STEPS + r; // the step: feeds byte j; its target is byte j + 1
            if (j + 1 < len + a.feed_last) {
                xv = (int)a.text[o + j];
                if (j + 1 < len && j + 1 >= a.skip[s]) tv = (int)a.text[o + j + 1];
            }
        }
        a.xi[(size_t)(r + 1) * a.lanes + l] = xv;
        a.ti[(size_t)(r + 1) * a.lanes + l] = tv;
    }
    const int N4 = a.N / 4;
    float4 *H4 = reinterpret_cast<float4 *>(a.H), *C4 = reinterpret_cast<float4 *>(a.C);
    for (long long i = tid; i < (long long)a.lanes * N4; i += nth) {
        const int l = (int)(i / N4), q = (int)(i - (long long)l * N4);
        const int s = slot[l];
        if (s < 0) continue;
        if (w == a.first[s]) { // the stream's start state
            H4[i] = reinterpret_cast<const float4 *>(a.H0)[(size_t)s * N4 + q];
            C4[i] = reinterpret_cast<const float4 *>(a.C0)[(size_t)s * N4 + q];
        } else { // the lane's last column of the window before (another column than the one written)
            H4[i] = H4[(size_t)EVAL_STEPS * a.lanes * N4 + i];
            C4[i] = C4[(size_t)EVAL_STEPS * a.lanes * N4 + i];
        }
    }
}

// The bits of the lane's stream in window w, for the thread that holds the lane: steps j0 .. j0 + rows - 1 of the stream's
// L - 1 steps with a target are in this window, in rows 1 .. rows; those at or above skip are scored.  Adds (double)colloss of
// the scored rows to bits[s] in row order and scatters the floats to sur (may be null) at the scored byte's place.
__device__ __forceinline__ void lane_bits(const LaneArgs &a, long long w, long long l, int s, float *sur) {
    const uint64_t o = a.off[s], n = a.off[s + 1] - o - 1; // (a placed stream has at least one byte)
    const uint64_t j0 = (uint64_t)(w - a.first[s]) * EVAL_STEPS, skip = a.skip[s];
    if (j0 >= n) return; // (feed_last: the window of the last byte alone)
    const int rows = n - j0 < (uint64_t)EVAL_STEPS ? (int)(n - j0) : EVAL_STEPS;
    const float *__restrict__ col = a.colloss + l;
    double sum = a.bits[s];
    for (int r0 = 0; r0 < rows; r0 += 16) { // sixteen independent loads in flight (a row past the last: the last again, so
        float v[16];                        // that no load hides behind a branch), then their additions in row order
#pragma unroll
        for (int u = 0; u < 16; u++) v[u] = col[(size_t)(r0 + u < rows ? r0 + u : rows - 1) * a.lanes];
#pragma unroll
        for (int u = 0; u < 16; u++) {
            if (r0 + u >= rows || j0 + r0 + u + 1 < skip) continue; // past the end / fed, not scored
            sum += (double)v[u];
            if (sur) sur[o + j0 + r0 + u + 1] = v[u];
        }
    }
    a.bits[s] = sum;
}

__global__ __launch_bounds__(256) void k_eval_fold(EvalArgs a, long long w) {
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x, nth = (long long)gridDim.x * 256;
    const int32_t *slot = a.slot + w * a.lanes;
    for (long long l = tid; l < a.lanes; l += nth)
        if (slot[l] >= 0) lane_bits(a, w, l, slot[l], a.sur);
    if (a.Hout == nullptr && a.Cout == nullptr) return;
    const int N4 = a.N / 4;
    for (long long i = tid; i < (long long)a.lanes * N4; i += nth) {
        const int l = (int)(i / N4), q = (int)(i - (long long)l * N4);
        const int s = slot[l];
        if (s < 0) continue;
        const uint64_t n = a.off[s + 1] - a.off[s] - 1, j0 = (uint64_t)(w - a.first[s]) * EVAL_STEPS;
        if (n - j0 > (uint64_t)EVAL_STEPS) continue; // the stream goes on in the next window
        const size_t src = (size_t)(n - j0) * a.lanes * N4 + i; // the column of its last step
        if (a.Hout) reinterpret_cast<float4 *>(a.Hout)[(size_t)s * N4 + q] = reinterpret_cast<const float4 *>(a.H)[src];
        if (a.Cout) reinterpret_cast<float4 *>(a.Cout)[(size_t)s * N4 + q] = reinterpret_cast<const float4 *>(a.C)[src];
    }
}

__global__ __launch_bounds__(256) void k_embed_fold(EmbedArgs a, long long w, long long pick_lo, long long pick_hi) {
    __shared__ double s_sum[32][4];
    __shared__ float4 s_max[8][32];
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x, nth = (long long)gridDim.x * 256;
    const int32_t *slot = a.slot + w * a.lanes;
    for (long long l = tid; l < a.lanes; l += nth)
        if (slot[l] >= 0) lane_bits(a, w, l, slot[l], nullptr);
    const int N4 = a.N / 4;
    const size_t stride = (size_t)a.lanes * N4; // float4s per row of H / C
    // The pools.  A workgroup takes one (source, lane, 32 float4s of N) at a time as 8 chunks of 16 rows x 32 threads: every
    // thread issues the loads of its chunk at once, so all 128 rows of the lane are in flight together, and the double sums
    // then pass through the chunks in row order by way of LDS: the additions and their order are those of one thread
    // walking the rows.  The maximum needs no order.
    const int nsrc = (a.last[0] ? 1 : 0) + (a.last[1] ? 1 : 0), groups = (N4 + 31) / 32;
    const int qq = threadIdx.x & 31, c = threadIdx.x >> 5;
    const float ninf = -__builtin_inff();
    for (long long u = blockIdx.x; u < (long long)nsrc * a.lanes * groups; u += gridDim.x) {
        const int g = (int)(u % groups), l = (int)(u / groups % a.lanes);
        const int x = a.last[0] ? (int)(u / groups / a.lanes) : 1;
        const int s = slot[l];
        if (s < 0) continue; // (the same for the whole workgroup)
        const int q = g * 32 + qq;
        const bool live = q < N4;
        const uint64_t L = a.off[s + 1] - a.off[s], j0 = (uint64_t)(w - a.first[s]) * EVAL_STEPS, skip = a.skip[s];
        const bool ends = L - j0 <= (uint64_t)EVAL_STEPS, fresh = w == a.first[s];
        const int rows = ends ? (int)(L - j0) : EVAL_STEPS; // >= 1: the plan gave the stream this window
        const int r_lo = skip <= j0 ? 0 : skip - j0 < (uint64_t)rows ? (int)(skip - j0) : rows; // rows r_lo .. rows - 1 are pooled
        const uint64_t count = skip < L ? L - skip : 0;
        const size_t at = (size_t)s * N4 + q;
        const float4 *__restrict__ col = reinterpret_cast<const float4 *>(x ? a.C : a.H) + stride + (size_t)l * N4 + q; // row 1
        double *sum = a.sum[x] + at * 4;
        float4 *maxv = reinterpret_cast<float4 *>(a.maxv[x]) + at;
        float4 v[16] = {};
        if (live && 16 * c < rows && 16 * c + 16 > r_lo) { // the chunk holds a pooled row: all its loads at once, none behind a
#pragma unroll                                             // branch of its own (a row past the last live one: that one again)
            for (int k = 0; k < 16; k++) v[k] = col[(size_t)(16 * c + k < rows ? 16 * c + k : rows - 1) * stride];
        }
        float4 lastv = make_float4(0.0f, 0.0f, 0.0f, 0.0f), m0 = make_float4(ninf, ninf, ninf, ninf);
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        if (c == 0 && live) {
            if (ends) lastv = col[(size_t)(rows - 1) * stride]; // position L - 1
            if (!fresh) s0 = sum[0], s1 = sum[1], s2 = sum[2], s3 = sum[3], m0 = *maxv;
        }
        float4 m = make_float4(ninf, ninf, ninf, ninf);
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const int r = 16 * c + k;
            if (r < r_lo || r >= rows) continue; // below skip / past the stream's end
            m.x = v[k].x > m.x ? v[k].x : m.x;
            m.y = v[k].y > m.y ? v[k].y : m.y;
            m.z = v[k].z > m.z ? v[k].z : m.z;
            m.w = v[k].w > m.w ? v[k].w : m.w;
        }
        s_max[c][qq] = m;
        for (int p = 0; p < 8; p++) { // chunk p adds its rows behind chunk p - 1's
            if (c == p) {
                if (p > 0) s0 = s_sum[qq][0], s1 = s_sum[qq][1], s2 = s_sum[qq][2], s3 = s_sum[qq][3];
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    const int r = 16 * c + k;
                    if (r < r_lo || r >= rows) continue;
                    s0 += (double)v[k].x, s1 += (double)v[k].y, s2 += (double)v[k].z, s3 += (double)v[k].w;
                }
                s_sum[qq][0] = s0, s_sum[qq][1] = s1, s_sum[qq][2] = s2, s_sum[qq][3] = s3;
            }
            __syncthreads();
        }
        if (c == 0 && live) {
            s0 = s_sum[qq][0], s1 = s_sum[qq][1], s2 = s_sum[qq][2], s3 = s_sum[qq][3];
            m = m0;
            for (int k = 0; k < 8; k++) {
                const float4 o = s_max[k][qq];
                m.x = o.x > m.x ? o.x : m.x;
                m.y = o.y > m.y ? o.y : m.y;
                m.z = o.z > m.z ? o.z : m.z;
                m.w = o.w > m.w ? o.w : m.w;
            }
            if (!ends) { // the stream goes on in the next window
                sum[0] = s0, sum[1] = s1, sum[2] = s2, sum[3] = s3;
                *maxv = m;
            } else {
                float4 mean = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (count) {
                    const double n = (double)count;
                    mean = make_float4((float)(s0 / n), (float)(s1 / n), (float)(s2 / n), (float)(s3 / n));
                } else
                    m = mean;
                reinterpret_cast<float4 *>(a.mean[x])[at] = mean;
                *maxv = m;
                reinterpret_cast<float4 *>(a.last[x])[at] = lastv;
            }
        }
        __syncthreads(); // (the LDS is the next unit's)
    }
    for (long long i = tid; i < (pick_hi - pick_lo) * N4; i += nth) {
        const long long e = pick_lo + i / N4;
        const int q = (int)(i % N4);
        const int lane = a.picks[3 * e], row = a.picks[3 * e + 1], k = a.picks[3 * e + 2];
        const size_t src = ((size_t)row * a.lanes + lane) * N4 + q;
        if (a.picked[0]) reinterpret_cast<float4 *>(a.picked[0])[(size_t)k * N4 + q] = reinterpret_cast<const float4 *>(a.H)[src];
        if (a.picked[1]) reinterpret_cast<float4 *>(a.picked[1])[(size_t)k * N4 + q] = reinterpret_cast<const float4 *>(a.C)[src];
    }
}

static int window_blocks(long long work, int cus) {
    long long blocks = (work + 255) / 256; // one element per thread while the grid stays within the CUs: every element is a
                                           // chain of dependent loads (slot, offsets, byte), so more threads, not longer loops
    if (blocks > cus) blocks = cus;
    return blocks < 1 ? 1 : (int)blocks;
}
void lane_window(const LaneArgs &a, int64_t w, int cus, hipStream_t st) {
    const long long work = (long long)a.lanes * (EVAL_STEPS > a.N / 4 ? EVAL_STEPS : a.N / 4);
    hipLaunchKernelGGL(k_lane_window, dim3(window_blocks(work, cus)), dim3(256), 0, st, a, (long long)w);
}
void eval_fold(const EvalArgs &a, int64_t w, int cus, hipStream_t st) {
    const long long work = a.Hout || a.Cout ? (long long)a.lanes * (a.N / 4) : a.lanes;
    hipLaunchKernelGGL(k_eval_fold, dim3(window_blocks(work, cus)), dim3(256), 0, st, a, (long long)w);
}
void embed_fold(const EmbedArgs &a, int64_t w, int64_t pick_lo, int64_t pick_hi, int cus, hipStream_t st) {
    const long long N4 = a.N / 4, nsrc = (a.last[0] ? 1 : 0) + (a.last[1] ? 1 : 0);
    long long want = nsrc * a.lanes * ((N4 + 31) / 32); // the pools: a workgroup per (source, lane, 32 float4s)
    want = std::max(want, ((pick_hi - pick_lo) * N4 + 255) / 256);
    want = std::max(want, (long long)(a.lanes + 255) / 256);
    const long long cap = (long long)(cus > 0 ? cus : 1) * 8; // eight 256-thread workgroups fill a CU's 32 wave slots
    const int blocks = (int)(want < 1 ? 1 : want > cap ? cap : want);
    hipLaunchKernelGGL(k_embed_fold, dim3(blocks), dim3(256), 0, st, a, (long long)w, (long long)pick_lo, (long long)pick_hi);
}

} // namespace lstmk
