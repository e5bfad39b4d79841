// score_head.inc -- k_score_head, the per-step kernel of lstm_hip_score.
// Included by kernels.hip inside namespace lstmk, at the place this text stood, and by the host emulations under tests/
// (tests/device_shim.h supplies the device words there).  Not a translation unit of its own.
// ------------------------------------------------------------------------------------------------
// score_head: one step of lstm_hip_score (kernels.h; DESIGN.md section 3.11).  At step t every stream with more than t bytes
// hands byte t to the recurrence, and the byte is scored with the distribution of the state after t inputs unless it is byte
// 0 of a call with first = 0:
//   z = Why*h + by        k_gen_head's sum: sequential in k, separate multiply and add, the same SB grouping rule
//   a.gsum (guides)       z_m <- a.wmain * z_m + a.gsum[s * 256 + m] (lstm_hip_score_guided, DESIGN.md section 3.24: a multiply and
//                         an add rounded separately; k_guide_logits' sum of this step); with a.gsum null nothing is read
//   CONSTRAIN             z_m = -inf where a.ctab[q * 256 + m] is 0xFFFF, q = a.qpos[position]: everything below sees the mask
//   e_m = expf(z_m) (STABLE: expf(z_m - max z)), s = the sum of e in index order, p_m = e_m / s
//   surprisal(m) = -log2f(p_m) (STABLE: lse_surprisal(s, max z, z_m)): k_gen_head's prompt bits, term by term
//   entropy = -(the sum in index order of p_m * log2f(p_m), 0 where p_m is not above 0)
//   DETAIL                rank_m = #{z_i > z_m} + #{i < m: z_i == z_m} (256 broadcast reads, as the FILTER head ranks); the
//                         thread of rank r < top_n writes alternative r: its byte and surprisal(m)
// Thread m owns logit m of the workgroup's SB streams; the stream's owner lane makes the three serial passes (max, s, entropy);
// thread x, the text byte's, writes surprisal and rank and adds the surprisal to bits.  Nothing is read back and no array of
// the call is read after it was written, so the launches of a call only chain through H.
// ------------------------------------------------------------------------------------------------
template <int SB, bool STABLE, bool DETAIL, bool CONSTRAIN>
__global__ __launch_bounds__(256) void k_score_head(ScoreHeadArgs a, long long t) {
    HEAD_DYNAMIC_LDS(float, hs); // [N][SB]
    __shared__ float ps[SB][256]; // the logits, then the expf terms, then the entropy terms
    __shared__ float s_zmax[STABLE ? SB : 1], s_sum[SB];
    const int m = threadIdx.x, N = a.N, s0 = blockIdx.x * SB;
    bool act[SB]; // stream j scores a byte at this step (the same in every thread)
    int xs[SB];   // that byte
    bool need = false;
#pragma unroll
    for (int j = 0; j < SB; j++) {
        const int s = s0 + j;
        act[j] = false;
        xs[j] = 0;
        if (s >= a.streams) continue;
        const unsigned long long len = a.off[s + 1] - a.off[s];
        if ((unsigned long long)t < len) {
            xs[j] = a.text[a.off[s] + t];
            act[j] = t >= 1 || a.first;
        } else if ((unsigned long long)t == len) { // the state after the stream's last byte
            if (a.h_out)
                for (int k = m; k < N; k += 256) a.h_out[(size_t)s * N + k] = a.H[(size_t)s * N + k];
            if (a.c_out)
                for (int k = m; k < N; k += 256) a.c_out[(size_t)s * N + k] = a.C[(size_t)s * N + k];
        }
        need |= act[j];
    }
    const int jo = (m & 63) * 4 + (m >> 6); // one owner thread per stream, spread over the four waves
    const bool owner = jo < SB && s0 + jo < a.streams;
    if (owner) {
        const int s = s0 + jo;
        a.x_next[s] = (unsigned long long)t < a.off[s + 1] - a.off[s] ? (int)a.text[a.off[s] + t] : -1;
    }
    if (!need) return; // (uniform)
    [[maybe_unused]] bool banned[CONSTRAIN ? SB : 1]; // is byte m forbidden where stream j stands?  (loaded ahead of the product)
    if constexpr (CONSTRAIN) {
#pragma unroll
        for (int j = 0; j < SB; j++)
            banned[j] = act[j] && a.ctab[(size_t)a.qpos[a.off[s0 + j] + t] * 256 + m] == 0xFFFF;
    }
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
        if (a.gsum && act[j]) y[j] = a.wmain * y[j] + a.gsum[(size_t)(s0 + j) * 256 + m]; // (uniform test; two roundings)
        if constexpr (CONSTRAIN)
            if (banned[j]) y[j] = -INFINITY;
        ps[j][m] = y[j];
    }
    __syncthreads();
    [[maybe_unused]] int rank[DETAIL ? SB : 1]; // of this thread's logit, in 0..255
    if constexpr (DETAIL) {
#pragma unroll
        for (int j = 0; j < SB; j++) rank[j] = 0;
        // i outside, the streams inside: SB broadcast reads in flight, not SB * 8 (with the streams outside, as the FILTER head
        // ranks, the SB = 16 instantiation needs more than 256 registers).  Idle streams are ranked too; nothing reads that.
#pragma unroll 2
        for (int i = 0; i < 256; i++)
#pragma unroll
            for (int j = 0; j < SB; j++) {
                const float zi = ps[j][i];
                rank[j] += (zi > y[j]) | ((zi == y[j]) & (i < m));
            }
    }
    const bool own = owner && ((unsigned long long)t < a.off[s0 + jo + 1] - a.off[s0 + jo]) && (t >= 1 || a.first);
    if constexpr (STABLE) {
        if (own) { // max z (every order gives the same max)
            float best = ps[jo][0];
            for (int i = 1; i < 256; i++)
                if (ps[jo][i] > best) best = ps[jo][i];
            s_zmax[jo] = best;
        }
    }
    __syncthreads(); // (ps is overwritten below)
#pragma unroll
    for (int j = 0; j < SB; j++) {
        if (!act[j]) continue;
        if constexpr (STABLE) ps[j][m] = expf(y[j] - s_zmax[j]);
        else ps[j][m] = expf(y[j]);
    }
    __syncthreads();
    if (own) {
        float s = 0.0f;
        for (int i = 0; i < 256; i++) s += ps[jo][i];
        s_sum[jo] = s;
    }
    __syncthreads();
    float sp[SB]; // surprisal of byte m
#pragma unroll
    for (int j = 0; j < SB; j++) {
        sp[j] = 0.0f;
        if (!act[j]) continue;
        const float p = ps[j][m] / s_sum[j];
        if constexpr (STABLE) sp[j] = lse_surprisal(s_sum[j], s_zmax[j], y[j]);
        else sp[j] = -log2f(p);
        ps[j][m] = p > 0.0f ? p * log2f(p) : 0.0f;
    }
    __syncthreads();
    if (own && a.entropy) {
        float s = 0.0f;
        for (int i = 0; i < 256; i++) s += ps[jo][i];
        a.entropy[a.off[s0 + jo] + t] = -s;
    }
#pragma unroll
    for (int j = 0; j < SB; j++) {
        if (!act[j]) continue;
        const int s = s0 + j;
        const size_t pos = (size_t)(a.off[s] + t);
        if (m == xs[j]) {
            if (a.surprisal) a.surprisal[pos] = sp[j];
            if (a.bits) a.bits[s] += (double)sp[j];
            if constexpr (DETAIL)
                if (a.rank) a.rank[pos] = (uint8_t)rank[j];
        }
        if constexpr (DETAIL)
            if (rank[j] < a.top_n) {
                if (a.top_byte) a.top_byte[pos * a.top_n + rank[j]] = (uint8_t)m;
                if (a.top_bits) a.top_bits[pos * a.top_n + rank[j]] = sp[j];
            }
    }
}
