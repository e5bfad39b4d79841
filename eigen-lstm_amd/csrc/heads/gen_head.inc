// gen_head.inc -- gen_phase, gen_exists and k_gen_head, the per-step kernel of lstm_hip_generate.
// Included by kernels.hip inside namespace lstmk, at the place this text stood, and by the host emulations under tests/
// (tests/device_shim.h supplies the device words there).  Not a translation unit of its own.
// ------------------------------------------------------------------------------------------------
// gen_head: one step of the batched generator (lstm_hip_generate; lstm_hip_sample on the persistent engine is its
// streams = 1 case).  Per step the host launches this kernel on the state after t inputs, then one k_fwd_step over all
// streams with the inputs it chose.  Per stream s, with L = its prompt length:
//   t <  L          input prompt[t]; for t >= 1 (and bits requested) bits[s] += -log2 p(prompt[t]) at temperature 1
//   L <= t < L + C  byte i = t - L drawn from p (mode 0: expf(z) unshifted, as b1_output, or expf(z - max z) when STABLE;
//                   1: expf((z - max z) / tau);
//                   2: argmax z, lowest index on ties) by the sequential float CDF walk of R/lstm.cc:321-338 (index 0
//                   if u passes every edge); it goes to out[i * streams + s] and becomes the next input
//   t == L + C      the state is the stream's final one: copied to h_out / c_out (the stream idles afterwards, x = -1)
// Workgroup g owns streams g*SB .. g*SB+SB-1; thread m owns logit m of all of them, so each Why element read serves SB
// streams (h of the group in LDS, k-major).  Each logit is summed sequentially in k with separate multiply and add
// (contraction is off in this file), so a stream's bytes do not depend on SB, on its position or on the other streams.
// STABLE (LSTM_HIP_STABLE_SOFTMAX): scored prompt bytes and mode-0 draws shift by max z too, and a prompt byte scores
// lse_surprisal (the max and the target's logit are taken by the stream's max thread).
// FILTER (lstm_hip_generate_ex with a filter, a stop byte or `kept` wanted; DESIGN.md section 3.8): the instantiation with
// FILTER = false is the code above and nothing else.  With it,
//   a.filter    a tempered draw keeps the `keep` most likely bytes: thread m ranks its logit among the stream's 256 (z
//               descending, index ascending: 256 broadcast reads of the z still in ps), the normalised terms p are scattered
//               to sorted[rank], the stream's owner lane walks them in rank order until the float sum reaches a.top_p (at
//               most a.keep_k of them), every thread clears its term if its rank is not kept, and the owner lane sums the
//               kept terms in index order and walks the CDF of p / that sum; past every edge the byte is the largest kept
//               index.  A stream's bytes still depend on nothing but its own h.  Greedy draws and prompt bytes ignore it.
//   a.stop_byte a stream draws a.end[s] bytes, not a.count: the owner lane sets it to i + 1 when draw i is the stop byte, so
//               the next launch copies the state after that byte to h_out / c_out and the stream idles.
//   a.kept      keep per filtered draw, 256 per unfiltered one, 1 per greedy one.
// CONSTRAIN (lstm_hip_generate_constrained; DESIGN.md section 3.10; implies FILTER, and without it the instantiation is the
// code above and nothing else): stream s is in state q = a.cstate[s] of the byte automaton a.ctab.  For a drawn byte thread m
// loads a.ctab[q * 256 + m] and, where that is 0xFFFF (forbidden), sets its logit to -inf before the logit goes to ps: rank,
// max, expf and sum all see the masked value.  A tempered draw is then always a filtered one, keep capped by a.ccount[q] (the
// allowed bytes of q), so the kept bytes are allowed ones.  The owner lane replaces a byte that is forbidden all the same
// (non-finite logits only) by the lowest allowed byte of q and writes the next state to a.cstate[s].  Prompt bytes ignore it.
// DEADLINE (lstm_hip_generate_accepting; DESIGN.md section 3.16; implies CONSTRAIN, and without it the instantiation is the code
// above and nothing else): at draw i of a stream, R = a.count - i draws remain.  Byte m EXISTS iff nx = a.ctab[q * 256 + m] is
// allowed and a.accept[nx] (m the stop byte) or bit nx of row R - 1 of a.frows (any other byte): an accepted end can still be
// reached behind it.  A byte that does not exist is masked like a forbidden one; thread m tests its own byte (one more load,
// ahead of the product: the row differs per stream, as prompts differ in length) and the group counts the existing bytes E of
// every stream in LDS, which caps keep in place of a.ccount[q].  The owner lane replaces a byte that does not exist by the
// lowest existing one.  The host has checked F[count][q0], so E >= 1 at every draw and the stream ends in an accepting state.
// PROCESS (lstm_hip_generate_processed; DESIGN.md section 3.22; implies FILTER, goes with any of the three above, and without it
// the instantiation is the code above and nothing else): per drawn byte, in this order,
//   a.gsum      (guides; lstm_hip_generate_guided, DESIGN.md section 3.24) thread m's logit becomes a.wmain * z + a.gsum[s * 256 + m],
//               a multiply and an add rounded separately behind by; the sum is k_guide_logits' of this step (guide_logits.inc).
//               With a.gsum null nothing is read and the logit is z.
//   a.bias      thread m adds a.bias[m] to its logit (one float add behind by; greedy draws see it, prompt bytes do not).
//   a.no_repeat ahead of the product the group's 256 threads scan the stream's text T = a.ptext[a.ptoff[s] ..) ++ its column of
//               a.out (draws 0 .. i - 1, strided by streams) in strides of 256 positions: where T[p .. p + n - 1) equals T's
//               last n - 1 bytes (and p + n - 1 < |T|) byte T[p + n - 1] is banned, an atomicOr into the stream's 256-bit mask
//               s_ban (zeroed one barrier earlier; the barrier behind the hs fill publishes it).  Thread m counts itself into
//               s_surv[j] if its byte is valid (allowed / existing) and not banned; one more barrier behind the product, and
//               with s_surv[j] == 0 the ban is dropped for this draw (the table always wins).  Otherwise a banned logit is
//               -inf like a forbidden one and s_surv[j] caps keep.  The scan is linear in |T| at every draw.
//   a.min_p     a tempered draw is always a filtered one; behind the nucleus walk (bounded by keep_k and the survivors, as
//               before) the owner lane walks sorted[1 .. keep) and cuts at the first term below a.min_p * sorted[0].
//   the owner lane replaces a byte that is not a survivor (non-finite logits only) by the lowest surviving one.
// ------------------------------------------------------------------------------------------------
// what stream s does at step t: 0 idle, 1 prompt byte scored, 2 drawn byte, 3 prompt byte not scored; *len = its prompt length
// (*drawn: the bytes the stream draws -- the call's count, or with FILTER its own end index)
template <bool FILTER>
__device__ __forceinline__ int gen_phase(const GenHeadArgs &a, int s, long long t, long long *len, int *drawn = nullptr) {
    *len = a.off ? (long long)(a.off[s + 1] - a.off[s]) : 0;
    const int n = FILTER ? a.end[s] : a.count;
    if (drawn) *drawn = n;
    if (t < *len) return (t >= 1 && a.bits) ? 1 : 3;
    return t - *len < n ? 2 : 0;
}
// does byte x exist for a stream in the state whose table row is `row`, `left` draws before its last one?  (DEADLINE)
__device__ __forceinline__ bool gen_exists(const GenHeadArgs &a, const uint16_t *row, int x, long long left) {
    const uint16_t nx = row[x];
    if (nx == 0xFFFF) return false;
    if (x == a.stop_byte) return a.accept[nx] != 0;
    return (a.frows[(size_t)left * a.fwords + (nx >> 5)] >> (nx & 31)) & 1u;
}
template <int SB, bool STABLE, bool FILTER, bool CONSTRAIN = false, bool DEADLINE = false, bool PROCESS = false>
__global__ __launch_bounds__(256) void k_gen_head(GenHeadArgs a, long long t) {
    static_assert(FILTER || !CONSTRAIN, "CONSTRAIN implies FILTER");
    static_assert(FILTER || !PROCESS, "PROCESS implies FILTER");
    static_assert(CONSTRAIN || !DEADLINE, "DEADLINE implies CONSTRAIN");
    HEAD_DYNAMIC_LDS(float, hs); // [N][SB]
    __shared__ float ps[SB][256];
    __shared__ float s_zmax[SB], s_sum[SB], s_zt[STABLE ? SB : 1];
    __shared__ int s_arg[SB];
    __shared__ float sorted[FILTER ? SB : 1][FILTER ? 256 : 1]; // p in rank order
    __shared__ int s_keep[FILTER ? SB : 1], s_last[FILTER ? SB : 1]; // bytes kept; the largest kept index
    [[maybe_unused]] __shared__ int s_exist[DEADLINE ? SB : 1]; // E: the bytes that exist for each drawing stream
    [[maybe_unused]] __shared__ unsigned s_ban[PROCESS ? SB : 1][8]; // bit b: byte b is banned by the n-gram rule (PROCESS)
    [[maybe_unused]] __shared__ int s_surv[PROCESS ? SB : 1]; // S: the valid bytes the ban leaves each drawing stream
    const int m = threadIdx.x, N = a.N, s0 = blockIdx.x * SB;
    int phase[SB]; // (the same in every thread)
    [[maybe_unused]] int cq[CONSTRAIN ? SB : 1]; // the automaton state of each drawing stream (read before any barrier)
    [[maybe_unused]] long long left[DEADLINE ? SB : 1]; // draws each drawing stream has before its last one: R - 1
    [[maybe_unused]] long long drew[PROCESS ? SB : 1]; // bytes each drawing stream has drawn so far: i
    bool need = false;
#pragma unroll
    for (int j = 0; j < SB; j++) {
        const int s = s0 + j;
        phase[j] = 0;
        if (s >= a.streams) continue;
        long long len;
        int drawn;
        phase[j] = gen_phase<FILTER>(a, s, t, &len, &drawn);
        need |= phase[j] == 1 || phase[j] == 2;
        if constexpr (CONSTRAIN) cq[j] = phase[j] == 2 ? a.cstate[s] : 0;
        if constexpr (DEADLINE) left[j] = phase[j] == 2 ? a.count - 1 - (t - len) : 0;
        if constexpr (PROCESS) drew[j] = phase[j] == 2 ? t - len : 0;
        if (t == len + drawn) { // the state after the stream's last input
            if (a.h_out)
                for (int k = m; k < N; k += 256) a.h_out[(size_t)s * N + k] = a.H[(size_t)s * N + k];
            if (a.c_out)
                for (int k = m; k < N; k += 256) a.c_out[(size_t)s * N + k] = a.C[(size_t)s * N + k];
        }
    }
    if (need) { // (uniform)
        [[maybe_unused]] bool banned[CONSTRAIN ? SB : 1]; // is byte m forbidden where stream j stands?  (loaded ahead of the product)
        if constexpr (CONSTRAIN) {
#pragma unroll
            for (int j = 0; j < SB; j++) {
                if constexpr (DEADLINE) banned[j] = phase[j] == 2 && !gen_exists(a, a.ctab + (size_t)cq[j] * 256, m, left[j]);
                else banned[j] = phase[j] == 2 && a.ctab[(size_t)cq[j] * 256 + m] == 0xFFFF;
            }
        }
        if constexpr (DEADLINE)
            if (m < SB) s_exist[m] = 0; // (counted behind the barrier below)
        if constexpr (PROCESS) {
            if (m < SB * 8) (&s_ban[0][0])[m] = 0u;
            if (m < SB) s_surv[m] = 0; // (counted behind the barrier below)
            if (a.no_repeat > 0) { // (uniform) the n-gram scan: position p of the text to thread p % 256
                __syncthreads();
                const long long n1 = a.no_repeat - 1;
#pragma unroll
                for (int j = 0; j < SB; j++) {
                    if (phase[j] != 2) continue;
                    const int s = s0 + j;
                    const uint8_t *text = a.ptext + a.ptoff[s];
                    const long long tl = (long long)(a.ptoff[s + 1] - a.ptoff[s]), tlen = tl + drew[j];
                    auto at = [&](long long p) -> unsigned { return p < tl ? text[p] : a.out[(size_t)(p - tl) * a.streams + s]; };
                    for (long long p = m; p + n1 < tlen; p += 256) {
                        long long k = 0;
                        while (k < n1 && at(p + k) == at(tlen - n1 + k)) k++;
                        if (k == n1) {
                            const unsigned b = at(p + n1);
                            atomicOr(&s_ban[j][b >> 5], 1u << (b & 31));
                        }
                    }
                }
            }
        }
        for (int i = m; i < N * SB; i += 256) {
            const int k = i / SB, j = i - k * SB;
            hs[i] = s0 + j < a.streams ? a.H[(size_t)(s0 + j) * N + k] : 0.0f;
        }
        __syncthreads();
        [[maybe_unused]] bool cut[PROCESS ? SB : 1]; // is byte m banned by the n-gram rule for stream j?
        if constexpr (PROCESS) {
#pragma unroll
            for (int j = 0; j < SB; j++) {
                cut[j] = phase[j] == 2 && ((s_ban[j][m >> 5] >> (m & 31)) & 1u);
                bool valid = phase[j] == 2 && !cut[j];
                if constexpr (CONSTRAIN) valid = valid && !banned[j];
                if (valid) atomicAdd(&s_surv[j], 1); // (read behind the barrier that follows the product)
            }
        }
        float y[SB];
#pragma unroll
        for (int j = 0; j < SB; j++) y[j] = 0.0f;
        for (int k0 = 0; k0 < N; k0 += 16) { // 16 loads in flight; the additions stay in k order (as b1_output)
            float wv[16];
#pragma unroll
            for (int i = 0; i < 16; i++) wv[i] = a.Why[(size_t)(k0 + i) * 256 + m];
#pragma unroll
            for (int i = 0; i < 16; i++)
#pragma unroll
                for (int j = 0; j < SB; j++) y[j] += wv[i] * hs[(k0 + i) * SB + j];
        }
        if constexpr (DEADLINE) {
#pragma unroll
            for (int j = 0; j < SB; j++)
                if (phase[j] == 2 && !banned[j]) atomicAdd(&s_exist[j], 1); // (read behind the filter's barriers)
        }
        [[maybe_unused]] float bias_m = 0.0f;
        if constexpr (PROCESS) {
            if (a.bias) bias_m = a.bias[m];
            __syncthreads(); // s_surv (and s_exist) are complete
        }
        const float bym = a.by[m];
        bool any_max = false;
        [[maybe_unused]] bool any_filter = false;
#pragma unroll
        for (int j = 0; j < SB; j++) {
            y[j] = y[j] + bym; // the logit z
            if constexpr (PROCESS) {
                if (a.gsum && phase[j] == 2) y[j] = a.wmain * y[j] + a.gsum[(size_t)(s0 + j) * 256 + m]; // (uniform test; two roundings)
                if (a.bias && phase[j] == 2) y[j] = y[j] + bias_m;
            }
            if constexpr (CONSTRAIN)
                if (banned[j]) y[j] = -INFINITY;
            if constexpr (PROCESS)
                if (cut[j] && s_surv[j] > 0) y[j] = -INFINITY; // (no survivor: the ban is dropped for this draw)
            ps[j][m] = y[j];
            any_max |= phase[j] == 2 && a.mode != 0;
            if constexpr (STABLE) any_max |= phase[j] == 1 || phase[j] == 2;
            if constexpr (FILTER) any_filter |= phase[j] == 2 && a.mode != 2 && (CONSTRAIN || PROCESS || a.filter);
        }
        [[maybe_unused]] int rank[FILTER ? SB : 1]; // of this thread's logit: #{z_i > z_m} + #{i < m: z_i == z_m}, in 0..255
        if constexpr (FILTER)
            if (any_filter) { // (uniform)
                __syncthreads();
#pragma unroll
                for (int j = 0; j < SB; j++) {
                    rank[j] = 0;
                    if (phase[j] != 2) continue;
                    const float zm = y[j];
                    int r = 0;
#pragma unroll 8
                    for (int i = 0; i < 256; i++) {
                        const float zi = ps[j][i];
                        r += (zi > zm) | ((zi == zm) & (i < m));
                    }
                    rank[j] = r;
                }
                __syncthreads(); // (ps is overwritten below)
            }
        if (any_max) { // max z / argmax z of each tempered or greedy stream (every order gives the same max)
            __syncthreads();
            long long len;
            const int pm = m < SB && s0 + m < a.streams ? gen_phase<FILTER>(a, s0 + m, t, &len) : 0;
            if (pm == 2 || (STABLE && pm == 1)) {
                float best = ps[m][0];
                int arg = 0;
                for (int i = 1; i < 256; i++)
                    if (ps[m][i] > best) {
                        best = ps[m][i];
                        arg = i;
                    }
                s_zmax[m] = best;
                s_arg[m] = arg;
                if constexpr (STABLE)
                    if (pm == 1) s_zt[m] = ps[m][a.prompts[a.off[s0 + m] + t]];
            }
            __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < SB; j++) {
            if (phase[j] == 1 || (phase[j] == 2 && a.mode == 0)) ps[j][m] = STABLE ? expf(y[j] - s_zmax[j]) : expf(y[j]);
            else if (phase[j] == 2 && a.mode == 1) ps[j][m] = expf((y[j] - s_zmax[j]) / a.tau);
        }
        __syncthreads();
        long long len;
        const int pm = m < SB && s0 + m < a.streams ? gen_phase<FILTER>(a, s0 + m, t, &len) : 0;
        if (pm == 1 || (pm == 2 && a.mode != 2)) {
            float s = 0.0f;
            for (int i = 0; i < 256; i++) s += ps[m][i];
            s_sum[m] = s;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < SB; j++)
            if (phase[j] == 1 || (phase[j] == 2 && a.mode != 2)) ps[j][m] = ps[j][m] / s_sum[j]; // p, the CDF's terms
        __syncthreads();
        if constexpr (FILTER)
            if (any_filter) { // (uniform)
#pragma unroll
                for (int j = 0; j < SB; j++)
                    if (phase[j] == 2) sorted[j][rank[j]] = ps[j][m];
                if (m < SB) s_last[m] = 0;
                __syncthreads();
                // the stream's owner lane (as below) walks the nucleus prefix: most likely first, one float sum
                const int jo = (m & 63) * 4 + (m >> 6);
                if (jo < SB && s0 + jo < a.streams) {
                    long long lo;
                    if (gen_phase<FILTER>(a, s0 + jo, t, &lo) == 2) {
                        int keep = a.keep_k;
                        if constexpr (DEADLINE) {
                            if (s_exist[jo] < keep) keep = s_exist[jo];
                        } else if constexpr (CONSTRAIN) {
                            const int allowed = a.ccount[a.cstate[s0 + jo]];
                            if (allowed < keep) keep = allowed;
                        }
                        if constexpr (PROCESS)
                            if (s_surv[jo] > 0 && s_surv[jo] < keep) keep = s_surv[jo]; // (S <= the valid bytes)
                        if (a.nucleus) {
                            float sum = 0.0f;
                            for (int r = 0; r < keep; r++) { // (past keep_k the nucleus no longer matters)
                                sum += sorted[jo][r];
                                if (sum >= a.top_p) {
                                    keep = r + 1;
                                    break;
                                }
                            }
                        }
                        if constexpr (PROCESS)
                            if (a.min_p > 0.0f) { // behind the nucleus walk: the first term below min_p * the largest
                                const float thr = a.min_p * sorted[jo][0];
                                for (int r = 1; r < keep; r++)
                                    if (sorted[jo][r] < thr) {
                                        keep = r;
                                        break;
                                    }
                            }
                        s_keep[jo] = keep;
                    }
                }
                __syncthreads();
#pragma unroll
                for (int j = 0; j < SB; j++) {
                    if (phase[j] != 2) continue;
                    if (rank[j] < s_keep[j]) atomicMax(&s_last[j], m);
                    else ps[j][m] = 0.0f;
                }
                __syncthreads();
            }
    }
    // one owner thread per stream, spread over the four waves
    const int j = (m & 63) * 4 + (m >> 6);
    if (j >= SB || s0 + j >= a.streams) return;
    const int s = s0 + j;
    long long len;
    const int ph = gen_phase<FILTER>(a, s, t, &len);
    int x = -1;
    if (ph == 1 || ph == 3) {
        x = a.prompts[a.off[s] + t];
        if (ph == 1) {
            if constexpr (STABLE) a.bits[s] += (double)lse_surprisal(s_sum[j], s_zmax[j], s_zt[j]);
            else a.bits[s] += -(double)log2f(ps[j][x]);
        }
    } else if (ph == 2) {
        const size_t i = (size_t)(t - len);
        [[maybe_unused]] int kept = 256;
        if (a.mode == 2) {
            x = s_arg[j];
            kept = 1;
        } else if (FILTER && (CONSTRAIN || PROCESS || a.filter)) {
            kept = s_keep[j];
            const float r = (float)a.u[i * a.streams + s];
            float sum = 0.0f; // of the kept terms, in index order
            for (int k = 0; k < 256; k++) sum += ps[j][k];
            float cdf = 0.0f;
            x = s_last[j];
            for (int k = 0; k < 256; k++) {
                cdf += ps[j][k] / sum;
                if (r < cdf) {
                    x = k;
                    break;
                }
            }
        } else {
            const float r = (float)a.u[i * a.streams + s];
            float cdf = 0.0f;
            x = 0;
            for (int k = 0; k < 256; k++) {
                cdf += ps[j][k];
                if (r < cdf) {
                    x = k;
                    break;
                }
            }
        }
        if constexpr (PROCESS) { // a byte that is no survivor gives way to the lowest surviving one; the automaton advances
            const bool drop = s_surv[j] == 0;
            [[maybe_unused]] const uint16_t *row = nullptr;
            if constexpr (CONSTRAIN) row = a.ctab + (size_t)a.cstate[s] * 256;
            auto survives = [&](int b) {
                if (!drop && ((s_ban[j][b >> 5] >> (b & 31)) & 1u)) return false;
                if constexpr (DEADLINE) return gen_exists(a, row, b, a.count - 1 - (long long)i);
                else if constexpr (CONSTRAIN) return row[b] != 0xFFFF;
                else return true;
            };
            if (!survives(x))
                for (x = 0; x < 255 && !survives(x); x++) {}
            if constexpr (CONSTRAIN)
                if (row[x] != 0xFFFF) a.cstate[s] = row[x];
        } else if constexpr (CONSTRAIN) { // advance the automaton; a forbidden byte gives way to the state's lowest allowed one
            const uint16_t *row = a.ctab + (size_t)a.cstate[s] * 256;
            if constexpr (DEADLINE) { // a byte that does not exist gives way to the lowest existing one
                const long long lf = a.count - 1 - (long long)i;
                if (!gen_exists(a, row, x, lf))
                    for (x = 0; x < 255 && !gen_exists(a, row, x, lf); x++) {}
            } else if (row[x] == 0xFFFF)
                for (x = 0; x < 255 && row[x] == 0xFFFF; x++) {}
            if (row[x] != 0xFFFF) a.cstate[s] = row[x]; // (an empty row cannot be reached: the state never leaves the table)
        }
        a.out[i * a.streams + s] = (uint8_t)x;
        if constexpr (FILTER) {
            if (a.kept) a.kept[i * a.streams + s] = (uint16_t)kept;
            if (x == a.stop_byte) a.end[s] = (int32_t)i + 1; // (read again by the next launch only)
        }
    }
    a.x_next[s] = x;
}
