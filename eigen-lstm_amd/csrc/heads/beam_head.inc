// beam_head.inc -- beam_before and k_beam_head, the per-step kernel of lstm_hip_beam_search.
// Included by kernels.hip inside namespace lstmk, at the place this text stood, and by the host emulations under tests/
// (tests/device_shim.h supplies the device words there).  Not a translation unit of its own.
// ------------------------------------------------------------------------------------------------
// beam_head: one step of beam search (lstm_hip_beam_search; DESIGN.md section 3.9).  One workgroup per stream s, whose W
// slots are columns s*W .. s*W+W-1; with L = the stream's prompt length:
//   t <  L          every slot gets input prompt[t]; the state is copied to Hr / Cr as it is
//   L <= t < L + C  selection i = t - L (below), the state gathered to Hr / Cr by parent
//   otherwise       the stream idles (x = -1)
// Selection: as k_gen_head with SB = W, thread m owns logit m of all W slots (h of the slots in LDS, k-major; the same k
// order and 16-deep load batching, so a logit has the bits of the generator's).  Per live slot j an owner lane takes
// zmax = max z and s = the sequential float sum of expf(z - zmax); thread m's candidate (j, m) costs
// cost_j + (double)lse_surprisal(s, zmax, z_m), NaN taken as +inf.  A finished slot offers one candidate, held by thread 0:
// itself, cost unchanged, byte 0.  Then W rounds of a block-wide arg-min under (cost ascending, parent ascending, z
// descending, byte ascending): the thread's best of its register-held candidates (all of one byte, so: lowest cost, then
// lowest parent; rescanned only after one of them was retired), 6 shuffle steps inside the wave, the four waves through
// LDS; the winner's thread retires it.  There are always at least W candidates, so every round finds one.  New slot r
// is round r's winner: tables, cost, length, finished flag and next input are written by thread r.
// WP: W rounded up to a power of two (register arrays); EXACT: W == WP, so that the LDS stride is a constant.
// CONSTRAIN (lstm_hip_beam_search_constrained; DESIGN.md section 3.12): the instantiation with CONSTRAIN = false is the code
// above and nothing else.  With it every slot carries a state q of the byte automaton a.ctab (s_q, read into LDS with the
// costs).  Thread m reads next[q_j][m] of every live slot j (one table row per slot, 2-byte coalesced loads) and keeps two
// masks, a bit per slot: `allowed` (the entry is not 0xFFFF) and `exists` (allowed, and with a.accept the deadline: at
// selection i the byte must lead to a state from which an accepted end is count - i - 1 bytes away -- bit next of row
// count - i - 1 of a.frows --, the stop byte into an accepting state).  z is set to -inf where the byte is not allowed, before
// the max and before expf, so a forbidden term adds 0.0f to the sum: cost, zmax and sum are the scorer's under the same
// table.  Only candidates that exist are offered.  Thread r writes the new slot's state: its parent's if that was finished,
// else next[q_p][b].
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool beam_before(double c1, int i1, float z1, double c2, int i2, float z2) { // idx = parent * 256 + byte
    if (c1 != c2) return c1 < c2;
    if ((i1 >> 8) != (i2 >> 8)) return (i1 >> 8) < (i2 >> 8);
    if (z1 != z2) return z1 > z2;
    return (i1 & 255) < (i2 & 255);
}
template <int WP, bool EXACT, bool CONSTRAIN = false>
__global__ __launch_bounds__(256) void k_beam_head(BeamHeadArgs a, long long t) {
    HEAD_DYNAMIC_LDS(float, hs); // [N][W]
    __shared__ float ps[WP][256];
    __shared__ double s_cost[WP], sel_cost[WP], w_cost[4];
    __shared__ float s_zmax[WP], s_sum[WP], w_z[4];
    __shared__ int s_len[WP], s_fin[WP], sel_idx[WP], w_idx[4];
    __shared__ int s_q[CONSTRAIN ? WP : 1];
    const int m = threadIdx.x, N = a.N, s = blockIdx.x, W = EXACT ? WP : a.W;
    const size_t c0 = (size_t)s * W, SW = (size_t)a.streams * W;
    const long long len = a.off ? (long long)(a.off[s + 1] - a.off[s]) : 0;
    const bool select = t >= len && t - len < a.count; // (uniform)
    constexpr int NONE = WP << 8;                      // no candidate: behind every real one (parent WP)
    if (m < W) sel_idx[m] = m << 8;                    // the gather of a step without a selection: every slot stays
    if (!select) {
        if (m < W) a.x_next[c0 + m] = t < len ? (int32_t)a.prompts[a.off[s] + t] : -1;
    } else {
        if (m < W) {
            s_cost[m] = a.cost[c0 + m];
            s_len[m] = a.len[c0 + m];
            s_fin[m] = a.fin[c0 + m];
            if constexpr (CONSTRAIN) s_q[m] = a.cstate[c0 + m];
        }
        for (int i = m; i < N * W; i += 256) {
            const int k = i / W, j = i - k * W;
            hs[i] = a.H[(c0 + j) * N + k];
        }
        __syncthreads();
        [[maybe_unused]] unsigned allowed = 0, exists = 0; // a bit per slot: byte m may follow it / is offered as a candidate
        if constexpr (CONSTRAIN) {
            const uint32_t *frow = a.frows ? a.frows + (size_t)(a.count - 1 - (t - len)) * a.fwords : nullptr;
#pragma unroll
            for (int j = 0; j < WP; j++) {
                if (j >= W || s_fin[j]) continue;
                const unsigned nx = a.ctab[(size_t)s_q[j] * 256 + m];
                if (nx == 0xFFFFu) continue;
                allowed |= 1u << j;
                bool ok = true;
                if (a.accept) ok = m == a.stop_byte ? a.accept[nx] != 0 : ((frow[nx >> 5] >> (nx & 31)) & 1u) != 0;
                if (ok) exists |= 1u << j;
            }
        }
        float y[WP];
        int jo[WP]; // slot whose h register j reads (registers W..WP-1 repeat the last slot and are never candidates)
#pragma unroll
        for (int j = 0; j < WP; j++) {
            y[j] = 0.0f;
            jo[j] = EXACT || j < W ? j : W - 1;
        }
        for (int k0 = 0; k0 < N; k0 += 16) { // as k_gen_head: 16 loads in flight, the additions in k order
            float wv[16];
#pragma unroll
            for (int i = 0; i < 16; i++) wv[i] = a.Why[(size_t)(k0 + i) * 256 + m];
#pragma unroll
            for (int i = 0; i < 16; i++)
#pragma unroll
                for (int j = 0; j < WP; j++) y[j] += wv[i] * hs[(k0 + i) * W + jo[j]];
        }
        const float bym = a.by[m];
#pragma unroll
        for (int j = 0; j < WP; j++) {
            y[j] = y[j] + bym; // the logit z
            if constexpr (CONSTRAIN)
                if (!((allowed >> j) & 1u)) y[j] = -INFINITY; // (finished slots too: their z is not read)
            if (j < W) ps[j][m] = y[j];
        }
        __syncthreads();
        const int own = (m & 63) * 4 + (m >> 6); // one owner thread per slot, spread over the four waves
        const bool owner = own < W && !s_fin[own];
        if (owner) { // (every order gives the same max)
            float best = ps[own][0];
            for (int i = 1; i < 256; i++) best = ps[own][i] > best ? ps[own][i] : best;
            s_zmax[own] = best;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < WP; j++)
            if (j < W && !s_fin[j]) ps[j][m] = expf(y[j] - s_zmax[j]);
        __syncthreads();
        if (owner) {
            float sum = 0.0f;
            for (int i = 0; i < 256; i++) sum += ps[own][i];
            s_sum[own] = sum;
        }
        __syncthreads();
        double ck[WP];        // this thread's candidates: slot j extended by byte m
        unsigned live = 0;    // ... those that exist and are not yet selected
#pragma unroll
        for (int j = 0; j < WP; j++) {
            ck[j] = (double)INFINITY;
            if (j >= W) continue;
            if (s_fin[j]) {
                if (m == 0) {
                    ck[j] = s_cost[j];
                    live |= 1u << j;
                }
                y[j] = 0.0f;
            } else {
                const double v = s_cost[j] + (double)lse_surprisal(s_sum[j], s_zmax[j], y[j]);
                ck[j] = v != v ? (double)INFINITY : v;
                if (!CONSTRAIN || ((exists >> j) & 1u)) live |= 1u << j;
            }
        }
        double lc = (double)INFINITY; // the thread's best live candidate
        float lz = 0.0f;
        int li = NONE;
        bool rescan = true;
        for (int r = 0; r < W; r++) {
            if (rescan) {
                lc = (double)INFINITY;
                lz = 0.0f;
                li = NONE;
#pragma unroll
                for (int j = 0; j < WP; j++)
                    if (((live >> j) & 1u) && (li == NONE || ck[j] < lc)) {
                        lc = ck[j];
                        lz = y[j];
                        li = (j << 8) | m;
                    }
                rescan = false;
            }
            double bc = lc;
            float bz = lz;
            int bi = li;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double oc = __shfl_xor(bc, o, 64);
                const float oz = __shfl_xor(bz, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (beam_before(oc, oi, oz, bc, bi, bz)) {
                    bc = oc;
                    bz = oz;
                    bi = oi;
                }
            }
            if ((m & 63) == 0) {
                w_cost[m >> 6] = bc;
                w_z[m >> 6] = bz;
                w_idx[m >> 6] = bi;
            }
            __syncthreads();
            bc = w_cost[0];
            bz = w_z[0];
            bi = w_idx[0];
#pragma unroll
            for (int w = 1; w < 4; w++)
                if (beam_before(w_cost[w], w_idx[w], w_z[w], bc, bi, bz)) {
                    bc = w_cost[w];
                    bz = w_z[w];
                    bi = w_idx[w];
                }
            if (bi < NONE && (bi & 255) == m) { // mine: retired
                live &= ~(1u << (bi >> 8));
                rescan = true;
            }
            if (m == 0) {
                sel_idx[r] = bi < NONE ? bi : (W - 1) << 8; // (a round always finds a candidate; the table stays in bounds regardless)
                sel_cost[r] = bc;
            }
            __syncthreads();
        }
        if (m < W) {
            const int p = sel_idx[m] >> 8, b = sel_idx[m] & 255, pf = s_fin[p];
            const size_t i = (size_t)(t - len);
            a.trace_parent[i * SW + c0 + m] = (uint8_t)p;
            a.trace_byte[i * SW + c0 + m] = (uint8_t)b;
            a.cost[c0 + m] = sel_cost[m];
            a.len[c0 + m] = s_len[p] + (pf ? 0 : 1);
            a.fin[c0 + m] = pf || b == a.stop_byte ? 1 : 0;
            a.x_next[c0 + m] = pf ? -1 : b;
            if constexpr (CONSTRAIN) {
                // every read of the old states comes from s_q, filled before the first barrier: writing the array in place
                // races with nothing (the workgroup owns its slots)
                const unsigned nx = pf ? 0xFFFFu : a.ctab[(size_t)s_q[p] * 256 + b];
                a.cstate[c0 + m] = nx == 0xFFFFu ? s_q[p] : (int)nx; // (a selected byte is allowed; the state stays in the table regardless)
            }
        }
    }
    __syncthreads();
    // states follow their parents (the workgroup owns every column it reads and writes; Hr / Cr are other buffers)
    for (int i = m; i < N * W; i += 256) {
        const int r = i / N, k = i - r * N, p = sel_idx[r] >> 8;
        a.Hr[(c0 + r) * N + k] = a.H[(c0 + p) * N + k];
        a.Cr[(c0 + r) * N + k] = a.C[(c0 + p) * N + k];
    }
}
