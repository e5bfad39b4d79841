// guide_logits.inc -- k_guide_logits, the per-step kernel of the guides of lstm_hip_generate_guided / lstm_hip_score_guided.
// Included by kernels.hip inside namespace lstmk, behind gen_head.inc (it calls gen_phase), and by the host emulations under
// tests/ (tests/device_shim.h supplies the device words there).  Not a translation unit of its own.
// ------------------------------------------------------------------------------------------------
// guide_logits: one launch per step, ahead of the head, for ALL guides of the call (DESIGN.md section 3.24).  Guide k carries its
// own state H[k] / C[k] ([streams][N[k]]), advanced beside the main model's by one k_fwd_step per guide on the head's x_next.
// On the state after t inputs, for every stream whose head needs logits at this step --
//   generator   the stream draws a byte: gen_phase<true> == 2 (a guided draw is a processed one, so a.end is always set)
//   scorer      the stream has a byte t and it is scored (t >= 1 or first)
// -- the kernel writes the weighted sum the head mixes in:
//   z^k_m = Why_k * h_k + by_k   k_gen_head's sum: sequential in the hidden index, separate multiply and add, by added last, so
//                                z^k is, bit for bit, what guide k's own call computes from that state
//   g_m = w[0] * z^0_m, then g_m = g_m + w[k] * z^k_m for k = 1 .. nguides - 1 in index order (one multiply, one add, each rounded)
//   a.gsum[s * 256 + m] = g_m
// Workgroup g owns streams g*SB .. g*SB+SB-1 and thread m owns logit m of all of them, as in k_gen_head; the loop over the guides
// is inside the kernel, which gives the index-order sum and costs one launch whatever nguides is.  Per guide, h_k of the group's
// streams is staged k-major in dynamic LDS ([widest N][SB] floats, reused from guide to guide between two barriers).  A stream's
// sum depends on nothing but its own states: not on SB, on its position or on the other streams.
// At the step where the head copies the main model's state to h_out / c_out -- the state after the stream's last input:
// t == prompt length + the bytes it draws (the stop byte included), or t == the text's length -- every guide's state of that
// stream goes to its h_out / c_out.  Streams that need nothing at this step are not computed and their rows of gsum not written.
// Coder mode (a.coder; lstm_hip_encode_mixed / lstm_hip_decode_mixed, DESIGN.md section 3.25): a stream is active iff t < its
// length, no state is copied out, and instead of the weighted sum each guide's own logits go to a.zk[(s * nguides + k) * 256 + m]
// (the coder's weights are per stream, and its update needs the members); rows of streams that have ended are not written.
// ------------------------------------------------------------------------------------------------
template <int SB>
__global__ __launch_bounds__(256) void k_guide_logits(GuideLogitsArgs a, long long t) {
    HEAD_DYNAMIC_LDS(float, hs); // [widest N][SB]
    const int m = threadIdx.x, s0 = blockIdx.x * SB;
    bool act[SB], fin[SB]; // stream j needs logits at this step / stands behind its last input (the same in every thread)
    bool need = false, last = false;
    GenHeadArgs ga{}; // what gen_phase reads of the generator's block
    ga.off = a.off;
    ga.end = a.end;
    ga.count = a.count;
#pragma unroll
    for (int j = 0; j < SB; j++) {
        const int s = s0 + j;
        act[j] = fin[j] = false;
        if (s >= a.streams) continue;
        if (a.coder) act[j] = (unsigned long long)t < a.off[s + 1] - a.off[s]; // (no end-state copy: fin stays false)
        else if (a.scorer) {
            const unsigned long long len = a.off[s + 1] - a.off[s];
            act[j] = (unsigned long long)t < len && (t >= 1 || a.first);
            fin[j] = (unsigned long long)t == len;
        } else {
            long long len;
            int drawn;
            act[j] = gen_phase<true>(ga, s, t, &len, &drawn) == 2;
            fin[j] = t == len + drawn;
        }
        need |= act[j];
        last |= fin[j];
    }
    if (last) { // (uniform)
#pragma unroll
        for (int g = 0; g < MAX_GUIDES; g++) {
            if (g >= a.nguides) break;
            const int N = a.N[g];
#pragma unroll
            for (int j = 0; j < SB; j++) {
                if (!fin[j]) continue;
                const size_t at = (size_t)(s0 + j) * N;
                if (a.h_out[g])
                    for (int k = m; k < N; k += 256) a.h_out[g][at + k] = a.H[g][at + k];
                if (a.c_out[g])
                    for (int k = m; k < N; k += 256) a.c_out[g][at + k] = a.C[g][at + k];
            }
        }
    }
    if (!need) return; // (uniform)
    float gs[SB];
#pragma unroll
    for (int j = 0; j < SB; j++) gs[j] = 0.0f;
#pragma unroll
    for (int g = 0; g < MAX_GUIDES; g++) {
        if (g >= a.nguides) break; // (uniform)
        const int N = a.N[g];
        const float *H = a.H[g], *Why = a.Why[g];
        if (g > 0) __syncthreads(); // (every thread is done with the guide before: hs is overwritten)
        for (int i = m; i < N * SB; i += 256) {
            const int k = i / SB, j = i - k * SB;
            hs[i] = s0 + j < a.streams ? H[(size_t)(s0 + j) * N + k] : 0.0f;
        }
        __syncthreads();
        float y[SB];
#pragma unroll
        for (int j = 0; j < SB; j++) y[j] = 0.0f;
        for (int k0 = 0; k0 < N; k0 += 16) { // as k_gen_head: 16 loads in flight, the additions in k order
            float wv[16];
#pragma unroll
            for (int i = 0; i < 16; i++) wv[i] = Why[(size_t)(k0 + i) * 256 + m];
#pragma unroll
            for (int i = 0; i < 16; i++)
#pragma unroll
                for (int j = 0; j < SB; j++) y[j] += wv[i] * hs[(k0 + i) * SB + j];
        }
        const float bym = a.by[g][m], w = a.w[g];
#pragma unroll
        for (int j = 0; j < SB; j++) {
            y[j] = y[j] + bym; // the guide's logit z^k
            if (g == 0) gs[j] = w * y[j];
            else gs[j] = gs[j] + w * y[j];
        }
        if (a.coder) // (uniform) the members themselves: the coder's weights are per stream, and its update needs them
#pragma unroll
            for (int j = 0; j < SB; j++)
                if (act[j]) a.zk[((size_t)(s0 + j) * a.nguides + g) * 256 + m] = y[j];
    }
    if (a.coder) return; // (uniform)
#pragma unroll
    for (int j = 0; j < SB; j++)
        if (act[j]) a.gsum[(size_t)(s0 + j) * 256 + m] = gs[j];
}
