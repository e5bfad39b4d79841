// Host emulation of the mixed coder's two launches per step for
// tests/test_mix_code_head_emulation_cpu.py: k_guide_logits<SB> in coder mode, then k_code_head<SB, true>, the kernels' own
// text (csrc/heads/guide_logits.inc and code_head.inc with heads/head_args.h) compiled for the host over tests/device_shim.h
// as tests/code_head_emulation.cc compiles the unmixed head.  With mix = 0 it runs k_code_head<SB, false> alone on the same
// inputs: the instantiation the unmixed calls launch.  It checks the heads' logic without a device; it says nothing about
// the GPU build.
//   mix_code_head_emulation DIR N streams steps SB decode mix nguides rate
// reads why ([N][256]), by, hs ([steps+1][streams][N], the state before each step), text_off, text, code, code_base, and per
// guide k g<k>_why, g<k>_by, g<k>_hs, with gn (the guides' widths) and v0 ([streams][1 + nguides], the call's weights), from
// DIR.  Runs steps t = 0 .. steps with the CoderState array and the weights carried between them as the API carries them,
// and writes code_out, text_out, trace ([total][3]), w_trace ([total][1 + nguides]), w_out, bits, code_len, xlog (x_next after
// every step), zklog (zk after every step's guide launch, set to -7 ahead of it) and err.
#include "device_shim.h"
#include "heads/head_args.h"
using namespace lstmk;
#include "heads/lse_surprisal.h"
#include "heads/gen_head.inc"
#include "heads/guide_logits.inc"
#include "heads/code_head.inc"

template <int SB> void launch(const GuideLogitsArgs &ga, const CodeHeadArgs &a, long long t, bool mix) {
    const int grid = (a.streams + SB - 1) / SB;
    if (mix) {
        run_blocks(grid, [&] { k_guide_logits<SB>(ga, t); });
        run_blocks(grid, [&] { k_code_head<SB, true>(a, t); });
    } else
        run_blocks(grid, [&] { k_code_head<SB, false>(a, t); });
}
int main(int argc, char **argv) {
    if (argc != 10) return 2;
    std::string d = argv[1];
    CodeHeadArgs a{};
    a.N = atoi(argv[2]); a.streams = atoi(argv[3]);
    const int steps = atoi(argv[4]), sb = atoi(argv[5]);
    a.decode = atoi(argv[6]);
    const bool mix = atoi(argv[7]) != 0;
    const int G = atoi(argv[8]);
    const float rate = (float)atof(argv[9]);
    if (G < 1 || G > MAX_GUIDES) return 2;
    auto Why = load<float>((d + "/why.bin").c_str()), by = load<float>((d + "/by.bin").c_str());
    auto Hs = load<float>((d + "/hs.bin").c_str());   // [steps+1][streams][N]
    auto text_off = load<uint64_t>((d + "/text_off.bin").c_str()), code_base = load<uint64_t>((d + "/code_base.bin").c_str());
    auto text = load<uint8_t>((d + "/text.bin").c_str()), code = load<uint8_t>((d + "/code.bin").c_str());
    auto gn = load<int32_t>((d + "/gn.bin").c_str());
    auto v = load<float>((d + "/v0.bin").c_str());
    const size_t n = (size_t)a.N * a.streams, total = text_off[a.streams];
    if (Hs.size() != n * (steps + 1) || text.size() < total + 1 || (int)gn.size() != G || v.size() != (size_t)a.streams * (1 + G)) return 3;
    std::vector<float> gWhy[MAX_GUIDES], gby[MAX_GUIDES], gHs[MAX_GUIDES];
    GuideLogitsArgs ga{};
    for (int k = 0; k < G; k++) {
        const std::string p = d + "/g" + std::to_string(k);
        gWhy[k] = load<float>((p + "_why.bin").c_str()); gby[k] = load<float>((p + "_by.bin").c_str());
        gHs[k] = load<float>((p + "_hs.bin").c_str());
        if (gHs[k].size() != (size_t)gn[k] * a.streams * (steps + 1)) return 3;
        ga.Why[k] = gWhy[k].data(); ga.by[k] = gby[k].data(); ga.N[k] = gn[k];
        ga.w[k] = -3.0f; // (coder mode: the call's weights are not the kernel's business)
    }
    std::vector<float> zk((size_t)a.streams * G * 256), zklog, w_trace((total + 1) * (1 + G), 0.0f);
    std::vector<uint32_t> trace(3 * total + 3, 0u), err(1, 0u);
    std::vector<double> bits(a.streams, 0.0);
    std::vector<uint64_t> code_len(a.streams, 0);
    std::vector<CoderState> state(a.streams);
    memset(state.data(), 0xEE, state.size() * sizeof(CoderState)); // (a step that read a state before writing it would show)
    std::vector<int32_t> xn(a.streams, -7), xlog;
    a.Why = Why.data(); a.by = by.data(); a.text_off = text_off.data(); a.text = text.data(); a.code = code.data();
    a.code_base = code_base.data(); a.code_len = code_len.data(); a.state = state.data(); a.x_next = xn.data(); a.err = err.data();
    if (!a.decode) { a.bits = bits.data(); a.trace = trace.data(); }
    if (mix) {
        a.zk = zk.data(); a.v = v.data(); a.nguides = G; a.rate = rate;
        if (!a.decode) a.w_trace = w_trace.data();
    }
    ga.nguides = G; ga.streams = a.streams; ga.off = text_off.data(); ga.coder = 1; ga.zk = zk.data();
    for (long long t = 0; t <= steps; t++) {
        a.H = Hs.data() + t * n;
        for (int k = 0; k < G; k++) ga.H[k] = gHs[k].data() + t * (size_t)gn[k] * a.streams;
        std::fill(zk.begin(), zk.end(), -7.0f);
        switch (sb) {
        case 1: launch<1>(ga, a, t, mix); break;
        case 2: launch<2>(ga, a, t, mix); break;
        default: return 2;
        }
        xlog.insert(xlog.end(), xn.begin(), xn.end());
        zklog.insert(zklog.end(), zk.begin(), zk.end());
    }
    save((d + "/code_out.bin").c_str(), code); save((d + "/text_out.bin").c_str(), text); save((d + "/trace.bin").c_str(), trace);
    save((d + "/bits.bin").c_str(), bits); save((d + "/code_len.bin").c_str(), code_len); save((d + "/xlog.bin").c_str(), xlog);
    save((d + "/err.bin").c_str(), err); save((d + "/w_trace.bin").c_str(), w_trace); save((d + "/w_out.bin").c_str(), v);
    save((d + "/zklog.bin").c_str(), zklog);
    return 0;
}
