// Host emulation of k_gen_head<SB, false, true> (eigen-lstm_amd/csrc/kernels.hip) for tests/test_sampling_head_emulation_cpu.py:
// the kernel's own text (csrc/heads/gen_head.inc, the file kernels.hip includes, with heads/head_args.h and the real
// heads/lse_surprisal.h) compiled for the host over tests/device_shim.h: one std::thread per work-item, a std::barrier for
// __syncthreads, function-static arrays for LDS.  It checks the head's logic -- ranks, nucleus walk, masked
// renormalisation, CDF walk, stop index, final-state copy -- without a device; it says nothing about the GPU build.
//   gen_head_emulation DIR N streams count steps SB mode tau keep_k nucleus top_p filter stop_byte
// reads why, by, hs ([steps+1][streams][N], the state before each step), u, off, prompts (.bin) from DIR and writes out,
// kept, end, ho, xlog (x_next after every step), bits.
#include "device_shim.h"
#include "heads/head_args.h"
using namespace lstmk;
#include "heads/lse_surprisal.h"
#include "heads/gen_head.inc"

template <int SB> void launch(const GenHeadArgs &a, long long t) {
    run_blocks((a.streams + SB - 1) / SB, [&] { k_gen_head<SB, false, true>(a, t); });
}
// argv: dir N streams count steps sb mode tau keep_k nucleus top_p filter stop_byte
int main(int argc, char **argv) {
    std::string d = argv[1];
    GenHeadArgs a{};
    a.N = atoi(argv[2]); a.streams = atoi(argv[3]); a.count = atoi(argv[4]);
    const int steps = atoi(argv[5]), sb = atoi(argv[6]);
    a.mode = atoi(argv[7]); a.tau = (float)atof(argv[8]); a.keep_k = atoi(argv[9]); a.nucleus = atoi(argv[10]);
    a.top_p = (float)atof(argv[11]); a.filter = atoi(argv[12]); a.stop_byte = atoi(argv[13]);
    auto Why = load<float>((d + "/why.bin").c_str()), by = load<float>((d + "/by.bin").c_str());
    auto Hs = load<float>((d + "/hs.bin").c_str());   // [steps+1][streams][N]
    auto u = load<double>((d + "/u.bin").c_str());
    auto off = load<uint64_t>((d + "/off.bin").c_str());
    auto prompts = load<uint8_t>((d + "/prompts.bin").c_str());
    const size_t n = (size_t)a.N * a.streams, nd = (size_t)a.count * a.streams;
    std::vector<uint8_t> out(nd, 0); std::vector<uint16_t> kept(nd, 0); std::vector<int32_t> end(a.streams, a.count), xn(a.streams);
    std::vector<float> ho(n, -7.f), co(n, -7.f); std::vector<double> bits(a.streams, 0.0);
    std::vector<int32_t> xlog;
    a.Why = Why.data(); a.by = by.data(); a.prompts = prompts.data(); a.off = off.data(); a.u = u.data(); a.out = out.data();
    a.bits = bits.data(); a.x_next = xn.data(); a.h_out = ho.data(); a.c_out = co.data(); a.end = end.data(); a.kept = kept.data();
    for (long long t = 0; t <= steps; t++) {
        a.H = Hs.data() + t * n; a.C = a.H;
        if (sb == 1) launch<1>(a, t); else if (sb == 4) launch<4>(a, t); else launch<16>(a, t);
        xlog.insert(xlog.end(), xn.begin(), xn.end());
    }
    save((d + "/out.bin").c_str(), out); save((d + "/kept.bin").c_str(), kept); save((d + "/end.bin").c_str(), end);
    save((d + "/ho.bin").c_str(), ho); save((d + "/xlog.bin").c_str(), xlog); save((d + "/bits.bin").c_str(), bits);
    return 0;
}
