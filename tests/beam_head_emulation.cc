// Host emulation of k_beam_head (eigen-lstm_amd/csrc/kernels.hip) for tests/test_beam_head_emulation_cpu.py: the kernel's own
// text (csrc/heads/beam_head.inc, the file kernels.hip includes, with heads/head_args.h and heads/lse_surprisal.h) compiled
// for the host over tests/device_shim.h, one std::thread per work-item, a std::barrier for __syncthreads, function-static arrays for LDS,
// cross-lane shuffles through a table.  It checks the head's logic -- per-slot max and sum, the W selection rounds, tables,
// costs, lengths, flags, next inputs, the gather -- without a device; it says nothing about the GPU build.
//   beam_head_emulation DIR N streams W count steps stop_byte
// reads why, by, hs and cs ([steps][streams*W][N], the state before each step), off, prompts (.bin) from DIR and writes the
// tables tp / tb, and per step xlog, costlog, lenlog, finlog, hr, cr.
#include "device_shim.h"
#include "heads/head_args.h"
using namespace lstmk;
#include "heads/lse_surprisal.h"
#include "heads/beam_head.inc"

template <int WP, bool EXACT> void launch(const BeamHeadArgs &a, long long t) {
    run_blocks(a.streams, [&] { k_beam_head<WP, EXACT>(a, t); });
}
int main(int argc, char **argv) {
    if (argc != 8) return 2;
    std::string d = argv[1];
    BeamHeadArgs a{};
    a.N = atoi(argv[2]); a.streams = atoi(argv[3]); a.W = atoi(argv[4]); a.count = atoi(argv[5]);
    const int steps = atoi(argv[6]);
    a.stop_byte = atoi(argv[7]);
    auto Why = load<float>((d + "/why.bin").c_str()), by = load<float>((d + "/by.bin").c_str());
    auto Hs = load<float>((d + "/hs.bin").c_str()), Cs = load<float>((d + "/cs.bin").c_str());
    auto off = load<uint64_t>((d + "/off.bin").c_str());
    auto prompts = load<uint8_t>((d + "/prompts.bin").c_str());
    const size_t cols = (size_t)a.streams * a.W, n = (size_t)a.N * cols, nd = (size_t)a.count * cols;
    std::vector<uint8_t> tp(nd, 0), tb(nd, 0);
    std::vector<double> cost(cols, (double)INFINITY), costlog;
    for (int s = 0; s < a.streams; s++) cost[(size_t)s * a.W] = 0.0;
    std::vector<int32_t> len(cols, 0), fin(cols, 0), xn(cols, -7), xlog, lenlog, finlog;
    std::vector<float> hr(n), cr(n), hrlog, crlog;
    a.Why = Why.data(); a.by = by.data(); a.prompts = prompts.data(); a.off = off.data(); a.x_next = xn.data();
    a.cost = cost.data(); a.len = len.data(); a.fin = fin.data(); a.trace_parent = tp.data(); a.trace_byte = tb.data();
    a.Hr = hr.data(); a.Cr = cr.data();
    for (long long t = 0; t < steps; t++) {
        a.H = Hs.data() + t * n; a.C = Cs.data() + t * n;
        switch (a.W) {
        case 1: launch<1, true>(a, t); break;
        case 4: launch<4, true>(a, t); break;
        case 5: launch<8, false>(a, t); break;
        case 32: launch<32, true>(a, t); break;
        default: return 2;
        }
        xlog.insert(xlog.end(), xn.begin(), xn.end());
        costlog.insert(costlog.end(), cost.begin(), cost.end());
        lenlog.insert(lenlog.end(), len.begin(), len.end());
        finlog.insert(finlog.end(), fin.begin(), fin.end());
        hrlog.insert(hrlog.end(), hr.begin(), hr.end());
        crlog.insert(crlog.end(), cr.begin(), cr.end());
    }
    save((d + "/tp.bin").c_str(), tp); save((d + "/tb.bin").c_str(), tb); save((d + "/xlog.bin").c_str(), xlog);
    save((d + "/costlog.bin").c_str(), costlog); save((d + "/lenlog.bin").c_str(), lenlog); save((d + "/finlog.bin").c_str(), finlog);
    save((d + "/hr.bin").c_str(), hrlog); save((d + "/cr.bin").c_str(), crlog);
    return 0;
}
