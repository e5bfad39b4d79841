// Host emulation of k_beam_head's CONSTRAIN instantiation (eigen-lstm_amd/csrc/kernels.hip) for
// tests/test_beam_head_constrained_emulation_cpu.py, made as tests/beam_head_emulation.cc makes the unconstrained one: the
// kernel's own text (csrc/heads/beam_head.inc, the file kernels.hip includes, with heads/head_args.h and
// heads/lse_surprisal.h) compiled for the host over tests/device_shim.h, one std::thread per work-item, a std::barrier for
// __syncthreads, function-static arrays for LDS, cross-lane shuffles through a table.  It checks the head's logic under a table -- the two masks, the masked
// max and sum, the W selection rounds over the candidates that exist, tables, costs, lengths, flags, next inputs, the new
// states, the gather -- without a device; it says nothing about the GPU build.
//   beam_head_constrained_emulation DIR N streams W count steps stop_byte states has_accept
// reads why, by, hs and cs ([steps][streams*W][N], the state before each step), off, prompts, table ([states][256]), q0 (the
// slots' start states), and with has_accept accept ([states]) and frows ([count][(states + 31) / 32]) (.bin) from DIR and
// writes the tables tp / tb, and per step xlog, costlog, lenlog, finlog, qlog, hr, cr.  Slots 1..W-1 start finished.
#include "device_shim.h"
#include "heads/head_args.h"
using namespace lstmk;
#include "heads/lse_surprisal.h"
#include "heads/beam_head.inc"

template <int WP, bool EXACT> void launch(const BeamHeadArgs &a, long long t) {
    run_blocks(a.streams, [&] { k_beam_head<WP, EXACT, true>(a, t); });
}
int main(int argc, char **argv) {
    if (argc != 10) return 2;
    std::string d = argv[1];
    BeamHeadArgs a{};
    a.N = atoi(argv[2]); a.streams = atoi(argv[3]); a.W = atoi(argv[4]); a.count = atoi(argv[5]);
    const int steps = atoi(argv[6]);
    a.stop_byte = atoi(argv[7]);
    const int Q = atoi(argv[8]), has_accept = atoi(argv[9]);
    auto table = load<uint16_t>((d + "/table.bin").c_str());
    auto q = load<int32_t>((d + "/q0.bin").c_str());
    std::vector<uint8_t> accept;
    std::vector<uint32_t> frows;
    if (has_accept) {
        accept = load<uint8_t>((d + "/accept.bin").c_str());
        frows = load<uint32_t>((d + "/frows.bin").c_str());
    }
    if (table.size() != (size_t)Q * 256) return 2;
    auto Why = load<float>((d + "/why.bin").c_str()), by = load<float>((d + "/by.bin").c_str());
    auto Hs = load<float>((d + "/hs.bin").c_str()), Cs = load<float>((d + "/cs.bin").c_str());
    auto off = load<uint64_t>((d + "/off.bin").c_str());
    auto prompts = load<uint8_t>((d + "/prompts.bin").c_str());
    const size_t cols = (size_t)a.streams * a.W, n = (size_t)a.N * cols, nd = (size_t)a.count * cols;
    std::vector<uint8_t> tp(nd, 0), tb(nd, 0);
    std::vector<double> cost(cols, (double)INFINITY), costlog;
    for (int s = 0; s < a.streams; s++) cost[(size_t)s * a.W] = 0.0;
    std::vector<int32_t> len(cols, 0), fin(cols, 1), xn(cols, -7), xlog, lenlog, finlog, qlog;
    for (int s = 0; s < a.streams; s++) fin[(size_t)s * a.W] = 0;
    if (q.size() != cols) return 2;
    std::vector<float> hr(n), cr(n), hrlog, crlog;
    a.Why = Why.data(); a.by = by.data(); a.prompts = prompts.data(); a.off = off.data(); a.x_next = xn.data();
    a.cost = cost.data(); a.len = len.data(); a.fin = fin.data(); a.trace_parent = tp.data(); a.trace_byte = tb.data();
    a.Hr = hr.data(); a.Cr = cr.data();
    a.ctab = table.data(); a.cstate = q.data(); a.fwords = (Q + 31) / 32;
    a.accept = has_accept ? accept.data() : nullptr; a.frows = has_accept ? frows.data() : nullptr;
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
        qlog.insert(qlog.end(), q.begin(), q.end());
        hrlog.insert(hrlog.end(), hr.begin(), hr.end());
        crlog.insert(crlog.end(), cr.begin(), cr.end());
    }
    save((d + "/tp.bin").c_str(), tp); save((d + "/tb.bin").c_str(), tb); save((d + "/xlog.bin").c_str(), xlog);
    save((d + "/costlog.bin").c_str(), costlog); save((d + "/lenlog.bin").c_str(), lenlog); save((d + "/finlog.bin").c_str(), finlog);
    save((d + "/qlog.bin").c_str(), qlog);
    save((d + "/hr.bin").c_str(), hrlog); save((d + "/cr.bin").c_str(), crlog);
    return 0;
}
