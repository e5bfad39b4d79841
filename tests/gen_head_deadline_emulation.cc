// Host emulation of k_gen_head<SB, false, true, true, true>, the DEADLINE instantiation (eigen-lstm_amd/csrc/kernels.hip), for
// tests/test_deadline_head_emulation_cpu.py, as tests/gen_head_constrained_emulation.cc emulates the CONSTRAIN one: the kernel's own text
// (csrc/heads/gen_head.inc, the file kernels.hip includes) compiled for the host over tests/device_shim.h, one std::thread
// per work-item, a std::barrier for __syncthreads, function-static arrays for LDS.  It checks the head's logic -- the bytes
// that exist within the deadline, their count in the group, the masked logits, ranks, the capped keep, nucleus walk,
// renormalisation, CDF walk, the automaton's advance, stop index, final-state copy -- without a device; it says nothing about
// the GPU build.
//   gen_head_deadline_emulation DIR N streams count steps SB mode tau keep_k nucleus top_p filter stop_byte
// reads why, by, hs ([steps+1][streams][N], the state before each step), u, off, prompts, tab ([states][256] uint16), cnt
// ([states] uint16), q ([streams] int32: the state after each prompt), acc ([states] uint8), frows ([count][fwords] uint32)
// (.bin) from DIR and writes out, kept, end, ho, xlog
// (x_next after every step), bits, qend ([streams] the final automaton states).
#include "device_shim.h"
#include "heads/head_args.h"
using namespace lstmk;
#include "heads/lse_surprisal.h"
#include "heads/gen_head.inc"

template <int SB> void launch(const GenHeadArgs &a, long long t) {
    run_blocks((a.streams + SB - 1) / SB, [&] { k_gen_head<SB, false, true, true, true>(a, t); });
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
    auto tab = load<uint16_t>((d + "/tab.bin").c_str()), cnt = load<uint16_t>((d + "/cnt.bin").c_str());
    auto q = load<int32_t>((d + "/q.bin").c_str());
    a.ctab = tab.data(); a.ccount = cnt.data(); a.cstate = q.data();
    auto acc = load<uint8_t>((d + "/acc.bin").c_str());
    auto frows = load<uint32_t>((d + "/frows.bin").c_str());
    a.accept = acc.data(); a.frows = frows.data(); a.fwords = ((int)cnt.size() + 31) / 32;
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
    save((d + "/qend.bin").c_str(), q);
    return 0;
}
