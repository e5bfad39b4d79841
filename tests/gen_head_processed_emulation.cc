// Host emulation of k_gen_head<SB, false, true, CONSTRAIN, DEADLINE, true>, the PROCESS instantiations (eigen-lstm_amd/csrc/kernels.hip),
// for tests/test_processed_head_emulation_cpu.py, as tests/gen_head_deadline_emulation.cc emulates the DEADLINE one: the kernel's
// own text (csrc/heads/gen_head.inc, the file kernels.hip includes) compiled for the host over tests/device_shim.h, one
// std::thread per work-item, a std::barrier for __syncthreads, function-static arrays for LDS.  It checks the head's logic --
// the bias, the n-gram scan over the uploaded text and the stream's column of out, the ban mask, the survivor count and the
// drop rule, the min-p walk behind the nucleus walk, the replacement rule -- without a device; it says nothing about the GPU
// build.
//   gen_head_processed_emulation DIR N streams count steps SB mode tau keep_k nucleus top_p filter stop_byte table has_bias
//                                min_p no_repeat
// table: 0 none, 1 a byte automaton, 2 with accepting states.  Reads why, by, hs ([steps+1][streams][N], the state before each
// step), u, off, prompts, and with a table tab, cnt, q, with accepting states acc, frows, with has_bias bias ([256] float), with
// no_repeat ptext, ptoff (each stream's history ++ prompt) (.bin) from DIR and writes out, kept, end, ho, xlog (x_next after
// every step), bits, qend.
#include "device_shim.h"
inline unsigned atomicOr(unsigned *p, unsigned v) { std::lock_guard<std::mutex> l(g_mu); unsigned o = *p; *p = o | v; return o; }
#include "heads/head_args.h"
using namespace lstmk;
#include "heads/lse_surprisal.h"
#include "heads/gen_head.inc"

template <int SB> void launch(const GenHeadArgs &a, long long t) {
    const int grid = (a.streams + SB - 1) / SB;
    if (a.frows) run_blocks(grid, [&] { k_gen_head<SB, false, true, true, true, true>(a, t); });
    else if (a.ctab) run_blocks(grid, [&] { k_gen_head<SB, false, true, true, false, true>(a, t); });
    else run_blocks(grid, [&] { k_gen_head<SB, false, true, false, false, true>(a, t); });
}
int main(int argc, char **argv) {
    if (argc != 18) return 2;
    std::string d = argv[1];
    GenHeadArgs a{};
    a.N = atoi(argv[2]); a.streams = atoi(argv[3]); a.count = atoi(argv[4]);
    const int steps = atoi(argv[5]), sb = atoi(argv[6]);
    a.mode = atoi(argv[7]); a.tau = (float)atof(argv[8]); a.keep_k = atoi(argv[9]); a.nucleus = atoi(argv[10]);
    a.top_p = (float)atof(argv[11]); a.filter = atoi(argv[12]); a.stop_byte = atoi(argv[13]);
    const int table = atoi(argv[14]), has_bias = atoi(argv[15]);
    a.process = 1; a.min_p = (float)atof(argv[16]); a.no_repeat = atoi(argv[17]);
    auto Why = load<float>((d + "/why.bin").c_str()), by = load<float>((d + "/by.bin").c_str());
    auto Hs = load<float>((d + "/hs.bin").c_str());   // [steps+1][streams][N]
    auto u = load<double>((d + "/u.bin").c_str());
    auto off = load<uint64_t>((d + "/off.bin").c_str());
    auto prompts = load<uint8_t>((d + "/prompts.bin").c_str());
    std::vector<uint16_t> tab, cnt; std::vector<int32_t> q(a.streams, 0); std::vector<uint8_t> acc, ptext; std::vector<uint32_t> frows;
    std::vector<float> bias; std::vector<uint64_t> ptoff;
    if (table >= 1) {
        tab = load<uint16_t>((d + "/tab.bin").c_str()); cnt = load<uint16_t>((d + "/cnt.bin").c_str());
        q = load<int32_t>((d + "/q.bin").c_str());
        a.ctab = tab.data(); a.ccount = cnt.data(); a.cstate = q.data();
    }
    if (table == 2) {
        acc = load<uint8_t>((d + "/acc.bin").c_str()); frows = load<uint32_t>((d + "/frows.bin").c_str());
        a.accept = acc.data(); a.frows = frows.data(); a.fwords = ((int)cnt.size() + 31) / 32;
    }
    if (has_bias) { bias = load<float>((d + "/bias.bin").c_str()); a.bias = bias.data(); }
    if (a.no_repeat > 0) {
        ptext = load<uint8_t>((d + "/ptext.bin").c_str()); ptoff = load<uint64_t>((d + "/ptoff.bin").c_str());
        a.ptext = ptext.data(); a.ptoff = ptoff.data();
    }
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
