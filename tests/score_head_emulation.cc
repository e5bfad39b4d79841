// Host emulation of k_score_head (eigen-lstm_amd/csrc/kernels.hip), for
// tests/test_score_head_emulation_cpu.py, as tests/gen_head_constrained_emulation.cc emulates the generator's head: the
// kernel's own text (csrc/heads/score_head.inc, the file kernels.hip includes, with heads/head_args.h and
// heads/lse_surprisal.h) compiled for the host over tests/device_shim.h, one std::thread per work-item, a std::barrier for
// __syncthreads, function-static arrays for LDS.  It checks the head's logic -- which bytes are scored, the masked logits, the serial sums,
// ranks, alternatives, the bits, the next inputs, the final-state copy -- without a device; it says nothing about the GPU build.
//   score_head_emulation DIR N streams steps SB stable detail constrain first top_n
// reads why, by, hs ([steps+1][streams][N], the state before each step), off, text, tab ([states][256] uint16), qpos ([total]
// uint16) (.bin) from DIR and writes surprisal, entropy, rank, top_byte, top_bits, bits, ho, xlog (x_next after every step).
#include "device_shim.h"
#include "heads/head_args.h"
using namespace lstmk;
#include "heads/lse_surprisal.h"
#include "heads/score_head.inc"

template <int SB, bool STABLE, bool DETAIL, bool CONSTRAIN> void launch(const ScoreHeadArgs &a, long long t) {
    run_blocks((a.streams + SB - 1) / SB, [&] { k_score_head<SB, STABLE, DETAIL, CONSTRAIN>(a, t); });
}
template <int SB> void launch_sb(const ScoreHeadArgs &a, long long t, int variant) {
    switch (variant) {
    case 0: return launch<SB, false, false, false>(a, t);
    case 1: return launch<SB, false, false, true>(a, t);
    case 2: return launch<SB, false, true, false>(a, t);
    case 3: return launch<SB, false, true, true>(a, t);
    case 4: return launch<SB, true, false, false>(a, t);
    case 5: return launch<SB, true, false, true>(a, t);
    case 6: return launch<SB, true, true, false>(a, t);
    default: return launch<SB, true, true, true>(a, t);
    }
}
int main(int argc, char **argv) {
    if (argc != 11) return 2;
    std::string d = argv[1];
    ScoreHeadArgs a{};
    a.N = atoi(argv[2]); a.streams = atoi(argv[3]);
    const int steps = atoi(argv[4]), sb = atoi(argv[5]), stable = atoi(argv[6]), detail = atoi(argv[7]), constrain = atoi(argv[8]);
    a.first = atoi(argv[9]); a.top_n = atoi(argv[10]);
    auto Why = load<float>((d + "/why.bin").c_str()), by = load<float>((d + "/by.bin").c_str());
    auto Hs = load<float>((d + "/hs.bin").c_str());   // [steps+1][streams][N]
    auto off = load<uint64_t>((d + "/off.bin").c_str());
    auto text = load<uint8_t>((d + "/text.bin").c_str());
    auto tab = load<uint16_t>((d + "/tab.bin").c_str()), qpos = load<uint16_t>((d + "/qpos.bin").c_str());
    const size_t n = (size_t)a.N * a.streams, total = off[a.streams], tn = total * (size_t)a.top_n;
    std::vector<float> sur(total, 0.f), ent(total, 0.f), tbi(tn, 0.f), ho(n, -7.f), co(n, -7.f);
    std::vector<uint8_t> rank(total, 0), tby(tn, 0);
    std::vector<double> bits(a.streams, 0.0);
    std::vector<int32_t> xn(a.streams), xlog;
    a.Why = Why.data(); a.by = by.data(); a.text = text.data(); a.off = off.data();
    a.surprisal = sur.data(); a.entropy = ent.data(); a.bits = bits.data(); a.x_next = xn.data(); a.h_out = ho.data(); a.c_out = co.data();
    if (detail) { a.rank = rank.data(); if (a.top_n) { a.top_byte = tby.data(); a.top_bits = tbi.data(); } }
    if (constrain) { a.ctab = tab.data(); a.qpos = qpos.data(); }
    const int variant = stable * 4 + detail * 2 + constrain;
    for (long long t = 0; t <= steps; t++) {
        a.H = Hs.data() + t * n; a.C = a.H;
        if (sb == 1) launch_sb<1>(a, t, variant); else if (sb == 4) launch_sb<4>(a, t, variant); else launch_sb<16>(a, t, variant);
        xlog.insert(xlog.end(), xn.begin(), xn.end());
    }
    save((d + "/surprisal.bin").c_str(), sur); save((d + "/entropy.bin").c_str(), ent); save((d + "/rank.bin").c_str(), rank);
    save((d + "/top_byte.bin").c_str(), tby); save((d + "/top_bits.bin").c_str(), tbi); save((d + "/bits.bin").c_str(), bits);
    save((d + "/ho.bin").c_str(), ho); save((d + "/xlog.bin").c_str(), xlog);
    return 0;
}
