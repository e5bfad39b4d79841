// Host emulation of k_guide_logits<SB> and of the two heads that mix its sum in -- k_gen_head's PROCESS instantiations and
// k_score_head with a.gsum set (eigen-lstm_amd/csrc/kernels.hip) -- for
// tests/test_guided_head_emulation_cpu.py, as tests/gen_head_processed_emulation.cc emulates the processed head: the kernels'
// own text (csrc/heads/guide_logits.inc, gen_head.inc, score_head.inc, the files kernels.hip includes) compiled for the host
// over tests/device_shim.h, one std::thread per work-item, a std::barrier for __syncthreads, function-static arrays for LDS.
// Per step it runs what the library launches: the guides' kernel, then the head.  It checks the logic -- which streams get a
// sum, the index-order mix, the guides' end states, the mixed logit ahead of the bias and of the mask -- without a device; it
// says nothing about the GPU build.
//   guided_head_emulation DIR head N streams count steps SB mode tau keep_k nucleus top_p stop_byte table has_bias nguides wmain
//                         first top_n
// head: 0 the generator's, 1 the scorer's (count, mode .. has_bias are then unused).  table: 0 none, 1 a byte automaton.  Reads
// why, by, hs ([steps+1][streams][N], the state before each step), off, prompts (the scorer's text), u, with a table tab, cnt, q
// (generator) or qpos (scorer), with has_bias bias, gn ([nguides] int32 widths), gw ([nguides] float weights) and per guide k
// g<k>_why, g<k>_by, g<k>_hs, g<k>_cs (.bin) from DIR.  Writes glog ([steps+1][streams][256]: gsum after every step's launch,
// filled with -7 before it), g<k>_ho, g<k>_co, ho, xlog and the head's outputs: out, kept, end, bits, qend (generator) or
// surprisal, entropy, rank, top_byte, top_bits, bits (scorer).
#include "device_shim.h"
#include "heads/head_args.h"
using namespace lstmk;
#include "heads/lse_surprisal.h"
#include "heads/gen_head.inc"
#include "heads/guide_logits.inc"
#include "heads/score_head.inc"

template <int SB> void launch(const GuideLogitsArgs &ga, const GenHeadArgs *a, const ScoreHeadArgs *b, long long t) {
    const int grid = (ga.streams + SB - 1) / SB;
    run_blocks(grid, [&] { k_guide_logits<SB>(ga, t); });
    if (a && a->ctab) run_blocks(grid, [&] { k_gen_head<SB, false, true, true, false, true>(*a, t); });
    else if (a) run_blocks(grid, [&] { k_gen_head<SB, false, true, false, false, true>(*a, t); });
    else if (b->ctab) run_blocks(grid, [&] { k_score_head<SB, false, true, true>(*b, t); });
    else run_blocks(grid, [&] { k_score_head<SB, false, true, false>(*b, t); });
}
int main(int argc, char **argv) {
    if (argc != 20) return 2;
    std::string d = argv[1];
    const int head = atoi(argv[2]), N = atoi(argv[3]), streams = atoi(argv[4]), count = atoi(argv[5]), steps = atoi(argv[6]),
              sb = atoi(argv[7]), table = atoi(argv[14]), has_bias = atoi(argv[15]), nguides = atoi(argv[16]);
    if (nguides < 1 || nguides > MAX_GUIDES) return 2;
    auto F = [&](const std::string &name) { return d + "/" + name + ".bin"; };
    auto Why = load<float>(F("why").c_str()), by = load<float>(F("by").c_str()), Hs = load<float>(F("hs").c_str());
    auto off = load<uint64_t>(F("off").c_str());
    auto prompts = load<uint8_t>(F("prompts").c_str());
    auto gn = load<int32_t>(F("gn").c_str());
    auto gw = load<float>(F("gw").c_str());
    std::vector<float> gWhy[MAX_GUIDES], gby[MAX_GUIDES], gHs[MAX_GUIDES], gCs[MAX_GUIDES], gho[MAX_GUIDES], gco[MAX_GUIDES];
    const size_t n = (size_t)N * streams, nd = (size_t)count * streams, total = off[streams];
    std::vector<float> gsum((size_t)streams * 256), glog;
    std::vector<int32_t> end(streams, count), xn(streams), xlog, q(streams, 0);
    GuideLogitsArgs ga{};
    ga.nguides = nguides; ga.streams = streams; ga.gsum = gsum.data(); ga.off = off.data();
    ga.scorer = head; ga.end = end.data(); ga.count = count; ga.first = atoi(argv[18]);
    for (int k = 0; k < nguides; k++) {
        const std::string g = "g" + std::to_string(k) + "_";
        gWhy[k] = load<float>(F(g + "why").c_str()); gby[k] = load<float>(F(g + "by").c_str());
        gHs[k] = load<float>(F(g + "hs").c_str()); gCs[k] = load<float>(F(g + "cs").c_str());
        gho[k].assign((size_t)gn[k] * streams, -7.f); gco[k].assign((size_t)gn[k] * streams, -7.f);
        ga.Why[k] = gWhy[k].data(); ga.by[k] = gby[k].data(); ga.h_out[k] = gho[k].data(); ga.c_out[k] = gco[k].data();
        ga.N[k] = gn[k]; ga.w[k] = gw[k];
    }
    std::vector<float> ho(n, -7.f), co(n, -7.f), bias, u_unused;
    std::vector<double> bits(streams, 0.0), u;
    std::vector<uint16_t> tab, cnt, qpos, kept(nd, 0);
    std::vector<uint8_t> out(nd, 0);
    GenHeadArgs a{};
    ScoreHeadArgs b{};
    const int top_n = atoi(argv[19]);
    std::vector<float> sur(total, 0.f), ent(total, 0.f), tbi(total * (size_t)top_n, 0.f);
    std::vector<uint8_t> rank(total, 0), tby(total * (size_t)top_n, 0);
    if (table) tab = load<uint16_t>(F("tab").c_str());
    if (head == 0) {
        u = load<double>(F("u").c_str());
        a.Why = Why.data(); a.by = by.data(); a.prompts = prompts.data(); a.off = off.data(); a.u = u.data(); a.out = out.data();
        a.bits = bits.data(); a.x_next = xn.data(); a.h_out = ho.data(); a.c_out = co.data(); a.end = end.data(); a.kept = kept.data();
        a.N = N; a.streams = streams; a.count = count;
        a.mode = atoi(argv[8]); a.tau = (float)atof(argv[9]); a.keep_k = atoi(argv[10]); a.nucleus = atoi(argv[11]);
        a.top_p = (float)atof(argv[12]); a.filter = a.keep_k < 256 || a.nucleus; a.stop_byte = atoi(argv[13]);
        a.process = 1; a.gsum = gsum.data(); a.wmain = (float)atof(argv[17]);
        if (table) {
            cnt = load<uint16_t>(F("cnt").c_str()); q = load<int32_t>(F("q").c_str());
            a.ctab = tab.data(); a.ccount = cnt.data(); a.cstate = q.data();
        }
        if (has_bias) { bias = load<float>(F("bias").c_str()); a.bias = bias.data(); }
    } else {
        b.Why = Why.data(); b.by = by.data(); b.text = prompts.data(); b.off = off.data();
        b.surprisal = sur.data(); b.entropy = ent.data(); b.rank = rank.data(); b.bits = bits.data(); b.x_next = xn.data();
        b.h_out = ho.data(); b.c_out = co.data(); b.N = N; b.streams = streams; b.first = ga.first; b.top_n = top_n;
        if (top_n) { b.top_byte = tby.data(); b.top_bits = tbi.data(); }
        if (table) { qpos = load<uint16_t>(F("qpos").c_str()); b.ctab = tab.data(); b.qpos = qpos.data(); }
        b.gsum = gsum.data(); b.wmain = (float)atof(argv[17]);
    }
    for (long long t = 0; t <= steps; t++) {
        a.H = b.H = Hs.data() + t * n; a.C = b.C = a.H;
        for (int k = 0; k < nguides; k++) {
            ga.H[k] = gHs[k].data() + t * (size_t)gn[k] * streams;
            ga.C[k] = gCs[k].data() + t * (size_t)gn[k] * streams;
        }
        std::fill(gsum.begin(), gsum.end(), -7.f);
        const GenHeadArgs *pa = head == 0 ? &a : nullptr;
        if (sb == 1) launch<1>(ga, pa, &b, t); else launch<2>(ga, pa, &b, t);
        glog.insert(glog.end(), gsum.begin(), gsum.end());
        xlog.insert(xlog.end(), xn.begin(), xn.end());
    }
    save(F("glog").c_str(), glog); save(F("ho").c_str(), ho); save(F("xlog").c_str(), xlog); save(F("bits").c_str(), bits);
    for (int k = 0; k < nguides; k++) {
        save(F("g" + std::to_string(k) + "_ho").c_str(), gho[k]); save(F("g" + std::to_string(k) + "_co").c_str(), gco[k]);
    }
    if (head == 0) {
        save(F("out").c_str(), out); save(F("kept").c_str(), kept); save(F("end").c_str(), end); save(F("qend").c_str(), q);
    } else {
        save(F("surprisal").c_str(), sur); save(F("entropy").c_str(), ent); save(F("rank").c_str(), rank);
        save(F("top_byte").c_str(), tby); save(F("top_bits").c_str(), tbi);
    }
    return 0;
}
