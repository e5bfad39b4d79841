// Host emulation of k_code_head (eigen-lstm_amd/csrc/kernels.hip), for
// tests/test_code_head_emulation_cpu.py, as tests/score_head_emulation.cc emulates the scorer's head: the kernel's own text
// (csrc/heads/code_head.inc, the file kernels.hip includes, with heads/head_args.h) compiled for the host over
// tests/device_shim.h, one std::thread per work-item, a std::barrier for __syncthreads, function-static arrays for LDS.  It
// checks the head's logic -- which streams are coded, the whole frequency table behind every coded byte, the range coder's
// bytes and state, the bits, the next inputs, the error word -- without a device; it says nothing about the GPU build.
//   code_head_emulation DIR N streams steps SB decode
// reads why ([N][256]), by, hs ([steps+1][streams][N], the state before each step), text_off, text, code, code_base (.bin) from
// DIR; text and code are the whole buffers, the one the direction writes holding the caller's sentinels.  Runs steps
// t = 0 .. steps with the CoderState array carried between them as the API carries it, and writes code_out, text_out, trace
// ([total][3]), bits, code_len, state ([streams] CoderState), xlog (x_next after every step) and err.
#include "device_shim.h"
#include "heads/head_args.h"
using namespace lstmk;
#include "heads/code_head.inc"

template <int SB> void launch(const CodeHeadArgs &a, long long t) {
    run_blocks((a.streams + SB - 1) / SB, [&] { k_code_head<SB>(a, t); });
}
int main(int argc, char **argv) {
    if (argc != 7) return 2;
    std::string d = argv[1];
    CodeHeadArgs a{};
    a.N = atoi(argv[2]); a.streams = atoi(argv[3]);
    const int steps = atoi(argv[4]), sb = atoi(argv[5]);
    a.decode = atoi(argv[6]);
    auto Why = load<float>((d + "/why.bin").c_str()), by = load<float>((d + "/by.bin").c_str());
    auto Hs = load<float>((d + "/hs.bin").c_str());   // [steps+1][streams][N]
    auto text_off = load<uint64_t>((d + "/text_off.bin").c_str()), code_base = load<uint64_t>((d + "/code_base.bin").c_str());
    auto text = load<uint8_t>((d + "/text.bin").c_str()), code = load<uint8_t>((d + "/code.bin").c_str());
    const size_t n = (size_t)a.N * a.streams, total = text_off[a.streams];
    if (Hs.size() != n * (steps + 1) || text.size() < total + 1) return 3;
    std::vector<uint32_t> trace(3 * total + 3, 0u), err(1, 0u);
    std::vector<double> bits(a.streams, 0.0);
    std::vector<uint64_t> code_len(a.streams, 0);
    std::vector<CoderState> state(a.streams);
    memset(state.data(), 0xEE, state.size() * sizeof(CoderState)); // (a step that read a state before writing it would show)
    std::vector<int32_t> xn(a.streams, -7), xlog;
    a.Why = Why.data(); a.by = by.data(); a.text_off = text_off.data(); a.text = text.data(); a.code = code.data();
    a.code_base = code_base.data(); a.code_len = code_len.data(); a.state = state.data(); a.x_next = xn.data(); a.err = err.data();
    if (!a.decode) { a.bits = bits.data(); a.trace = trace.data(); }
    for (long long t = 0; t <= steps; t++) {
        a.H = Hs.data() + t * n;
        switch (sb) {
        case 1: launch<1>(a, t); break;
        case 2: launch<2>(a, t); break;
        case 4: launch<4>(a, t); break;
        case 8: launch<8>(a, t); break;
        case 16: launch<16>(a, t); break;
        default: return 2;
        }
        xlog.insert(xlog.end(), xn.begin(), xn.end());
    }
    save((d + "/code_out.bin").c_str(), code); save((d + "/text_out.bin").c_str(), text); save((d + "/trace.bin").c_str(), trace);
    save((d + "/bits.bin").c_str(), bits); save((d + "/code_len.bin").c_str(), code_len); save((d + "/state.bin").c_str(), state);
    save((d + "/xlog.bin").c_str(), xlog); save((d + "/err.bin").c_str(), err);
    return 0;
}
