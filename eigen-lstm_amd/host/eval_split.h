// eval_split.h -- texts cut into streams for lstm_hip_eval_texts (include/lstm_hip.h): what
// lstm --test-streams and lstm_generate --score-streams share.  Host only.
//
// A text of L >= 2 bytes in `pieces` streams: piece i scores the bytes a_i .. a_{i+1} - 1 with
// a_i = 1 + floor(i (L - 1) / pieces); its stream is text[max(0, a_i - 1 - warm) .. a_{i+1}) and its skip a_i minus that
// start, so the bytes before a_i are fed from a zero state as warm-up and every byte 1 .. L - 1 is scored exactly once.
// With pieces = 1 that is the one stream lstm_hip_eval_bits runs.
#pragma once
#include "../../include/lstm_hip.h"

#include <algorithm>
#include <cstdint>
#include <vector>

struct EvalSplit {
    std::vector<uint8_t> bytes;      // the streams, back to back (neighbours overlap, so they are copies)
    std::vector<uint64_t> off{0};    // [streams + 1]
    std::vector<uint64_t> skip;      // [streams]
    std::vector<size_t> first{0};    // [texts + 1]: the streams of text f are first[f] .. first[f + 1] - 1

    void add(const uint8_t *text, size_t L, size_t pieces, size_t warm) {
        for (size_t i = 0; i < pieces; i++) {
            // (i * (L - 1) stays inside 64 bits for every text that fits in memory with pieces <= 2^20)
            const size_t a = 1 + (size_t)((unsigned __int128)i * (L - 1) / pieces);
            const size_t b = 1 + (size_t)((unsigned __int128)(i + 1) * (L - 1) / pieces);
            const size_t start = a - 1 > warm ? a - 1 - warm : 0;
            bytes.insert(bytes.end(), text + start, text + b);
            off.push_back(bytes.size());
            skip.push_back(a - start);
        }
        first.push_back(skip.size());
    }
    // bits[f]: the summed bits of text f's pieces.  lanes: at most as many as there are streams
    int run(lstm_hip_t *h, std::vector<double> &bits) const {
        const size_t streams = skip.size();
        std::vector<double> per(streams);
        const lstm_hip_eval_opt opt{(uint32_t)sizeof(lstm_hip_eval_opt), (int32_t)std::min<size_t>(streams, 4096)};
        const int rc = lstm_hip_eval_texts(h, (int32_t)streams, bytes.data(), off.data(), nullptr, nullptr, skip.data(), &opt,
                                           per.data(), nullptr, nullptr, nullptr, nullptr);
        if (rc != 0) return rc;
        bits.assign(first.size() - 1, 0.0);
        for (size_t f = 0; f + 1 < first.size(); f++)
            for (size_t s = first[f]; s < first[f + 1]; s++) bits[f] += per[s];
        return 0;
    }
};
