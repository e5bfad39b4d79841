// head_args.h -- the argument blocks of the inference heads (k_gen_head, k_guide_logits, k_beam_head, k_code_head, k_score_head), in plain
// C++ so that the host emulations under tests/ compile the same declarations as the library.  kernels.h includes it and
// declares the launchers.
#pragma once
#include <stdint.h>

namespace lstmk {

// ---- batched generator (lstm_hip_generate): per step gen_head on the state after t inputs, then fwd_step over all
// streams with x_next as inputs.  Arrays are [streams] or [count][streams]; H, C, h_out, c_out are [streams][N], N % 16 == 0
struct GenHeadArgs {
    const float *Why, *by;
    const float *H, *C;         // state after t inputs
    const uint8_t *prompts;     // concatenated prompts (null: none)
    const uint64_t *off;        // streams + 1 prompt offsets (null: no prompts)
    const double *u;            // draws [count][streams] (null when mode == 2)
    uint8_t *out;               // drawn bytes [count][streams]
    double *bits;               // prompt bits per stream, accumulated (null: not scored)
    int32_t *x_next;            // the next input of every stream (-1: none)
    float *h_out, *c_out;       // the state after each stream's last input (null: not kept)
    int N, streams, count;
    int mode;                   // 0: temperature 1 (expf as the sampler: unshifted, or shifted when stable), 1: tempered, 2: greedy
    float tau;
    // sampling controls (lstm_hip_generate_ex): read only by the FILTER instantiation, which
    // gen_head takes when `end` is set
    int keep_k;                 // top-k: 1..255, or 256 (off)
    int nucleus;                // 1: top_p < 1 was asked for
    float top_p;                // (float)top_p, the mass the nucleus prefix has to reach
    int filter;                 // 1: top-k or nucleus on (tempered draws are filtered)
    int stop_byte;              // -1: none; else a stream ends with its first drawn byte equal to it
    int32_t *end;               // [streams] number of bytes each stream draws: `count` at the start, i + 1 once draw i stops it
    uint16_t *kept;             // [count][streams] bytes kept per draw (null: not wanted); zeroed by the caller
    // byte automaton (lstm_hip_generate_constrained): read only by the CONSTRAIN instantiation, which
    // gen_head takes when `ctab` is set (`end` is set with it)
    const uint16_t *ctab;       // [states][256] the state after byte b in state q, 0xFFFF: b is forbidden there
    const uint16_t *ccount;     // [states] allowed bytes of each state (>= 1 for every state a stream can reach)
    int32_t *cstate;            // [streams] the state of every stream: after its prompt at the start, then after each drawn byte
    // accepting states (lstm_hip_generate_accepting): read only by the DEADLINE instantiation, which
    // gen_head takes when `frows` is set (`ctab` is set with it); all null / 0 otherwise
    const uint8_t *accept;      // [states] nonzero: a stream may end there
    const uint32_t *frows;      // [count][fwords] bit q of row R: an accepted end can be reached from q with R more bytes
    int fwords;                 // words of one row: (states + 31) / 32
    // logit processors (lstm_hip_generate_processed): read only by the PROCESS instantiation, which
    // gen_head takes when `process` is set (`end` is set with it); all null / 0 otherwise
    int process;                // 1: some processor is on (a tempered draw is then a filtered one)
    const float *bias;          // [256] added to the logits of a drawn byte (null: none)
    float min_p;                // (float)min_p: 0 off, else terms below min_p * the largest term are cut
    int no_repeat;              // n: 0 off, else 1..64
    const uint8_t *ptext;       // each stream's history ++ prompt, concatenated (null: all empty); with no_repeat
    const uint64_t *ptoff;      // streams + 1 offsets into ptext; with no_repeat
    // guides (lstm_hip_generate_guided): read only by the PROCESS instantiation (`process` is set with
    // it); null / 0 otherwise
    const float *gsum;          // [streams][256] the guides' weighted logit sum of this step, written by k_guide_logits (null: none)
    float wmain;                // (float)main_weight: a drawn byte's logit becomes wmain * z + gsum ahead of the bias
};

// ---- guides (lstm_hip_generate_guided / lstm_hip_score_guided): per step guide_logits on every guide's
// state after t inputs, ahead of the head: gsum[s][m] = w[0] * z^0_m, then + w[k] * z^k_m for k = 1.. in index order, for the
// streams whose head needs logits at this step; and each guide's state to its h_out / c_out at the step where the head copies
// the main model's.  Afterwards one fwd_step per guide on the head's x_next.  H, C, h_out, c_out of guide k are [streams][N[k]].
constexpr int MAX_GUIDES = 4;   // LSTM_HIP_MAX_GUIDES
struct GuideLogitsArgs {
    const float *Why[MAX_GUIDES], *by[MAX_GUIDES];
    const float *H[MAX_GUIDES], *C[MAX_GUIDES]; // state after t inputs
    float *h_out[MAX_GUIDES], *c_out[MAX_GUIDES]; // the state after each stream's last input (null: not kept)
    int N[MAX_GUIDES];          // internal widths, each % 16 == 0
    float w[MAX_GUIDES];        // (float)weight
    float *gsum;                // [streams][256]
    int nguides, streams;
    const uint64_t *off;        // streams + 1 offsets: the generator's prompts (null: none) or the scorer's texts
    int scorer;                 // 0: the generator's streams (off, end, count as GenHeadArgs), 1: the scorer's (off, first)
    int32_t *end;               // generator: GenHeadArgs::end, only read (always set: a guided draw is a processed one)
    int count;                  // generator: GenHeadArgs::count
    int first;                  // scorer: ScoreHeadArgs::first
    // the mixed coder (lstm_hip_encode_mixed / lstm_hip_decode_mixed): off is the coder's text_off, a
    // stream is active at step t iff t < its length, no state is copied out and gsum is not written; all 0 / null otherwise
    int coder;                  // 1: the coder's streams
    float *zk;                  // coder: [streams][nguides][256] every guide's own, unweighted logits of this step
};

// ---- beam search (lstm_hip_beam_search): per step beam_head on the state after t inputs, then
// fwd_step over all streams * W columns with x_next as inputs, reading the REORDERED state beam_head wrote.  Column
// c = s * W + r is slot r of stream s; per-slot arrays are [streams * W], the tables [count][streams * W].
struct BeamHeadArgs {
    const float *Why, *by;
    const float *H, *C;         // state after t inputs, [streams * W][N]
    float *Hr, *Cr;             // the same columns in the order of the new slots (never the buffers H, C)
    const uint8_t *prompts;     // concatenated prompts (null: none)
    const uint64_t *off;        // streams + 1 prompt offsets (null: no prompts)
    int32_t *x_next;            // the next input of every column (-1: none)
    double *cost;               // per slot: summed bits (slot 0 starts at 0, the others at +inf)
    int32_t *len, *fin;         // per slot: selected bytes so far; 1 once the stop byte was selected
    uint8_t *trace_parent, *trace_byte; // per selection and slot: the slot it extends, the byte (0 for a finished parent)
    int N, streams, W, count;
    int stop_byte;              // -1: none
    // byte automaton (lstm_hip_beam_search_constrained): read only by the CONSTRAIN instantiation,
    // which beam_head takes when `ctab` is set; all null / 0 in the unconstrained call
    const uint16_t *ctab;       // [states][256] the state after byte b in state q, 0xFFFF: b is forbidden there
    int32_t *cstate;            // per slot: its state, read at the start of a selection and rewritten in place at its end
    const uint8_t *accept;      // [states] nonzero: a hypothesis may end there (null: everywhere, and no deadline)
    const uint32_t *frows;      // [count][fwords] bit q of row R: an accepted end can be reached from q with R more bytes
    int fwords;                 // words of one row: (states + 31) / 32
};

// ---- model-driven range coder (lstm_hip_encode / lstm_hip_decode): per step code_head on the state
// after t inputs (byte t of every stream with more than t bytes is coded), then fwd_step over all streams with x_next.
// Stream s owns text[text_off[s] .. text_off[s+1]) and code[code_base[s] .. code_base[s+1]): the encoder never writes past
// the end of its range, the decoder reads 0 there.
constexpr uint32_t CODER_TOTAL_BITS = 16;   // totals <= 2^16 (the carryless coder's BOT)
constexpr uint32_t CODER_SCALE = 65024;     // q_m = 1 + (uint32)(p_m * 65024.0f): sum <= 256 + 65025 < 2^16
constexpr uint32_t CODE_ERR_TOTAL = 1u;     // a frequency total above 2^16 (the quantisation bound broken)
constexpr uint32_t CODE_ERR_BOUND = 2u;     // a code would pass its stream's range (lstm_hip_code_bound broken)
struct CoderState {                         // per stream, in device memory between steps
    uint32_t low, range, code, pad;
    uint64_t pos;                           // code bytes written (encoder) / read (decoder) so far
};
struct CodeHeadArgs {
    const float *Why, *by;
    const float *H;             // state after t inputs, [streams][N]
    const uint64_t *text_off;   // streams + 1
    uint8_t *text;              // encoder: read; decoder: written
    uint8_t *code;              // encoder: written; decoder: read
    const uint64_t *code_base;  // streams + 1: each stream's code range
    uint64_t *code_len;         // encoder: each stream's code length, written after its flush
    CoderState *state;          // [streams]
    double *bits;               // encoder: sum of -log2(freq / total) per stream, accumulated (null: not kept)
    uint32_t *trace;            // encoder: (cum, freq, total) per coded byte, in text order (null: not kept)
    int32_t *x_next;            // the next input of every stream (-1: none)
    uint32_t *err;              // OR of CODE_ERR_*
    int N, streams, decode;
    // the mixed coder (lstm_hip_encode_mixed / lstm_hip_decode_mixed): read only by the MIX
    // instantiation, which code_head_mixed launches; all null / 0 in the unmixed call
    const float *zk;            // [streams][nguides][256] the guides' logits of this step, written by k_guide_logits
    float *v;                   // [streams][1 + nguides] each stream's weights: the call's at the start, rewritten after every byte
    float *w_trace;             // encoder: [total][1 + nguides] the weights each byte was coded under, in text order (null: not kept)
    int nguides;                // 1 .. MAX_GUIDES
    float rate;                 // (float)rate: 0 leaves v alone
};

// ---- per-byte scores (lstm_hip_score): per step score_head on the state after t inputs (byte t of
// every stream with more than t bytes is scored, byte 0 only when `first`), then fwd_step over all streams with x_next.
// Per-position arrays are indexed like text (entry off[s] + j for byte j of stream s) and zeroed by the caller: the entries of
// unscored bytes are never written.  A null output is not computed; rank, top_byte or top_bits select the DETAIL
// instantiation, ctab the CONSTRAIN one.
struct ScoreHeadArgs {
    const float *Why, *by;
    const float *H, *C;         // state after t inputs, [streams][N]
    const uint8_t *text;        // concatenated texts
    const uint64_t *off;        // streams + 1 text offsets
    float *surprisal, *entropy; // [total]
    uint8_t *rank;              // [total]
    uint8_t *top_byte;          // [total][top_n]
    float *top_bits;            // [total][top_n]
    double *bits;               // [streams] sum of the stream's surprisals, accumulated in text order
    int32_t *x_next;            // the next input of every stream (-1: none)
    float *h_out, *c_out;       // the state after each stream's last byte (null: not kept)
    const uint16_t *ctab;       // [states][256] the byte automaton (GenHeadArgs::ctab), or null
    const uint16_t *qpos;       // [total] the automaton state each byte stands in (walked by the host); with ctab
    int N, streams, first, top_n;
    // guides (lstm_hip_score_guided), as GenHeadArgs::gsum / wmain: a scored byte's logit becomes
    // wmain * z + gsum ahead of the constraint mask
    const float *gsum;          // [streams][256], or null
    float wmain;
};

} // namespace lstmk
