// generate_main.cc -- use a trained model: score files and generate text from a checkpoint, through lstm_hip_generate
// (include/lstm_hip.h).  The reference's test() and sample() (OV/lstm_eigen_class_CUDA/lstm.cc:578-720, R/lstm.cc:293-356)
// over many streams at once.  No HIP, no torch here.
//
//   lstm_generate --load PREFIX [--score FILE ...] [--score-bytes FILE [--top N]] [--count C --streams K --prime TEXT|--prime-file F
//                 --temperature T --top-k K --top-p P --stop-byte B --seed S --utf8 --allow SPEC --ban SPEC --regex PATTERN
//                 --logit-bias BIAS --min-p P --no-repeat-ngram N
//                 [--guide PREFIX --guide-weight B]... [--main-weight A] | --guidance G [--negative-prime TEXT]
//                 | --beams W --nbest K --length-alpha A [--constrain-search --utf8 --allow SPEC --ban SPEC --regex PATTERN]]
//                 [--score-streams K [--score-warmup W]] [--fast-math] [--stable-softmax] [--device D]
//   lstm_generate --load PREFIX --embed FILE [--embed-delim B] [--pool last|mean|max|concat] [--embed-cell] [--embed-streams K]
//                 --embed-out OUT
//
// --load reads the five-file text checkpoint PREFIX_{W,U,Why,b,by}.txt (checkpoint.h); N is the rows of W / 4.
// --score runs every FILE as one stream from h = c = 0 and prints "FILE: X.XXXXX bits/char (n bytes)" per file (bits over
// the n - 1 predicted bytes, as lstm_hip_eval_bits) and a total weighted by those bytes.
// With --score-streams K (1..4096) every FILE is cut into K streams and all files are scored in one lstm_hip_eval_texts call, on
// the training window's forward path (eval_split.h): each piece after a file's first starts from a zero state --score-warmup W
// bytes (default 0) before its first scored byte; every byte but a file's first is still scored once, and the lines are the same.
// --score-bytes FILE prints one tab-separated row per byte of FILE (lstm_hip_score): its offset, the byte in hex, its surprisal
// in bits, the entropy of the distribution it was scored under, its rank (0: the model's first guess), then with --top N
// (1..8) the N most likely bytes at that place, each as hex byte and bits; after the rows the --score line of FILE.  The first
// byte is an input only, as for --score, and its row holds zeros.  With --utf8 / --allow / --ban every byte is scored under
// that table (forbidden bytes have no mass; a FILE the table rejects is refused) and the first byte is scored too, from
// the zero state, so the closing line then divides by all n bytes.  It goes with neither --score nor --count.
// --count prints K samples of C bytes, each continuing from the prompt (--prime / --prime-file, default none) from a zero
// state; the draws come from SeededRng(S) (rng.h), byte i of stream s taking draw i*K + s, so a seed gives the same text.
// --temperature 0 is greedy decoding and takes no draws.  --top-k K (1..255) draws among the K most likely bytes, --top-p P
// (0 < P < 1) among the smallest most-likely-first set of mass P, and with --stop-byte B (decimal, 0..255; 10 is a newline)
// a sample ends with its first drawn byte B: it is printed up to and including that byte (lstm_hip_generate_ex).
// --utf8 draws well-formed UTF-8 only (lstm_hip_generate_constrained under the table of lstm_hip_dfa_utf8; the prompt must be
// well-formed too) and prints a sample without an incomplete final character.  --allow SPEC draws only the listed bytes, --ban
// SPEC never the listed ones; SPEC is comma-separated bytes and ranges, decimal or 0x hex (0x20-0x7e,10).  With --utf8 they
// restrict its table (lstm_hip_dfa_restrict: a lead byte goes with its last continuation byte); without it the table has one
// state.  None of the three goes with --score, and with --beams they need --constrain-search (below).
// --beams W (1..32) searches instead of drawing (lstm_hip_beam_search): per stream the W most likely continuations of C bytes
// the beam search finds, of which the --nbest K (default 1) best are printed under "== sample s hypothesis k: X bits ==",
// ranked by their bits, or with --length-alpha A > 0 by bits / length^A.  It takes --prime, --count, --streams and
// --stop-byte (a hypothesis ends with its first selected byte B); it draws nothing, so the sampling options are refused.
// --beams 1 prints the text of --temperature 0.  With --constrain-search it goes with --utf8 / --allow / --ban: the search is
// over the continuations that table accepts (lstm_hip_beam_search_constrained).  With --utf8 the only accepting state is the
// character boundary, so every printed hypothesis is whole characters; with --allow / --ban alone there are no accepting
// states.  A stream whose table allows fewer than W continuations has fewer hypotheses: those that do not exist are not
// printed, and --nbest counts the ones that do.  Without --constrain-search the three are refused with --beams, as they were
// before the search took a constraint: they are options of drawing, and a script that relied on the refusal still gets it.
// --regex PATTERN draws whole matches of PATTERN only (lstm_hip_dfa_regex, lstm_hip_generate_accepting): a byte regular
// expression with the meaning Python's re.fullmatch gives a bytes pattern, in the subset include/lstm_hip.h lists (a
// quantifier binds the last byte: group a multi-byte character before repeating it).  With --stop-byte B a sample is a match
// of at most C - 1 bytes followed by B, and B must not occur in a match; WITHOUT --stop-byte a sample is a match of EXACTLY C
// bytes; a pattern that has none of that length is refused, and so is one with a match that nothing can follow (its table
// would hold a state without an allowed byte, which the calls refuse): such patterns take a stop byte.  The prompt is walked through the pattern first, so it must
// begin a match.  With --utf8 the matches are also well-formed UTF-8 (lstm_hip_dfa_intersect with the UTF-8 table, whole
// characters only); --allow / --ban then restrict the resulting table (lstm_hip_dfa_restrict).  With --beams
// --constrain-search the same table and accepting states go to the search.  A pattern the compiler refuses ends the program
// with the library's message, which names the offending byte of the pattern.
// --logit-bias BIAS, --min-p P and --no-repeat-ngram N are the logit processors of lstm_hip_generate_processed, applied to drawn
// bytes only, under whatever table the options above made: BIAS is comma-separated SPEC:VALUE items in the range syntax of
// --allow (0x41-0x5a:-2.5,10:+1) whose VALUE is added to the logits of those bytes (greedy decoding sees it); P (0 < P <= 1)
// cuts the bytes less than P times as likely as the most likely one; N (1..64) never draws a byte that would complete an N-byte
// sequence the sample, prompt included, already holds -- it ends the loops of --temperature 0 -- and gives way where the table
// would otherwise have no byte left.  The scan behind N is linear in the sample's length at every draw.  All three are options of
// drawing and are refused with --beams: beam search, the scorer and the coders take no processors.
// --guide PREFIX --guide-weight B loads a second checkpoint, of any width, as a guide (lstm_hip_generate_guided /
// lstm_hip_score_guided): it is fed the bytes the loaded model is fed, from a zero state of its own, and every drawn byte's
// logits become A * z + the sum of B * the guide's logits, ahead of the processors above; A is --main-weight (default 1).  The
// pair is repeatable up to four times, each --guide with the --guide-weight that follows it.  1.5 and -0.5 with a smaller model
// is contrastive decoding; weights that sum to 1 are the geometric mean of an ensemble.  With --score F or --score-bytes F
// (and no --count) the files are scored under the mix instead; it does not go with --score-streams.
// --guidance G --negative-prime TEXT uses the loaded model as its own guide, with the weights (1 + G, -G): the guide is primed
// with TEXT (empty by default) instead of --prime.  Both primings are calls that draw nothing and hand their end state over, and
// the drawing call then gets no prompt (a table's state and the n-gram rule's history are handed over with it).  It goes with
// --count only and not with --guide.  --beams refuses all of these: beam search takes no guides.
// --embed FILE writes what the model computed about every record of FILE (lstm_hip_embed_texts): FILE is cut after every
// delimiter byte (--embed-delim B, 0..255, default 10; the delimiter stays the last byte of its record and a last record may
// lack it, as lstm --records cuts), all records are embedded in one call from h = c = 0, --embed-streams K of them side by side
// (1..4096, default 64), and OUT gets one tab-separated row of %.9g floats per record: the hidden state pooled as --pool says
// -- last (the default: the state after the record's last byte), mean or max over all its positions, or concat: last, max,
// mean, in that order -- and with --embed-cell the same of the cell state behind it.  It goes with neither --count nor --score*.
// --stable-softmax scores and draws at temperature 1 with the
// max-shifted softmax (LSTM_HIP_STABLE_SOFTMAX), for checkpoints whose logits pass expf's range.
#include "../../include/lstm_hip.h"
#include "checkpoint.h"
#include "eval_split.h"
#include "rng.h"

#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <string>
#include <vector>

namespace {

const char *const kUsage =
    "usage: lstm_generate --load PREFIX [--score FILE ...] [--score-bytes FILE [--top N]]\n"
    "                     [--count C --streams K --prime TEXT|--prime-file F\n"
    "                     --temperature T --top-k K --top-p P --stop-byte B --seed S\n"
    "                     --utf8 --allow SPEC --ban SPEC --regex PATTERN\n"
    "                     --logit-bias BIAS --min-p P --no-repeat-ngram N\n"
    "                     [--guide PREFIX --guide-weight B]... [--main-weight A] | --guidance G [--negative-prime TEXT]\n"
    "                     | --beams W --nbest K --length-alpha A\n"
    "                       [--constrain-search --utf8 --allow SPEC --ban SPEC --regex PATTERN]]\n"
    "                     [--score-streams K [--score-warmup W]] [--fast-math] [--stable-softmax] [--device D]\n"
    "       lstm_generate --load PREFIX --embed FILE [--embed-delim B] [--pool last|mean|max|concat] [--embed-cell]\n"
    "                     [--embed-streams K] --embed-out OUT\n"
    "  --embed FILE   cut FILE into records after every delimiter byte (--embed-delim B, default 10) and write one\n"
    "                 tab-separated row per record to --embed-out OUT: the hidden state pooled as --pool says (last, mean,\n"
    "                 max, or concat = last, max, mean), with --embed-cell the cell state too; --embed-streams K records\n"
    "                 side by side (1..4096, default 64)\n"
    "  --score-streams K   with --score: cut every FILE into K streams (1..4096) and score all files in one call on the\n"
    "                 trainer's forward path; --score-warmup W feeds W bytes before each later piece's first scored byte\n"
    "  --score-bytes FILE  one row per byte: offset, byte, surprisal, entropy, rank; then the --score line of FILE\n"
    "  --top N        with --score-bytes: add the N most likely bytes of every place (1..8) with their bits\n"
    "  --top-k K      draw among the K most likely bytes (1..255; 0 or 256: all)\n"
    "  --top-p P      draw among the smallest most-likely-first set of bytes whose mass reaches P (0 < P <= 1)\n"
    "  --stop-byte B  end a sample with its first drawn byte B (decimal, 0..255) and print it up to that byte\n"
    "  --utf8         draw well-formed UTF-8 only; a sample is printed without an incomplete final character\n"
    "                 (with --beams --constrain-search: search whole characters only)\n"
    "  --allow SPEC   draw only these bytes: comma-separated bytes and ranges, decimal or 0x hex (0x20-0x7e,10)\n"
    "  --ban SPEC     never draw these bytes (same SPEC); with --utf8 both restrict the UTF-8 table\n"
    "  --regex PATTERN  draw whole matches of this byte regular expression only (re.fullmatch on bytes; a quantifier\n"
    "                 binds the last byte).  With --stop-byte B: a match, then B.  Without it: a match of exactly --count\n"
    "                 bytes.  --utf8 intersects with well-formed UTF-8; --allow / --ban restrict the result\n"
    "  --logit-bias BIAS  add VALUE to the logits of the listed bytes before every draw: comma-separated SPEC:VALUE items\n"
    "                 (0x41-0x5a:-2.5,10:+1); greedy decoding sees it too\n"
    "  --min-p P      draw among the bytes at least P times as likely as the most likely one (0 < P <= 1; 0: off)\n"
    "  --no-repeat-ngram N  never draw a byte that would complete an N-byte sequence the sample (prompt included) already\n"
    "                 holds (1..64; 0: off); a table (--utf8, --allow, --ban, --regex) wins where the two leave no byte\n"
    "  --guide PREFIX  load a second checkpoint (any width) as a guide, fed the same bytes: the logits of every drawn byte\n"
    "                 become A * z + the sum of B * the guide's; repeatable up to four times, each with its --guide-weight.\n"
    "                 With --score / --score-bytes (and no --count) the files are scored under the mix\n"
    "  --guide-weight B  the weight of the --guide before it (finite; negative: contrast against that model)\n"
    "  --main-weight A  the weight of the loaded model's own logits (finite, default 1); needs --guide\n"
    "  --guidance G   the loaded model as its own guide with the weights (1 + G, -G), primed with --negative-prime\n"
    "  --negative-prime TEXT  what the guide of --guidance reads in place of --prime (default: nothing)\n"
    "  --beams W      beam search with W hypotheses per stream (1..32) instead of drawing; W x --streams <= 4096;\n"
    "  --constrain-search  with --beams: let --utf8 / --allow / --ban constrain the search to the continuations they\n"
    "                 accept (without it they are refused with --beams); hypotheses that do not exist are not printed\n"
    "  --nbest K      print the K best hypotheses of every stream (1..W, default 1) with their bits\n"
    "  --length-alpha A  rank hypotheses by bits / length^A (default 0: by bits)\n";

[[noreturn]] void usage(const std::string &m) {
    fprintf(stderr, "lstm_generate: %s\n%s", m.c_str(), kUsage);
    exit(2);
}
[[noreturn]] void die(const std::string &m) {
    fprintf(stderr, "lstm_generate: %s\n", m.c_str());
    exit(1);
}
#define CK(call)                                                                \
    do {                                                                        \
        int rc_ = (call);                                                       \
        if (rc_ != 0) die(std::string(#call) + ": " + lstm_hip_last_error());   \
    } while (0)

bool read_file(const std::string &path, std::vector<uint8_t> &v) {
    FILE *fp = fopen(path.c_str(), "rb");
    if (!fp) return false;
    char buf[1 << 16];
    while (size_t len = fread(buf, 1, sizeof(buf), fp)) v.insert(v.end(), buf, buf + len);
    fclose(fp);
    return true;
}

// whole-string numbers only: "12x", "" and out-of-range values are usage errors
long parse_int(const std::string &opt, const std::string &v, long lo, long hi) {
    char *end = nullptr;
    errno = 0;
    const long x = strtol(v.c_str(), &end, 10);
    if (v.empty() || *end != '\0' || errno != 0 || x < lo || x > hi)
        usage(opt + " needs an integer in [" + std::to_string(lo) + ", " + std::to_string(hi) + "], got '" + v + "'");
    return x;
}
double parse_double(const std::string &opt, const std::string &v) {
    char *end = nullptr;
    const double x = strtod(v.c_str(), &end);
    if (v.empty() || *end != '\0' || !std::isfinite(x) || x < 0.0) usage(opt + " needs a finite number >= 0, got '" + v + "'");
    return x;
}

// SPEC: comma-separated bytes and ranges lo-hi, decimal or 0x hex; sets flag[b] = 1 for every listed byte
void parse_spec(const std::string &opt, const std::string &v, uint8_t flag[256]) {
    auto bad = [&]() { usage(opt + " needs bytes and ranges such as 0x20-0x7e,10 (each in [0, 255]), got '" + v + "'"); };
    auto number = [&](const std::string &t) -> long {
        const bool hex = t.size() > 2 && t[0] == '0' && (t[1] == 'x' || t[1] == 'X');
        const std::string digits = hex ? t.substr(2) : t;
        if (digits.empty() || digits.size() > 3 ||
            digits.find_first_not_of(hex ? "0123456789abcdefABCDEF" : "0123456789") != std::string::npos)
            bad();
        const long x = strtol(digits.c_str(), nullptr, hex ? 16 : 10);
        if (x > 255) bad();
        return x;
    };
    if (v.empty()) bad();
    for (size_t at = 0; at <= v.size();) {
        const size_t comma = std::min(v.find(',', at), v.size());
        const std::string item = v.substr(at, comma - at);
        const size_t dash = item.find('-');
        const long lo = number(item.substr(0, dash)), hi = dash == std::string::npos ? lo : number(item.substr(dash + 1));
        if (hi < lo) bad();
        for (long b = lo; b <= hi; b++) flag[b] = 1;
        at = comma + 1;
    }
}

// BIAS: comma-separated SPEC:VALUE items, SPEC one byte or range as above, VALUE a finite number with an optional sign
// (0x41-0x5a:-2.5,10:+1); a byte listed twice takes the later value
void parse_bias(const std::string &opt, const std::string &v, float bias[256]) {
    auto bad = [&]() { usage(opt + " needs items byte-or-range:value such as 0x41-0x5a:-2.5,10:+1 (finite values), got '" + v + "'"); };
    if (v.empty()) bad();
    for (size_t at = 0; at <= v.size();) {
        const size_t comma = std::min(v.find(',', at), v.size());
        const std::string item = v.substr(at, comma - at);
        const size_t colon = item.find(':');
        if (colon == std::string::npos || colon == 0 || colon + 1 == item.size() || item.find(',') != std::string::npos) bad();
        uint8_t flag[256] = {};
        parse_spec(opt, item.substr(0, colon), flag);
        const std::string num = item.substr(colon + 1);
        char *end = nullptr;
        const double x = strtod(num.c_str(), &end);
        if (*end != '\0' || !std::isfinite(x) || !std::isfinite((float)x)) bad();
        for (int b = 0; b < 256; b++)
            if (flag[b]) bias[b] = (float)x;
        at = comma + 1;
    }
}

// a finite number of either sign: "", "1x", inf and nan are usage errors
double parse_finite(const std::string &opt, const std::string &v) {
    char *end = nullptr;
    const double x = strtod(v.c_str(), &end);
    if (v.empty() || *end != '\0' || !std::isfinite(x)) usage(opt + " needs a finite number, got '" + v + "'");
    return x;
}

struct Options {
    std::vector<std::string> guides;      // --guide PREFIX, up to LSTM_HIP_MAX_GUIDES of them
    std::vector<double> guide_weights;    // --guide-weight B, one per --guide
    double main_weight = 1.0;             // --main-weight A
    bool has_main_weight = false;
    double guidance = 0.0;                // --guidance G
    bool has_guidance = false, has_negative_prime = false;
    std::string negative_prime;           // --negative-prime TEXT
    bool has_bias = false;   // --logit-bias
    float bias[256] = {};
    double min_p = 0.0;      // --min-p
    long no_repeat = 0;      // --no-repeat-ngram
    std::string load, prime, prime_file;
    bool has_prime = false;
    std::vector<std::string> sampling_opts; // options that only mean something with --count
    std::vector<std::string> score;
    std::string score_bytes; // --score-bytes FILE
    long score_streams = 0, score_warmup = -1; // --score-streams K (0: lstm_hip_generate's prompt bits), --score-warmup W
    long top = -1;           // --top N (-1: not given)
    std::string embed, embed_out, pool; // --embed FILE, --embed-out OUT, --pool (empty: last)
    long embed_delim = 10, embed_streams = 64;
    bool embed_cell = false;
    std::string embed_opt;   // the last option given that needs --embed
    long count = -1, streams = 1, device = 0;
    double temperature = 1.0, top_p = 1.0;
    long top_k = 0, stop_byte = -1;
    long beams = 0, nbest = 1; // beams 0: draw
    double length_alpha = 0.0;
    std::vector<std::string> draw_opts, beam_opts; // options that only mean something without / with --beams
    std::vector<std::string> constraint_opts;      // --utf8, --allow, --ban as given
    uint32_t seed = 1;
    unsigned flags = 0;
    bool utf8 = false, has_allow = false, has_ban = false, has_regex = false;
    std::string regex;           // --regex PATTERN
    std::vector<uint8_t> accept; // with --regex: the accepting states of `table`
    bool constrain_search = false; // --constrain-search: with --beams the constraint options constrain the search
    uint8_t allow[256] = {}, ban[256] = {};
    std::vector<uint16_t> table; // the constraint of --utf8 / --allow / --ban (empty: none), `states` rows of 256
    int32_t states = 0;
};

Options parse(int argc, char **argv) {
    Options o;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto val = [&]() -> std::string {
            if (i + 1 >= argc) usage("missing value for " + a);
            return argv[++i];
        };
        if (a == "--load") o.load = val();
        else if (a == "--score") {
            o.score.push_back(val());
            while (i + 1 < argc && std::string(argv[i + 1]).rfind("--", 0) != 0) o.score.push_back(argv[++i]);
        } else if (a == "--score-bytes") o.score_bytes = val();
        else if (a == "--score-streams") o.score_streams = parse_int(a, val(), 1, 4096);
        else if (a == "--score-warmup") o.score_warmup = parse_int(a, val(), 0, 1L << 30);
        else if (a == "--top") o.top = parse_int(a, val(), 1, 8);
        else if (a == "--embed") o.embed = val();
        else if (a == "--embed-out") o.embed_out = val(), o.embed_opt = a;
        else if (a == "--embed-delim") o.embed_delim = parse_int(a, val(), 0, 255), o.embed_opt = a;
        else if (a == "--embed-streams") o.embed_streams = parse_int(a, val(), 1, 4096), o.embed_opt = a;
        else if (a == "--embed-cell") o.embed_cell = true, o.embed_opt = a;
        else if (a == "--pool") {
            o.pool = val(), o.embed_opt = a;
            if (o.pool != "last" && o.pool != "mean" && o.pool != "max" && o.pool != "concat")
                usage(a + " needs one of last, mean, max, concat, got '" + o.pool + "'");
        }
        else if (a == "--count") o.count = parse_int(a, val(), 0, 1L << 30);
        else if (a == "--streams") {
            o.streams = parse_int(a, val(), 1, 4096);
            o.sampling_opts.push_back(a);
        }
        else if (a == "--prime") {
            o.prime = val();
            o.has_prime = true;
            o.sampling_opts.push_back(a);
        } else if (a == "--prime-file") {
            o.prime_file = val();
            o.sampling_opts.push_back(a);
        } else if (a == "--temperature") {
            o.temperature = parse_double(a, val());
            o.sampling_opts.push_back(a);
            o.draw_opts.push_back(a);
        } else if (a == "--top-k") {
            o.top_k = parse_int(a, val(), 0, 256);
            o.sampling_opts.push_back(a);
            o.draw_opts.push_back(a);
        } else if (a == "--top-p") {
            o.top_p = parse_double(a, val());
            if (!(o.top_p > 0.0 && o.top_p <= 1.0)) usage(a + " needs a number in (0, 1]");
            o.sampling_opts.push_back(a);
            o.draw_opts.push_back(a);
        } else if (a == "--stop-byte") {
            o.stop_byte = parse_int(a, val(), 0, 255);
            o.sampling_opts.push_back(a);
        } else if (a == "--logit-bias") {
            parse_bias(a, val(), o.bias);
            o.has_bias = true;
            o.sampling_opts.push_back(a);
            o.draw_opts.push_back(a);
        } else if (a == "--min-p") {
            o.min_p = parse_double(a, val());
            if (!(o.min_p <= 1.0)) usage(a + " needs a number in [0, 1]");
            o.sampling_opts.push_back(a);
            o.draw_opts.push_back(a);
        } else if (a == "--no-repeat-ngram") {
            o.no_repeat = parse_int(a, val(), 0, 64);
            o.sampling_opts.push_back(a);
            o.draw_opts.push_back(a);
        } else if (a == "--guide") {
            if (o.guides.size() != o.guide_weights.size()) usage("--guide " + o.guides.back() + " needs a --guide-weight before the next --guide");
            if (o.guides.size() == LSTM_HIP_MAX_GUIDES) usage("--guide may be given at most " + std::to_string(LSTM_HIP_MAX_GUIDES) + " times");
            o.guides.push_back(val());
            o.draw_opts.push_back(a);
        } else if (a == "--guide-weight") {
            if (o.guides.size() != o.guide_weights.size() + 1) usage("--guide-weight follows the --guide it belongs to");
            o.guide_weights.push_back(parse_finite(a, val()));
        } else if (a == "--main-weight") {
            o.main_weight = parse_finite(a, val());
            o.has_main_weight = true;
        } else if (a == "--guidance") {
            o.guidance = parse_finite(a, val());
            o.has_guidance = true;
            o.sampling_opts.push_back(a);
            o.draw_opts.push_back(a);
        } else if (a == "--negative-prime") {
            o.negative_prime = val();
            o.has_negative_prime = true;
        } else if (a == "--seed") {
            o.seed = (uint32_t)parse_int(a, val(), 0, 0xFFFFFFFFL);
            o.sampling_opts.push_back(a);
            o.draw_opts.push_back(a);
        } else if (a == "--utf8" || a == "--allow" || a == "--ban") {
            if (a == "--utf8") o.utf8 = true;
            else if (a == "--allow") {
                parse_spec(a, val(), o.allow);
                o.has_allow = true;
            } else {
                parse_spec(a, val(), o.ban);
                o.has_ban = true;
            }
            o.sampling_opts.push_back(a);
            o.constraint_opts.push_back(a);
        } else if (a == "--regex") {
            o.regex = val();
            o.has_regex = true;
            o.sampling_opts.push_back(a);
            o.constraint_opts.push_back(a);
        } else if (a == "--beams") {
            o.beams = parse_int(a, val(), 1, 32);
            o.sampling_opts.push_back(a);
        } else if (a == "--constrain-search") {
            o.constrain_search = true;
            o.sampling_opts.push_back(a);
            o.beam_opts.push_back(a);
        } else if (a == "--nbest") {
            o.nbest = parse_int(a, val(), 1, 32);
            o.sampling_opts.push_back(a);
            o.beam_opts.push_back(a);
        } else if (a == "--length-alpha") {
            o.length_alpha = parse_double(a, val());
            o.sampling_opts.push_back(a);
            o.beam_opts.push_back(a);
        }
        else if (a == "--device") o.device = parse_int(a, val(), 0, 1 << 20);
        else if (a == "--fast-math") o.flags |= LSTM_HIP_FAST_MATH;
        else if (a == "--stable-softmax") o.flags |= LSTM_HIP_STABLE_SOFTMAX;
        else if (a == "-h" || a == "--help") {
            printf("%s", kUsage);
            exit(0);
        } else usage("unknown argument " + a);
    }
    if (o.load.empty()) usage("--load PREFIX is required");
    if (!o.embed_opt.empty() && o.embed.empty()) usage(o.embed_opt + " needs --embed");
    if (!o.embed.empty()) { // a mode of its own
        if (o.count >= 0 || !o.score.empty() || !o.score_bytes.empty()) usage("--embed goes with neither --count nor --score / --score-bytes");
        if (o.embed_out.empty()) usage("--embed needs --embed-out OUT");
    }
    if (o.score.empty() && o.count < 0 && o.score_bytes.empty() && o.embed.empty())
        usage("nothing to do: give --score, --score-bytes, --embed and/or --count");
    if (o.guides.size() != o.guide_weights.size()) usage("--guide " + o.guides.back() + " needs a --guide-weight");
    if (o.has_main_weight && o.guides.empty()) usage("--main-weight needs --guide");
    if (o.has_negative_prime && !o.has_guidance) usage("--negative-prime needs --guidance");
    if (o.has_guidance && !o.guides.empty()) usage("--guidance does not go with --guide: it makes the loaded model its own guide");
    if (o.has_guidance && !o.score.empty()) usage("--guidance guides the drawing: it does not go with --score");
    if (!o.guides.empty()) {
        if (!o.embed.empty()) usage("--guide does not go with --embed");
        if (o.score_streams > 0) usage("--guide does not go with --score-streams: that path takes no guides");
        if (o.count >= 0 && !o.score.empty()) usage("--guide with --count guides the drawing: score the files in a run of their own");
    }
    if (o.top >= 0 && o.score_bytes.empty()) usage("--top needs --score-bytes");
    if (o.score_streams > 0 && o.score.empty()) usage("--score-streams needs --score");
    if (o.score_warmup >= 0 && o.score_streams == 0) usage("--score-warmup needs --score-streams");
    if (o.score_streams > 0 && o.score.size() * (size_t)o.score_streams > (size_t)1 << 30) usage("--score-streams x files is too large");
    if (!o.score_bytes.empty()) { // a mode of its own; of the sampling options it takes the constraint's
        if (o.count >= 0 || !o.score.empty()) usage("--score-bytes goes with neither --count nor --score");
        for (const std::string &a : o.sampling_opts)
            if (std::find(o.constraint_opts.begin(), o.constraint_opts.end(), a) == o.constraint_opts.end()) usage(a + " needs --count");
        o.sampling_opts.clear();
    }
    if (o.has_prime && !o.prime_file.empty()) usage("--prime and --prime-file exclude each other");
    if (o.count < 0 && !o.sampling_opts.empty()) usage(o.sampling_opts[0] + " needs --count");
    if ((long long)std::max(o.count, 0L) * o.streams > (1LL << 31) - 1) usage("--count x --streams is too large");
    if (o.beams == 0 && !o.beam_opts.empty()) usage(o.beam_opts[0] + " needs --beams");
    if (o.beams > 0) {
        if (!o.draw_opts.empty()) usage(o.draw_opts[0] + " means nothing with --beams: a beam search draws nothing");
        if (!o.constraint_opts.empty() && !o.constrain_search)
            usage(o.constraint_opts[0] + " is an option of drawing: with --beams it needs --constrain-search");
        if (o.constrain_search && o.constraint_opts.empty()) usage("--constrain-search needs --utf8, --allow, --ban or --regex");
        if (o.nbest > o.beams) usage("--nbest cannot pass --beams");
        if (o.beams * o.streams > 4096) usage("--beams x --streams must be at most 4096");
        if ((long long)std::max(o.count, 0L) * o.streams * o.beams > (1LL << 31) - 1) usage("--count x --streams x --beams is too large");
    }
    if (!o.constraint_opts.empty()) {
        if (!o.score.empty()) usage(o.constraint_opts[0] + " does not go with --score: scoring ignores a constraint");
        o.states = o.utf8 ? lstm_hip_dfa_utf8(nullptr) : 1;
        o.table.assign((size_t)o.states * 256, 0); // one state: every byte leads back to it
        if (o.utf8) lstm_hip_dfa_utf8(o.table.data());
        if (o.has_regex) { // the pattern's table (followed by the stop byte, if any), then its product with the UTF-8 table
            const uint8_t *pat = reinterpret_cast<const uint8_t *>(o.regex.data());
            int32_t q = lstm_hip_dfa_regex(pat, o.regex.size(), (int32_t)o.stop_byte, nullptr, nullptr, 0, nullptr);
            if (q < 0) die(std::string("--regex: ") + lstm_hip_last_error());
            std::vector<uint16_t> rx((size_t)q * 256);
            std::vector<uint8_t> acc(q);
            if (lstm_hip_dfa_regex(pat, o.regex.size(), (int32_t)o.stop_byte, rx.data(), acc.data(), q, nullptr) != q)
                die(std::string("--regex: ") + lstm_hip_last_error());
            if (o.stop_byte < 0) // the calls refuse a table with a reachable row that allows nothing, and pruning it would drop matches
                for (int32_t s = 0; s < q; s++)
                    if (acc[s] && std::all_of(rx.begin() + (size_t)s * 256, rx.begin() + (size_t)(s + 1) * 256, [](uint16_t v) { return v == 0xFFFF; }))
                        die("--regex without --stop-byte: the pattern has a match that nothing can follow, so its table has a state "
                            "without an allowed byte; give --stop-byte B (a match, then B)");
            if (o.utf8) {
                std::vector<uint8_t> boundary(o.states, 0);
                boundary[0] = 1;
                const int32_t p = lstm_hip_dfa_intersect(rx.data(), q, acc.data(), o.table.data(), o.states, boundary.data(), nullptr, nullptr, 0);
                if (p < 0) die(std::string("--regex with --utf8: ") + lstm_hip_last_error());
                std::vector<uint16_t> both((size_t)p * 256);
                std::vector<uint8_t> acc2(p);
                if (lstm_hip_dfa_intersect(rx.data(), q, acc.data(), o.table.data(), o.states, boundary.data(), both.data(), acc2.data(), p) != p)
                    die(std::string("--regex with --utf8: ") + lstm_hip_last_error());
                rx.swap(both), acc.swap(acc2), q = p;
            }
            o.table.swap(rx), o.accept.swap(acc), o.states = q;
        }
        uint8_t allow[256];
        for (int b = 0; b < 256; b++) allow[b] = (!o.has_allow || o.allow[b]) && !o.ban[b];
        if (lstm_hip_dfa_restrict(o.table.data(), o.states, allow) != 0)
            usage(std::string("--allow / --ban leave nothing to draw: ") + lstm_hip_last_error());
    }
    return o;
}

} // namespace

int main(int argc, char **argv) {
    const Options o = parse(argc, argv);
    const int M = LSTM_HIP_VOCAB;
    std::string err;
    const int N = checkpoint::hidden_size(o.load, M, &err);
    if (N == 0) die(err);
    std::vector<float> P(lstm_hip_param_count(N, M));
    const int rc = checkpoint::load_params(o.load, P, N, M, &err);
    if (rc == 0) die("missing a file of " + o.load + "_{W,U,Why,b,by}.txt");
    if (rc < 0) die(err);
    std::vector<std::vector<uint8_t>> texts;
    for (const std::string &f : o.score) {
        texts.emplace_back();
        if (!read_file(f, texts.back())) die("cannot read " + f);
        if (texts.back().size() < 2) die(f + ": need at least 2 bytes to score");
    }
    std::vector<uint8_t> prime(o.prime.begin(), o.prime.end());
    if (!o.prime_file.empty() && !read_file(o.prime_file, prime)) die("cannot read " + o.prime_file);

    // every hidden size runs (LSTM_HIP_PAD_HIDDEN); S and B of the handle are not used by the generator
    lstm_hip_config cfg{N, M, 2, 1, (int32_t)o.device, o.flags | LSTM_HIP_PAD_HIDDEN};
    lstm_hip_t *h = nullptr;
    CK(lstm_hip_create(&cfg, &h));
    CK(lstm_hip_set_params(h, 0, P.data()));

    // the guides: a handle per --guide checkpoint, each of its own width; --guidance takes the loaded model itself
    std::vector<lstm_hip_t *> guide_handles;
    std::vector<lstm_hip_guide> guides;
    for (size_t k = 0; k < o.guides.size(); k++) {
        const int Ng = checkpoint::hidden_size(o.guides[k], M, &err);
        if (Ng == 0) die(err);
        std::vector<float> Pg(lstm_hip_param_count(Ng, M));
        const int rg = checkpoint::load_params(o.guides[k], Pg, Ng, M, &err);
        if (rg == 0) die("missing a file of " + o.guides[k] + "_{W,U,Why,b,by}.txt");
        if (rg < 0) die(err);
        lstm_hip_config gcfg{Ng, M, 2, 1, (int32_t)o.device, o.flags | LSTM_HIP_PAD_HIDDEN};
        lstm_hip_t *g = nullptr;
        CK(lstm_hip_create(&gcfg, &g));
        CK(lstm_hip_set_params(g, 0, Pg.data()));
        guide_handles.push_back(g);
        guides.push_back(lstm_hip_guide{g, o.guide_weights[k], nullptr, nullptr, nullptr, nullptr});
    }
    if (o.has_guidance) guides.push_back(lstm_hip_guide{h, -o.guidance, nullptr, nullptr, nullptr, nullptr});
    const lstm_hip_guidance gd{(uint32_t)sizeof(lstm_hip_guidance), o.has_guidance ? 1.0 + o.guidance : o.main_weight,
                               (int32_t)guides.size(), guides.data()};
    const bool guided = !guides.empty();

    if (!texts.empty() && guided) { // every file as one stream under the mix: lstm_hip_score_guided's bits (byte 0 an input only)
        double sum_bits = 0.0, sum_chars = 0.0;
        for (size_t f0 = 0; f0 < texts.size(); f0 += 4096) {
            const size_t k = std::min<size_t>(4096, texts.size() - f0);
            std::vector<uint64_t> off(k + 1, 0);
            std::vector<uint8_t> all;
            for (size_t s = 0; s < k; s++) {
                all.insert(all.end(), texts[f0 + s].begin(), texts[f0 + s].end());
                off[s + 1] = all.size();
            }
            std::vector<double> bits(k);
            const lstm_hip_scoring opt{(uint32_t)sizeof(lstm_hip_scoring), 0, 0, nullptr};
            lstm_hip_scores out{};
            out.size = (uint32_t)sizeof(lstm_hip_scores);
            out.bits = bits.data();
            CK(lstm_hip_score_guided(h, (int32_t)k, all.data(), off.data(), nullptr, nullptr, &opt, nullptr, &out, nullptr, nullptr, &gd));
            for (size_t s = 0; s < k; s++) {
                const size_t n = texts[f0 + s].size();
                printf("%s: %.5f bits/char (%zu bytes)\n", o.score[f0 + s].c_str(), bits[s] / (double)(n - 1), n);
                sum_bits += bits[s];
                sum_chars += (double)(n - 1);
            }
        }
        printf("total: %.5f bits/char (%.0f bytes scored in %zu files)\n", sum_bits / sum_chars, sum_chars, texts.size());
    } else
    if (!texts.empty()) { // one stream per file, in chunks of at most 4096 files
        double sum_bits = 0.0, sum_chars = 0.0;
        if (o.score_streams > 0) { // every file in K pieces, all of them in one call
            EvalSplit split;
            for (const std::vector<uint8_t> &t : texts) split.add(t.data(), t.size(), (size_t)o.score_streams, (size_t)std::max(o.score_warmup, 0L));
            std::vector<double> bits;
            CK(split.run(h, bits));
            for (size_t s = 0; s < texts.size(); s++) {
                const size_t n = texts[s].size();
                printf("%s: %.5f bits/char (%zu bytes)\n", o.score[s].c_str(), bits[s] / (double)(n - 1), n);
                sum_bits += bits[s];
                sum_chars += (double)(n - 1);
            }
        } else
        for (size_t f0 = 0; f0 < texts.size(); f0 += 4096) {
            const size_t k = std::min<size_t>(4096, texts.size() - f0);
            std::vector<uint64_t> off(k + 1, 0);
            std::vector<uint8_t> all;
            for (size_t s = 0; s < k; s++) {
                all.insert(all.end(), texts[f0 + s].begin(), texts[f0 + s].end());
                off[s + 1] = all.size();
            }
            std::vector<double> bits(k);
            CK(lstm_hip_generate(h, (int32_t)k, all.data(), off.data(), nullptr, nullptr, 1.0, nullptr, 0, nullptr, bits.data(),
                                 nullptr, nullptr));
            for (size_t s = 0; s < k; s++) {
                const size_t n = texts[f0 + s].size();
                printf("%s: %.5f bits/char (%zu bytes)\n", o.score[f0 + s].c_str(), bits[s] / (double)(n - 1), n);
                sum_bits += bits[s];
                sum_chars += (double)(n - 1);
            }
        }
        printf("total: %.5f bits/char (%.0f bytes scored in %zu files)\n", sum_bits / sum_chars, sum_chars, texts.size());
    }

    if (!o.score_bytes.empty()) { // one stream from h = c = 0
        std::vector<uint8_t> text;
        if (!read_file(o.score_bytes, text)) die("cannot read " + o.score_bytes);
        if (text.size() < 2) die(o.score_bytes + ": need at least 2 bytes to score");
        const size_t n = text.size(), top = o.top > 0 ? (size_t)o.top : 0;
        const bool constrained = !o.table.empty();
        const uint64_t off[2] = {0, n};
        std::vector<float> surprisal(n), entropy(n), top_bits(n * top);
        std::vector<uint8_t> rank(n), top_byte(n * top);
        double bits = 0.0;
        const lstm_hip_constraint con{(uint32_t)sizeof(lstm_hip_constraint), o.states, o.table.data()};
        const lstm_hip_scoring opt{(uint32_t)sizeof(lstm_hip_scoring), constrained ? 1 : 0, (int32_t)top, constrained ? &con : nullptr};
        const lstm_hip_scores out{(uint32_t)sizeof(lstm_hip_scores), surprisal.data(), entropy.data(), rank.data(),
                                  top ? top_byte.data() : nullptr, top ? top_bits.data() : nullptr, &bits, nullptr};
        CK(lstm_hip_score_guided(h, 1, text.data(), off, nullptr, nullptr, &opt, nullptr, &out, nullptr, nullptr, guided ? &gd : nullptr));
        for (size_t j = 0; j < n; j++) {
            printf("%zu\t%02x\t%.5f\t%.5f\t%d", j, (unsigned)text[j], surprisal[j], entropy[j], (int)rank[j]);
            for (size_t r = 0; r < top; r++) printf("\t%02x\t%.5f", (unsigned)top_byte[j * top + r], top_bits[j * top + r]);
            fputc('\n', stdout);
        }
        printf("%s: %.5f bits/char (%zu bytes)\n", o.score_bytes.c_str(), bits / (double)(constrained ? n : n - 1), n);
    }

    if (!o.embed.empty()) { // every record of the file, all in one call
        std::vector<uint8_t> text;
        if (!read_file(o.embed, text)) die("cannot read " + o.embed);
        std::vector<uint64_t> off(1, 0);
        for (size_t i = 0; i < text.size(); i++)
            if (text[i] == (uint8_t)o.embed_delim) off.push_back(i + 1);
        if (off.back() != text.size()) off.push_back(text.size()); // a last record may lack its delimiter
        const size_t K = off.size() - 1;
        if (K == 0) die(o.embed + ": no record to embed");
        if (K > (size_t)1 << 30) die(o.embed + ": too many records");
        const std::string pool = o.pool.empty() ? "last" : o.pool;
        const bool concat = pool == "concat";
        std::vector<float> block[2][3]; // [h, c][last, max, mean]: the order of concat
        lstm_hip_embedding out{};
        out.size = (uint32_t)sizeof(lstm_hip_embedding);
        float **slot[2][3] = {{&out.last_h, &out.max_h, &out.mean_h}, {&out.last_c, &out.max_c, &out.mean_c}};
        const char *const name[3] = {"last", "max", "mean"};
        for (int x = 0; x < (o.embed_cell ? 2 : 1); x++)
            for (int k = 0; k < 3; k++)
                if (concat || pool == name[k]) {
                    block[x][k].resize(K * (size_t)N);
                    *slot[x][k] = block[x][k].data();
                }
        const lstm_hip_eval_opt eopt{(uint32_t)sizeof(lstm_hip_eval_opt), (int32_t)std::min<size_t>((size_t)o.embed_streams, K)};
        CK(lstm_hip_embed_texts(h, (int32_t)K, text.data(), off.data(), nullptr, nullptr, nullptr, &eopt, nullptr, 0, &out, nullptr));
        FILE *fp = fopen(o.embed_out.c_str(), "w");
        if (!fp) die("cannot write " + o.embed_out);
        for (size_t s = 0; s < K; s++) {
            bool first = true;
            for (int x = 0; x < 2; x++)
                for (int k = 0; k < 3; k++)
                    for (size_t i = 0; i < (block[x][k].empty() ? 0 : (size_t)N); i++) {
                        fprintf(fp, first ? "%.9g" : "\t%.9g", (double)block[x][k][s * N + i]);
                        first = false;
                    }
            fputc('\n', fp);
        }
        if (fclose(fp) != 0) die("cannot write " + o.embed_out);
        fprintf(stderr, "lstm_generate: %zu records embedded (%s%s, %zu floats each)\n", K, pool.c_str(), o.embed_cell ? ", cell" : "",
                (size_t)N * (concat ? 3 : 1) * (o.embed_cell ? 2 : 1));
    }

    if (o.count >= 0 && o.beams > 0) {
        const int K = (int)o.streams, C = (int)o.count, W = (int)o.beams;
        std::vector<uint64_t> off(K + 1);
        std::vector<uint8_t> prompts;
        for (int s = 0; s < K; s++) {
            prompts.insert(prompts.end(), prime.begin(), prime.end());
            off[s + 1] = prompts.size();
        }
        std::vector<uint8_t> out((size_t)C * K * W + 1);
        std::vector<int32_t> out_len((size_t)K * W);
        std::vector<double> bits((size_t)K * W);
        const lstm_hip_beam opt{(uint32_t)sizeof(lstm_hip_beam), (int32_t)W, (int32_t)o.stop_byte};
        if (o.table.empty())
            CK(lstm_hip_beam_search(h, K, prompts.data(), off.data(), nullptr, nullptr, &opt, C, out.data(), out_len.data(),
                                    bits.data(), nullptr, nullptr));
        else { // --utf8: a hypothesis may end on a character boundary only (state 0 of the table); --regex: on a match
            const lstm_hip_constraint con{(uint32_t)sizeof(lstm_hip_constraint), o.states, o.table.data()};
            std::vector<uint8_t> accept(o.states, 0);
            accept[0] = 1;
            if (o.has_regex) accept = o.accept;
            const lstm_hip_beam_constraint bc{(uint32_t)sizeof(lstm_hip_beam_constraint), &con, o.utf8 || o.has_regex ? accept.data() : nullptr};
            CK(lstm_hip_beam_search_constrained(h, K, prompts.data(), off.data(), nullptr, nullptr, &opt, C, out.data(),
                                                out_len.data(), bits.data(), nullptr, nullptr, &bc, nullptr, nullptr));
        }
        for (int s = 0; s < K; s++) {
            std::vector<int> order;
            for (int r = 0; r < W; r++) // under a constraint, infinite bits and no bytes: no such hypothesis
                if (o.table.empty() || !(std::isinf(bits[s * W + r]) && out_len[s * W + r] == 0)) order.push_back(s * W + r);
            auto score = [&](int c) { return bits[c] / std::pow((double)std::max(out_len[c], 1), o.length_alpha); };
            if (o.length_alpha > 0.0) std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return score(x) < score(y); });
            for (int k = 0; k < (int)std::min<size_t>(o.nbest, order.size()); k++) {
                const int c = order[k];
                printf("== sample %d hypothesis %d: %.5f bits ==\n", s, k, bits[c]);
                fwrite(prime.data(), 1, prime.size(), stdout);
                fwrite(out.data() + (size_t)c * C, 1, (size_t)out_len[c], stdout);
                fputc('\n', stdout);
            }
        }
    } else if (o.count >= 0) {
        const int K = (int)o.streams, C = (int)o.count;
        std::vector<uint64_t> off(K + 1);
        std::vector<uint8_t> prompts;
        for (int s = 0; s < K; s++) {
            prompts.insert(prompts.end(), prime.begin(), prime.end());
            off[s + 1] = prompts.size();
        }
        std::vector<double> u;
        if (o.temperature > 0.0) {
            SeededRng rng(o.seed);
            u.resize((size_t)C * K);
            for (double &x : u) x = rng.uniform();
        }
        std::vector<uint8_t> out((size_t)C * K);
        const lstm_hip_sampling opt{(uint32_t)sizeof(lstm_hip_sampling), o.temperature, (int32_t)o.top_k, o.top_p, (int32_t)o.stop_byte};
        std::vector<int32_t> out_len(K);
        std::vector<int32_t> end_state(K, 0);
        if (guided) { // the mix, ahead of the processors, under whatever table the options made
            const lstm_hip_constraint con{(uint32_t)sizeof(lstm_hip_constraint), o.states, o.table.data()};
            const lstm_hip_beam_constraint bc{(uint32_t)sizeof(lstm_hip_beam_constraint), &con, o.has_regex ? o.accept.data() : nullptr};
            const bool tab = !o.table.empty();
            lstm_hip_logit_processors lp{(uint32_t)sizeof(lstm_hip_logit_processors), o.has_bias ? o.bias : nullptr, o.min_p,
                                         (int32_t)o.no_repeat, nullptr, nullptr};
            if (!o.has_guidance)
                CK(lstm_hip_generate_guided(h, K, prompts.data(), off.data(), nullptr, nullptr, &opt, u.empty() ? nullptr : u.data(), C,
                                            out.data(), nullptr, nullptr, nullptr, out_len.data(), nullptr, tab ? &bc : nullptr, nullptr,
                                            tab ? end_state.data() : nullptr, &lp, &gd));
            else { // both primings are calls that draw nothing; their end states start the drawing call, which gets no prompt
                const size_t n = (size_t)K * N;
                std::vector<float> hm(n), cm(n), hn, cn;
                CK(lstm_hip_generate(h, K, prompts.data(), off.data(), nullptr, nullptr, 1.0, nullptr, 0, nullptr, nullptr, hm.data(),
                                     cm.data()));
                if (!o.negative_prime.empty()) {
                    std::vector<uint64_t> noff(K + 1);
                    std::vector<uint8_t> neg;
                    for (int s = 0; s < K; s++) {
                        neg.insert(neg.end(), o.negative_prime.begin(), o.negative_prime.end());
                        noff[s + 1] = neg.size();
                    }
                    hn.resize(n), cn.resize(n);
                    CK(lstm_hip_generate(h, K, neg.data(), noff.data(), nullptr, nullptr, 1.0, nullptr, 0, nullptr, nullptr, hn.data(),
                                         cn.data()));
                }
                lstm_hip_guide self = guides[0];
                self.h0 = hn.empty() ? nullptr : hn.data();
                self.c0 = cn.empty() ? nullptr : cn.data();
                const lstm_hip_guidance own{(uint32_t)sizeof(lstm_hip_guidance), gd.main_weight, 1, &self};
                std::vector<int32_t> start(K, 0); // the table's state behind the prime, which the drawing call no longer walks
                if (tab) {
                    int32_t q = 0;
                    for (size_t i = 0; i < prime.size(); i++) {
                        const uint16_t v = o.table[(size_t)q * 256 + prime[i]];
                        if (v == 0xFFFF) die("--prime: byte " + std::to_string(i) + " is forbidden by the table the options made");
                        q = v;
                    }
                    std::fill(start.begin(), start.end(), q);
                }
                if (o.no_repeat > 0) { // the rule still sees the prime: as the history
                    lp.history = prompts.data();
                    lp.history_off = off.data();
                }
                CK(lstm_hip_generate_guided(h, K, nullptr, nullptr, hm.data(), cm.data(), &opt, u.empty() ? nullptr : u.data(), C,
                                            out.data(), nullptr, nullptr, nullptr, out_len.data(), nullptr, tab ? &bc : nullptr,
                                            tab ? start.data() : nullptr, tab ? end_state.data() : nullptr, &lp, &own));
            }
        } else if (o.has_bias || o.min_p > 0.0 || o.no_repeat > 0) { // logit processors, under whatever table the options made
            const lstm_hip_constraint con{(uint32_t)sizeof(lstm_hip_constraint), o.states, o.table.data()};
            const lstm_hip_beam_constraint bc{(uint32_t)sizeof(lstm_hip_beam_constraint), &con, o.has_regex ? o.accept.data() : nullptr};
            const lstm_hip_logit_processors lp{(uint32_t)sizeof(lstm_hip_logit_processors), o.has_bias ? o.bias : nullptr, o.min_p,
                                               (int32_t)o.no_repeat, nullptr, nullptr};
            const bool tab = !o.table.empty();
            CK(lstm_hip_generate_processed(h, K, prompts.data(), off.data(), nullptr, nullptr, &opt, u.empty() ? nullptr : u.data(), C,
                                           out.data(), nullptr, nullptr, nullptr, out_len.data(), nullptr, tab ? &bc : nullptr, nullptr,
                                           tab ? end_state.data() : nullptr, &lp));
        } else if (o.table.empty())
            CK(lstm_hip_generate_ex(h, K, prompts.data(), off.data(), nullptr, nullptr, &opt, u.empty() ? nullptr : u.data(), C,
                                    out.data(), nullptr, nullptr, nullptr, out_len.data(), nullptr));
        else if (o.has_regex) { // whole matches only: the accepting states and the deadline of --count
            const lstm_hip_constraint con{(uint32_t)sizeof(lstm_hip_constraint), o.states, o.table.data()};
            const lstm_hip_beam_constraint bc{(uint32_t)sizeof(lstm_hip_beam_constraint), &con, o.accept.data()};
            CK(lstm_hip_generate_accepting(h, K, prompts.data(), off.data(), nullptr, nullptr, &opt, u.empty() ? nullptr : u.data(), C,
                                           out.data(), nullptr, nullptr, nullptr, out_len.data(), nullptr, &bc, nullptr,
                                           end_state.data()));
        } else {
            const lstm_hip_constraint con{(uint32_t)sizeof(lstm_hip_constraint), o.states, o.table.data()};
            CK(lstm_hip_generate_constrained(h, K, prompts.data(), off.data(), nullptr, nullptr, &opt, u.empty() ? nullptr : u.data(),
                                             C, out.data(), nullptr, nullptr, nullptr, out_len.data(), nullptr, &con, nullptr,
                                             end_state.data()));
        }
        for (int s = 0; s < K; s++) {
            printf("== sample %d ==\n", s);
            std::vector<uint8_t> text(prime);
            for (int i = 0; i < out_len[s]; i++) text.push_back(out[(size_t)i * K + s]);
            size_t n = text.size();
            if (o.utf8 && !o.has_regex && end_state[s] != 0) { // cut back to the last character boundary (state 0 of the table)
                int32_t q = 0;
                n = 0;
                for (size_t i = 0; i < text.size(); i++) {
                    q = o.table[(size_t)q * 256 + text[i]];
                    if (q == 0) n = i + 1;
                }
            }
            fwrite(text.data(), 1, n, stdout);
            fputc('\n', stdout);
        }
    }
    for (lstm_hip_t *g : guide_handles) CK(lstm_hip_destroy(g));
    CK(lstm_hip_destroy(h));
    return 0;
}
