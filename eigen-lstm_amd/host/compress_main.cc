// compress_main.cc -- compress and decompress files with a trained model, through lstm_hip_encode / lstm_hip_decode
// (include/lstm_hip.h).  No HIP, no torch here.
//
//   lstm_compress --load PREFIX (-c|-d) IN OUT [--streams K] [--fast-math] [--device D]
//
// --load reads the five-file text checkpoint PREFIX_{W,U,Why,b,by}.txt (checkpoint.h); N is the rows of W / 4, and the
// handle is always padded (LSTM_HIP_PAD_HIDDEN), as lstm_generate's.
// -c splits IN into K streams, stream s = bytes [floor(s*len/K), floor((s+1)*len/K)), codes them side by side and writes
// the container below to OUT, then prints one line: input bytes, output bytes, code bytes, bits/char of the code and the
// model's ideal bits/char (sum of -log2(freq/total) / len).  Default K: len / 16384 clamped to [1, 256].
// -d checks the container against the checkpoint (magic, versions, N, parameter hash) before it creates a handle, decodes,
// checks the CRC32 and only then writes OUT (through a temporary file renamed into place).
// --fast-math (-c only) codes with LSTM_HIP_FAST_MATH; the flag is recorded in the container and -d follows it.
//
// Container, little-endian:
//   u32 magic "LHAC" | u32 format version | u32 coder version | u32 N | u32 flags (LSTM_HIP_FAST_MATH or 0)
//   | u64 FNV-1a of the logical parameter block (its float32 bytes) | u64 original length | u32 K | u32 CRC32 of the original
//   | K x u64 code lengths | the K codes back to back
//
//   lstm_compress --load PREFIX --guide PREFIX2 [--guide-weight B] [--main-weight A] [--mix-rate R] (-c|-d) IN OUT [...]
//
// --guide (up to four, each with its own --guide-weight behind it) codes on a log-linear mix of the --load model and the guides'
// (lstm_hip_encode_mixed / lstm_hip_decode_mixed): logits mixed with the weights A (default 0.5) and B
// (default 0.5 each), and with --mix-rate R > 0 (default 0: fixed weights) every stream learns its weights from the bytes it
// has coded.  --fast-math then applies to every model.  -d takes the same --load / --guide order, reads weights and rate from
// the container and names the model whose parameters differ.  Without --guide nothing changes: the container is LHAC.
//
// Mixed container, little-endian, G guides:
//   u32 magic "LHAM" | u32 format version | u32 coder version | u32 mix coder version | u32 1 + G
//   | (1 + G) x (u32 N | u32 flags (LSTM_HIP_FAST_MATH or 0) | u64 FNV-1a of the model's logical parameter block), main model first
//   | (1 + G) x u32 weight (the float's bits), main model first | u32 rate (the float's bits)
//   | u64 original length | u32 K | u32 CRC32 of the original | K x u64 code lengths | the K codes back to back
//
//   lstm_compress --adapt (-c|-d) IN OUT [--hidden N --seq S --streams B --lr X --seed K --optimizer adagrad|adam
//                 --adam-betas B1,B2 --adam-eps E --weight-decay W --clip-norm X --stable-softmax --bf16 --fast-math
//                 --load PREFIX --device D]
//
// --adapt codes with no checkpoint (lstm_hip_encode_adaptive / lstm_hip_decode_adaptive): the model
// starts from the seeded initialisation of `lstm` (rng.h: W, U, Why ~ N(0, 0.01) in that order, b = by = 0) -- or, with
// --load, from a checkpoint as a prior -- and trains on every block of S-1 bytes per stream after it was coded.  The B
// streams split IN as above.  -d takes everything from the container (only --device, and --load where a prior was used);
// the decoder repeats the training, so it needs the same device model and engine plan, which the container records.
//
// Adaptive container, little-endian (312-byte header):
//   u32 magic "LHAD" | u32 format version | u32 coder version | u32 adaptive version | u32 N | u32 S | u32 B | u32 create flags
//   | u64 lr (the double's bits) | u32 optimizer kind | u32 prior (1: --load) | 4 x u64 beta1, beta2, eps, weight decay (bits)
//   | u64 clip norm (bits) | u32 seed | u32 CU count | u64 FNV-1a of the INITIAL logical parameter block | u64 original length
//   | u32 CRC32 of the original | u32 0 | char[64] device name | char[128] plan identity (lstm_hip_plan_identity)
//   | B x u64 code lengths | the B codes back to back
#include "../../include/lstm_hip.h"
#include "checkpoint.h"
#include "rng.h"

#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

const char *const kUsage = "usage: lstm_compress --load PREFIX (-c|-d) IN OUT [--streams K] [--fast-math] [--device D]\n"
                            "       lstm_compress --load PREFIX --guide PREFIX2 [--guide-weight B] [--main-weight A] [--mix-rate R]\n"
                            "                     (-c|-d) IN OUT [--streams K] [--fast-math] [--device D]   (up to 4 --guide;\n"
                            "                     -d: the same --load / --guide order, weights and rate from the container)\n"
                            "       lstm_compress --adapt (-c|-d) IN OUT [--hidden N --seq S --streams B --lr X --seed K\n"
                            "                     --optimizer adagrad|adam --adam-betas B1,B2 --adam-eps E --weight-decay W\n"
                            "                     --clip-norm X --stable-softmax --bf16 --fast-math\n"
                            "                     --load PREFIX --device D]   (-d: only --device, and --load for a prior)\n";
constexpr uint32_t kMagic = 0x4341484Cu; // "LHAC"
constexpr uint32_t kFormat = 1;
constexpr size_t kHeader = 44;
constexpr uint32_t kMagicMixed = 0x4D41484Cu; // "LHAM"
constexpr uint32_t kFormatMixed = 1;
constexpr uint32_t kMagicAdaptive = 0x4441484Cu; // "LHAD"
constexpr uint32_t kFormatAdaptive = 1;
constexpr size_t kHeaderAdaptive = 312, kNameBytes = 64, kPlanBytes = 128;
constexpr uint32_t kKnownFlags = LSTM_HIP_FAST_MATH | LSTM_HIP_BF16_RECURRENCE | LSTM_HIP_PAD_HIDDEN |
                                 LSTM_HIP_STABLE_SOFTMAX;
constexpr uint64_t kBytesPerStream = 16384; // default K: one stream per 16 KB ...
constexpr long kDefaultMaxStreams = 256;   // ... up to 256 streams

[[noreturn]] void usage(const std::string &m) {
    fprintf(stderr, "lstm_compress: %s\n%s", m.c_str(), kUsage);
    exit(2);
}
[[noreturn]] void die(const std::string &m) {
    fprintf(stderr, "lstm_compress: %s\n", m.c_str());
    exit(1);
}
#define CK(call)                                                              \
    do {                                                                      \
        int rc_ = (call);                                                     \
        if (rc_ != 0) die(std::string(#call) + ": " + lstm_hip_last_error()); \
    } while (0)

long parse_int(const std::string &opt, const std::string &v, long lo, long hi) {
    char *end = nullptr;
    errno = 0;
    const long x = strtol(v.c_str(), &end, 10);
    if (v.empty() || *end != '\0' || errno != 0 || x < lo || x > hi)
        usage(opt + " needs an integer in [" + std::to_string(lo) + ", " + std::to_string(hi) + "], got '" + v + "'");
    return x;
}

struct Options {
    std::string load, in, out;
    char mode = 0; // 'c' or 'd'
    long streams = 0, device = 0; // streams 0: the default rule
    unsigned flags = 0;
    // --adapt
    bool adapt = false;
    std::string model_opt; // the last option given that only --adapt -c takes
    long N = 128, S = 32;
    uint32_t seed = 1;
    double lr = 0.05, beta1 = 0.9, beta2 = 0.999, adam_eps = 1e-8, weight_decay = 0.0, clip_norm = 0.0;
    bool adam = false;
    std::string adam_opt; // the last Adam option given (refused without --optimizer adam)
    // --guide
    std::vector<std::string> guides;
    std::vector<double> guide_weights; // one per guide
    double main_weight = 0.5, mix_rate = 0.0;
    std::string mix_opt; // the last option given that only --guide -c takes
};

double parse_double(const std::string &opt, const std::string &v, double lo, bool lo_open, double hi, bool inf_ok) {
    char *end = nullptr;
    errno = 0;
    const double x = strtod(v.c_str(), &end);
    const bool inf = std::isinf(x) && x > 0; // (hi is exclusive; +inf passes only where the option takes it)
    if (v.empty() || *end != '\0' || std::isnan(x) || x < lo || (lo_open && x == lo) || (inf ? !inf_ok : x >= hi))
        usage(opt + " needs a number " + (lo_open ? "> " : ">= ") + std::to_string(lo) + (std::isinf(hi) ? "" : " and < " + std::to_string(hi)) +
              ", got '" + v + "'");
    return x;
}
uint64_t dbits(double x) {
    uint64_t u;
    memcpy(&u, &x, 8);
    return u;
}
double bits_to_double(uint64_t u) {
    double x;
    memcpy(&x, &u, 8);
    return x;
}

Options parse(int argc, char **argv) {
    Options o;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto val = [&]() -> std::string {
            if (i + 1 >= argc) usage("missing value for " + a);
            return argv[++i];
        };
        if (a == "--load") o.load = val();
        else if (a == "-c" || a == "-d") {
            if (o.mode) usage("give one of -c and -d");
            o.mode = a[1];
            if (i + 2 >= argc) usage(a + " needs IN and OUT");
            o.in = argv[++i];
            o.out = argv[++i];
        } else if (a == "--streams") o.streams = parse_int(a, val(), 1, 4096);
        else if (a == "--device") o.device = parse_int(a, val(), 0, 1 << 20);
        else if (a == "--fast-math") o.flags |= LSTM_HIP_FAST_MATH;
        else if (a == "--adapt") o.adapt = true;
        else if (a == "--guide") {
            if (o.guides.size() == LSTM_HIP_MAX_GUIDES) usage("at most " + std::to_string(LSTM_HIP_MAX_GUIDES) + " --guide");
            o.guides.push_back(val());
            o.guide_weights.push_back(0.5);
        } else if (a == "--guide-weight") {
            const double w = parse_double(o.mix_opt = a, val(), -INFINITY, false, INFINITY, false);
            if (o.guides.empty()) usage("--guide-weight stands behind the --guide it belongs to");
            o.guide_weights.back() = w;
        } else if (a == "--main-weight") o.main_weight = parse_double(o.mix_opt = a, val(), -INFINITY, false, INFINITY, false);
        else if (a == "--mix-rate") o.mix_rate = parse_double(o.mix_opt = a, val(), 0.0, false, INFINITY, false);
        else if (a == "--hidden") o.N = parse_int(o.model_opt = a, val(), 1, 16384);
        else if (a == "--seq") o.S = parse_int(o.model_opt = a, val(), 2, 1 << 16);
        else if (a == "--seed") o.seed = (uint32_t)parse_int(o.model_opt = a, val(), 0, 0xFFFFFFFFl);
        else if (a == "--lr") o.lr = parse_double(o.model_opt = a, val(), 0.0, false, INFINITY, false);
        else if (a == "--clip-norm") o.clip_norm = parse_double(o.model_opt = a, val(), 0.0, false, INFINITY, true);
        else if (a == "--stable-softmax") o.model_opt = a, o.flags |= LSTM_HIP_STABLE_SOFTMAX;
        else if (a == "--bf16") o.model_opt = a, o.flags |= LSTM_HIP_BF16_RECURRENCE;
        else if (a == "--optimizer") {
            const std::string v = val();
            if (v != "adagrad" && v != "adam") usage("--optimizer needs adagrad or adam, got '" + v + "'");
            o.model_opt = a, o.adam = v == "adam";
        } else if (a == "--adam-betas") {
            const std::string v = val();
            const size_t comma = v.find(',');
            if (comma == std::string::npos) usage("--adam-betas needs B1,B2, got '" + v + "'");
            o.beta1 = parse_double(a, v.substr(0, comma), 0.0, false, 1.0, false);
            o.beta2 = parse_double(a, v.substr(comma + 1), 0.0, false, 1.0, false);
            o.model_opt = o.adam_opt = a;
        } else if (a == "--adam-eps") o.adam_eps = parse_double(o.model_opt = o.adam_opt = a, val(), 0.0, true, INFINITY, false);
        else if (a == "--weight-decay") o.weight_decay = parse_double(o.model_opt = o.adam_opt = a, val(), 0.0, false, INFINITY, false);
        else if (a == "-h" || a == "--help") {
            printf("%s", kUsage);
            exit(0);
        } else usage("unknown argument " + a);
    }
    if (!o.adapt) {
        if (!o.model_opt.empty()) usage(o.model_opt + " needs --adapt");
        if (o.load.empty()) usage("--load PREFIX is required");
    }
    if (!o.mode) usage("nothing to do: give -c or -d");
    if (o.adapt && !o.guides.empty()) usage("--guide needs --load without --adapt (the adaptive coders take no guides)");
    if (o.guides.empty() && !o.mix_opt.empty()) usage(o.mix_opt + " needs --guide");
    if (o.mode == 'd' && !o.mix_opt.empty()) usage(o.mix_opt + " is read from the container with -d");
    if (o.adapt && o.mode == 'd' && !o.model_opt.empty()) usage(o.model_opt + " is read from the container with -d");
    if (!o.adam_opt.empty() && !o.adam) usage(o.adam_opt + " needs --optimizer adam");
    if (o.mode == 'd' && o.streams) usage("--streams is read from the container with -d");
    if (o.mode == 'd' && o.flags) usage("--fast-math is read from the container with -d");
    return o;
}

bool read_file(const std::string &path, std::vector<uint8_t> &v) {
    FILE *fp = fopen(path.c_str(), "rb");
    if (!fp) return false;
    char buf[1 << 16];
    while (size_t len = fread(buf, 1, sizeof(buf), fp)) v.insert(v.end(), buf, buf + len);
    const bool ok = !ferror(fp);
    fclose(fp);
    return ok;
}
// written to OUT.tmp and renamed into place: OUT exists only when the whole file was written
void write_file(const std::string &path, const std::vector<uint8_t> &v) {
    const std::string tmp = path + ".tmp";
    FILE *fp = fopen(tmp.c_str(), "wb");
    if (!fp) die("cannot write " + tmp);
    const bool ok = fwrite(v.data(), 1, v.size(), fp) == v.size();
    if (fclose(fp) != 0 || !ok) {
        remove(tmp.c_str());
        die("cannot write " + tmp);
    }
    if (rename(tmp.c_str(), path.c_str()) != 0) {
        remove(tmp.c_str());
        die("cannot rename " + tmp + " to " + path);
    }
}

uint32_t crc32(const std::vector<uint8_t> &v) { // IEEE 802.3 (zlib's crc32)
    uint32_t table[256];
    for (uint32_t i = 0; i < 256; i++) {
        uint32_t c = i;
        for (int k = 0; k < 8; k++) c = c & 1 ? 0xEDB88320u ^ (c >> 1) : c >> 1;
        table[i] = c;
    }
    uint32_t c = 0xFFFFFFFFu;
    for (uint8_t b : v) c = table[(c ^ b) & 0xFF] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}
uint64_t fnv1a(const std::vector<float> &P) { // over the float32 bytes, little-endian
    uint64_t h = 0xcbf29ce484222325ull;
    for (float f : P) {
        uint32_t u;
        memcpy(&u, &f, 4);
        for (int k = 0; k < 4; k++) {
            h ^= (u >> (8 * k)) & 0xFF;
            h *= 0x100000001b3ull;
        }
    }
    return h;
}

void put32(std::vector<uint8_t> &v, uint32_t x) {
    for (int k = 0; k < 4; k++) v.push_back((uint8_t)(x >> (8 * k)));
}
void put64(std::vector<uint8_t> &v, uint64_t x) {
    for (int k = 0; k < 8; k++) v.push_back((uint8_t)(x >> (8 * k)));
}
uint32_t get32(const uint8_t *p) {
    uint32_t x = 0;
    for (int k = 0; k < 4; k++) x |= (uint32_t)p[k] << (8 * k);
    return x;
}
uint64_t get64(const uint8_t *p) {
    uint64_t x = 0;
    for (int k = 0; k < 8; k++) x |= (uint64_t)p[k] << (8 * k);
    return x;
}

// the checkpoint: N and the logical parameter block
int load_model(const std::string &prefix, std::vector<float> &P) {
    const int M = LSTM_HIP_VOCAB;
    std::string err;
    const int N = checkpoint::hidden_size(prefix, M, &err);
    if (N == 0) die(err);
    P.assign(lstm_hip_param_count(N, M), 0.0f);
    const int rc = checkpoint::load_params(prefix, P, N, M, &err);
    if (rc == 0) die("missing a file of " + prefix + "_{W,U,Why,b,by}.txt");
    if (rc < 0) die(err);
    return N;
}
lstm_hip_t *make_handle(int N, const std::vector<float> &P, unsigned flags, long device) {
    lstm_hip_config cfg{N, LSTM_HIP_VOCAB, 2, 1, (int32_t)device, flags | LSTM_HIP_PAD_HIDDEN};
    lstm_hip_t *h = nullptr;
    CK(lstm_hip_create(&cfg, &h));
    CK(lstm_hip_set_params(h, 0, P.data()));
    return h;
}

void compress(const Options &o) {
    std::vector<uint8_t> text;
    if (!read_file(o.in, text)) die("cannot read " + o.in);
    std::vector<float> P;
    const int N = load_model(o.load, P);
    const uint64_t len = text.size();
    long K = o.streams;
    if (K == 0) K = (long)std::min<uint64_t>(kDefaultMaxStreams, std::max<uint64_t>(1, len / kBytesPerStream));
    std::vector<uint64_t> off(K + 1);
    for (long s = 0; s <= K; s++) off[s] = (uint64_t)((unsigned __int128)s * len / (unsigned)K);
    uint64_t cap = 0;
    for (long s = 0; s < K; s++) cap += lstm_hip_code_bound(off[s + 1] - off[s]);
    std::vector<uint8_t> code(cap ? cap : 1);
    std::vector<uint64_t> code_off(K + 1);
    std::vector<double> bits(K);
    lstm_hip_t *h = make_handle(N, P, o.flags, o.device);
    CK(lstm_hip_encode(h, (int32_t)K, text.data(), off.data(), code.data(), cap, code_off.data(), bits.data(), nullptr));
    CK(lstm_hip_destroy(h));

    std::vector<uint8_t> out;
    put32(out, kMagic);
    put32(out, kFormat);
    put32(out, lstm_hip_coder_version());
    put32(out, (uint32_t)N);
    put32(out, o.flags & LSTM_HIP_FAST_MATH);
    put64(out, fnv1a(P));
    put64(out, len);
    put32(out, (uint32_t)K);
    put32(out, crc32(text));
    for (long s = 0; s < K; s++) put64(out, code_off[s + 1] - code_off[s]);
    out.insert(out.end(), code.begin(), code.begin() + code_off[K]);
    write_file(o.out, out);
    double sum = 0.0;
    for (double b : bits) sum += b;
    const double n = len ? (double)len : 1.0;
    printf("in %llu bytes, out %zu bytes, code %llu bytes in %ld streams: %.5f bits/char (model %.5f bits/char)\n",
           (unsigned long long)len, out.size(), (unsigned long long)code_off[K], K, 8.0 * (double)code_off[K] / n, sum / n);
}

void decompress(const Options &o) {
    std::vector<uint8_t> in;
    if (!read_file(o.in, in)) die("cannot read " + o.in);
    if (in.size() >= 4 && get32(&in[0]) == kMagicAdaptive)
        die(o.in + ": an adaptive lstm_compress file (LHAD): decode it with --adapt -d");
    if (in.size() >= 4 && get32(&in[0]) == kMagicMixed)
        die(o.in + ": a mixed lstm_compress file (LHAM): decode it with --load PREFIX --guide PREFIX2 -d");
    if (in.size() < kHeader) die(o.in + ": truncated header (" + std::to_string(in.size()) + " bytes)");
    if (get32(&in[0]) != kMagic) die(o.in + ": not an lstm_compress file (bad magic)");
    if (get32(&in[4]) != kFormat) die(o.in + ": container format " + std::to_string(get32(&in[4])) + ", this program reads " + std::to_string(kFormat));
    if (get32(&in[8]) != lstm_hip_coder_version())
        die(o.in + ": coder version " + std::to_string(get32(&in[8])) + ", this library codes version " + std::to_string(lstm_hip_coder_version()));
    const uint32_t N = get32(&in[12]), flags = get32(&in[16]);
    const uint64_t hash = get64(&in[20]), len = get64(&in[28]);
    const uint32_t K = get32(&in[36]), crc = get32(&in[40]);
    if (flags & ~LSTM_HIP_FAST_MATH) die(o.in + ": unknown flags " + std::to_string(flags));
    if (K < 1 || K > 4096) die(o.in + ": stream count " + std::to_string(K) + " outside [1, 4096]");
    if (in.size() < kHeader + 8ull * K) die(o.in + ": truncated header (" + std::to_string(in.size()) + " bytes)");
    std::vector<uint64_t> code_off(K + 1, 0), text_off(K + 1);
    for (uint32_t s = 0; s < K; s++) {
        const uint64_t n = get64(&in[kHeader + 8 * s]);
        if (n > in.size()) die(o.in + ": corrupt code length");
        code_off[s + 1] = code_off[s] + n;
    }
    if (code_off[K] != in.size() - kHeader - 8ull * K)
        die(o.in + ": " + std::to_string(in.size() - kHeader - 8ull * K) + " code bytes, the header says " + std::to_string(code_off[K]));
    for (uint32_t s = 0; s <= K; s++) text_off[s] = (uint64_t)((unsigned __int128)s * len / K);

    std::vector<float> P;
    const int Nc = load_model(o.load, P);
    if ((uint32_t)Nc != N) die(o.in + ": coded with a hidden size of " + std::to_string(N) + ", the checkpoint has " + std::to_string(Nc));
    if (fnv1a(P) != hash) die(o.in + ": coded with other parameters than " + o.load + " (parameter hash differs)");

    std::vector<uint8_t> text(len ? len : 1);
    lstm_hip_t *h = make_handle(Nc, P, flags, o.device);
    CK(lstm_hip_decode(h, (int32_t)K, in.data() + kHeader + 8ull * K, code_off.data(), text_off.data(), text.data()));
    CK(lstm_hip_destroy(h));
    text.resize(len);
    if (crc32(text) != crc) die(o.in + ": CRC32 of the decoded text differs; " + o.out + " not written");
    write_file(o.out, text);
}

// ---- --guide -------------------------------------------------------------------------------------------------------------
uint32_t fbits(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    return u;
}
float bits_to_float(uint32_t u) {
    float x;
    memcpy(&x, &u, 4);
    return x;
}
struct MixedModels { // the --load model, then the guides in their order
    std::vector<std::string> prefix;
    std::vector<std::vector<float>> P;
    std::vector<int> N;
    std::vector<lstm_hip_t *> h;
    std::vector<lstm_hip_guide> guide;
    lstm_hip_guidance gd{};
    lstm_hip_mix_coding mx{};
};
void load_mixed(const Options &o, MixedModels &m) {
    m.prefix.push_back(o.load);
    m.prefix.insert(m.prefix.end(), o.guides.begin(), o.guides.end());
    m.P.resize(m.prefix.size());
    for (size_t k = 0; k < m.prefix.size(); k++) m.N.push_back(load_model(m.prefix[k], m.P[k]));
}
// the handles and the two blocks of the call: weights[0] the main model's
void open_mixed(MixedModels &m, unsigned flags, long device, const std::vector<float> &weights, float rate) {
    for (size_t k = 0; k < m.prefix.size(); k++) m.h.push_back(make_handle(m.N[k], m.P[k], flags, device));
    for (size_t k = 1; k < m.h.size(); k++) m.guide.push_back(lstm_hip_guide{m.h[k], (double)weights[k], nullptr, nullptr, nullptr, nullptr});
    m.gd = lstm_hip_guidance{sizeof(lstm_hip_guidance), (double)weights[0], (int32_t)m.guide.size(), m.guide.data()};
    m.mx = lstm_hip_mix_coding{sizeof(lstm_hip_mix_coding), (double)rate};
}
void close_mixed(MixedModels &m) {
    for (lstm_hip_t *h : m.h) CK(lstm_hip_destroy(h));
}

void compress_mixed(const Options &o) {
    std::vector<uint8_t> text;
    if (!read_file(o.in, text)) die("cannot read " + o.in);
    MixedModels m;
    load_mixed(o, m);
    const uint64_t len = text.size();
    long K = o.streams;
    if (K == 0) K = (long)std::min<uint64_t>(kDefaultMaxStreams, std::max<uint64_t>(1, len / kBytesPerStream));
    std::vector<uint64_t> off(K + 1);
    for (long s = 0; s <= K; s++) off[s] = (uint64_t)((unsigned __int128)s * len / (unsigned)K);
    uint64_t cap = 0;
    for (long s = 0; s < K; s++) cap += lstm_hip_code_bound(off[s + 1] - off[s]);
    std::vector<uint8_t> code(cap ? cap : 1);
    std::vector<uint64_t> code_off(K + 1);
    std::vector<double> bits(K);
    std::vector<float> weights{(float)o.main_weight}; // narrowed here, as the library narrows them: the container holds what was used
    for (double w : o.guide_weights) weights.push_back((float)w);
    const float rate = (float)o.mix_rate;
    const size_t G1 = weights.size();
    std::vector<float> w_out((size_t)K * G1);
    open_mixed(m, o.flags, o.device, weights, rate);
    CK(lstm_hip_encode_mixed(m.h[0], (int32_t)K, text.data(), off.data(), code.data(), cap, code_off.data(), bits.data(), nullptr, &m.gd,
                             &m.mx, w_out.data(), nullptr));
    close_mixed(m);

    std::vector<uint8_t> out;
    put32(out, kMagicMixed);
    put32(out, kFormatMixed);
    put32(out, lstm_hip_coder_version());
    put32(out, lstm_hip_mix_coder_version());
    put32(out, (uint32_t)G1);
    for (size_t k = 0; k < G1; k++) {
        put32(out, (uint32_t)m.N[k]);
        put32(out, o.flags & LSTM_HIP_FAST_MATH);
        put64(out, fnv1a(m.P[k]));
    }
    for (float w : weights) put32(out, fbits(w));
    put32(out, fbits(rate));
    put64(out, len);
    put32(out, (uint32_t)K);
    put32(out, crc32(text));
    for (long s = 0; s < K; s++) put64(out, code_off[s + 1] - code_off[s]);
    out.insert(out.end(), code.begin(), code.begin() + code_off[K]);
    write_file(o.out, out);
    double sum = 0.0;
    for (double b : bits) sum += b;
    const double n = len ? (double)len : 1.0;
    printf("in %llu bytes, out %zu bytes, code %llu bytes in %ld streams, %zu models: %.5f bits/char (model %.5f bits/char)\n",
           (unsigned long long)len, out.size(), (unsigned long long)code_off[K], K, G1, 8.0 * (double)code_off[K] / n, sum / n);
    if (rate > 0.0f)
        for (size_t k = 0; k < G1; k++) { // the range of the streams' final weights, per model
            float lo = w_out[k], hi = w_out[k];
            for (long s = 1; s < K; s++) lo = std::min(lo, w_out[s * G1 + k]), hi = std::max(hi, w_out[s * G1 + k]);
            printf("model %zu: weight %g, final %g .. %g\n", k, (double)weights[k], (double)lo, (double)hi);
        }
}

void decompress_mixed(const Options &o) {
    std::vector<uint8_t> in;
    if (!read_file(o.in, in)) die("cannot read " + o.in);
    if (in.size() >= 4 && get32(&in[0]) == kMagic) die(o.in + ": a static lstm_compress file (LHAC), coded without guides: decode it without --guide");
    if (in.size() >= 4 && get32(&in[0]) == kMagicAdaptive) die(o.in + ": an adaptive lstm_compress file (LHAD): decode it with --adapt -d");
    if (in.size() < 20) die(o.in + ": truncated header (" + std::to_string(in.size()) + " bytes)");
    if (get32(&in[0]) != kMagicMixed) die(o.in + ": not a mixed lstm_compress file (bad magic)");
    if (get32(&in[4]) != kFormatMixed) die(o.in + ": container format " + std::to_string(get32(&in[4])) + ", this program reads " + std::to_string(kFormatMixed));
    if (get32(&in[8]) != lstm_hip_coder_version())
        die(o.in + ": coder version " + std::to_string(get32(&in[8])) + ", this library codes version " + std::to_string(lstm_hip_coder_version()));
    if (get32(&in[12]) != lstm_hip_mix_coder_version())
        die(o.in + ": mix coder version " + std::to_string(get32(&in[12])) + ", this library codes version " +
            std::to_string(lstm_hip_mix_coder_version()));
    const uint32_t G1 = get32(&in[16]);
    if (G1 < 2 || G1 > 1 + LSTM_HIP_MAX_GUIDES) die(o.in + ": model count " + std::to_string(G1) + " outside [2, " + std::to_string(1 + LSTM_HIP_MAX_GUIDES) + "]");
    if (G1 != 1 + o.guides.size())
        die(o.in + ": coded with " + std::to_string(G1 - 1) + " guides, " + std::to_string(o.guides.size()) + " given with --guide");
    const size_t header = 20 + 16ull * G1 + 4ull * G1 + 4 + 16;
    if (in.size() < header) die(o.in + ": truncated header (" + std::to_string(in.size()) + " bytes)");
    const uint8_t *at = &in[20 + 16ull * G1];
    std::vector<float> weights;
    for (uint32_t k = 0; k < G1; k++) weights.push_back(bits_to_float(get32(at + 4 * k)));
    at += 4ull * G1;
    const float rate = bits_to_float(get32(at));
    const uint64_t len = get64(at + 4);
    const uint32_t K = get32(at + 12), crc = get32(at + 16);
    for (float w : weights)
        if (!std::isfinite(w)) die(o.in + ": corrupt weight");
    if (!std::isfinite(rate) || rate < 0.0f) die(o.in + ": corrupt mix rate");
    if (K < 1 || K > 4096) die(o.in + ": stream count " + std::to_string(K) + " outside [1, 4096]");
    if (in.size() < header + 8ull * K) die(o.in + ": truncated header (" + std::to_string(in.size()) + " bytes)");
    std::vector<uint64_t> code_off(K + 1, 0), text_off(K + 1);
    for (uint32_t s = 0; s < K; s++) {
        const uint64_t n = get64(&in[header + 8 * s]);
        if (n > in.size()) die(o.in + ": corrupt code length");
        code_off[s + 1] = code_off[s] + n;
    }
    if (code_off[K] != in.size() - header - 8ull * K)
        die(o.in + ": " + std::to_string(in.size() - header - 8ull * K) + " code bytes, the header says " + std::to_string(code_off[K]));
    for (uint32_t s = 0; s <= K; s++) text_off[s] = (uint64_t)((unsigned __int128)s * len / K);

    MixedModels m;
    load_mixed(o, m);
    uint32_t flags = 0;
    for (uint32_t k = 0; k < G1; k++) { // every model against its record, before any handle is made
        const uint8_t *rec = &in[20 + 16ull * k];
        const std::string who = k == 0 ? "the --load model " + m.prefix[k] : "guide " + std::to_string(k) + " (" + m.prefix[k] + ")";
        if (get32(rec + 4) & ~LSTM_HIP_FAST_MATH) die(o.in + ": unknown flags " + std::to_string(get32(rec + 4)));
        if (k == 0) flags = get32(rec + 4);
        else if (get32(rec + 4) != flags) die(o.in + ": the models' flags differ");
        if (get32(rec) != (uint32_t)m.N[k])
            die(o.in + ": model " + std::to_string(k) + " was coded with a hidden size of " + std::to_string(get32(rec)) + ", " + who + " has " +
                std::to_string(m.N[k]));
        if (get64(rec + 8) != fnv1a(m.P[k]))
            die(o.in + ": model " + std::to_string(k) + " was coded with other parameters than " + who + " (parameter hash differs)");
    }
    std::vector<uint8_t> text(len ? len : 1);
    open_mixed(m, flags, o.device, weights, rate);
    CK(lstm_hip_decode_mixed(m.h[0], (int32_t)K, in.data() + header + 8ull * K, code_off.data(), text_off.data(), text.data(), &m.gd, &m.mx,
                             nullptr));
    close_mixed(m);
    text.resize(len);
    if (crc32(text) != crc) die(o.in + ": CRC32 of the decoded text differs; " + o.out + " not written");
    write_file(o.out, text);
}

// ---- --adapt ------------------------------------------------------------------------------------------------------------
struct Adaptive { // what fixes the model and its training: the container's fields
    uint32_t N = 0, S = 0, B = 0, flags = 0, opt = LSTM_HIP_OPT_ADAGRAD, prior = 0, seed = 0;
    double lr = 0.0, beta1 = 0.0, beta2 = 0.0, eps = 0.0, wd = 0.0, clip = 0.0;
};
// the initial logical parameter block: lstm's seeded initialisation, or the checkpoint where a prior was given
std::vector<float> initial_params(const Adaptive &m, const std::string &load, const std::string &what) {
    const int M = LSTM_HIP_VOCAB;
    std::vector<float> P;
    if (m.prior) {
        const int Nc = load_model(load, P);
        if ((uint32_t)Nc != m.N) die(what + ": a hidden size of " + std::to_string(m.N) + ", the checkpoint " + load + " has " + std::to_string(Nc));
        return P;
    }
    P.assign(lstm_hip_param_count((int32_t)m.N, M), 0.0f);
    SeededRng rng(m.seed);
    const auto bl = checkpoint::blocks((int)m.N, M);
    rng.randn(P.data() + bl[0].off, 4 * (int)m.N, M, 0.0, 0.01);
    rng.randn(P.data() + bl[1].off, 4 * (int)m.N, (int)m.N, 0.0, 0.01);
    rng.randn(P.data() + bl[3].off, M, (int)m.N, 0.0, 0.01);
    return P;
}
struct Identity {
    char name[kNameBytes] = {};
    char plan[kPlanBytes] = {};
    int32_t cus = 0;
};
lstm_hip_t *make_adaptive_handle(const Adaptive &m, const std::vector<float> &P, long device, Identity &id) {
    lstm_hip_config cfg{(int32_t)m.N, LSTM_HIP_VOCAB, (int32_t)m.S, (int32_t)m.B, (int32_t)device, m.flags};
    lstm_hip_t *h = nullptr;
    CK(lstm_hip_create(&cfg, &h));
    CK(lstm_hip_set_params(h, 0, P.data()));
    if (m.opt == LSTM_HIP_OPT_ADAM) CK(lstm_hip_set_optimizer(h, LSTM_HIP_OPT_ADAM, m.beta1, m.beta2, m.eps, m.wd));
    if (m.clip > 0.0) CK(lstm_hip_set_grad_clip(h, m.clip));
    int32_t mhz = 0;
    CK(lstm_hip_device_info((int32_t)device, id.name, &id.cus, &mhz));
    CK(lstm_hip_plan_identity(h, id.plan, sizeof(id.plan)));
    return h;
}

void compress_adaptive(const Options &o) {
    std::vector<uint8_t> text;
    if (!read_file(o.in, text)) die("cannot read " + o.in);
    const uint64_t len = text.size();
    Adaptive m;
    m.N = (uint32_t)o.N, m.S = (uint32_t)o.S, m.flags = o.flags | LSTM_HIP_PAD_HIDDEN, m.seed = o.seed, m.lr = o.lr, m.clip = o.clip_norm;
    m.prior = o.load.empty() ? 0 : 1;
    if (o.adam) m.opt = LSTM_HIP_OPT_ADAM, m.beta1 = o.beta1, m.beta2 = o.beta2, m.eps = o.adam_eps, m.wd = o.weight_decay;
    if (m.prior) {
        std::string err;
        const int Nc = checkpoint::hidden_size(o.load, LSTM_HIP_VOCAB, &err);
        if (Nc == 0) die(err);
        m.N = (uint32_t)Nc; // the prior decides the hidden size
    }
    long K = o.streams;
    if (K == 0) K = (long)std::min<uint64_t>(kDefaultMaxStreams, std::max<uint64_t>(1, len / kBytesPerStream));
    m.B = (uint32_t)K;
    const std::vector<float> P = initial_params(m, o.load, o.in);
    std::vector<uint64_t> off(K + 1);
    for (long s = 0; s <= K; s++) off[s] = (uint64_t)((unsigned __int128)s * len / (unsigned)K);
    uint64_t cap = 0;
    for (long s = 0; s < K; s++) cap += lstm_hip_code_bound(off[s + 1] - off[s]);
    std::vector<uint8_t> code(cap ? cap : 1);
    std::vector<uint64_t> code_off(K + 1);
    std::vector<double> bits(K);
    Identity id;
    lstm_hip_t *h = make_adaptive_handle(m, P, o.device, id);
    CK(lstm_hip_encode_adaptive(h, text.data(), off.data(), m.lr, code.data(), cap, code_off.data(), bits.data(), nullptr, nullptr));
    CK(lstm_hip_destroy(h));

    std::vector<uint8_t> out;
    put32(out, kMagicAdaptive);
    put32(out, kFormatAdaptive);
    put32(out, lstm_hip_coder_version());
    put32(out, lstm_hip_adaptive_version());
    put32(out, m.N);
    put32(out, m.S);
    put32(out, m.B);
    put32(out, m.flags);
    put64(out, dbits(m.lr));
    put32(out, m.opt);
    put32(out, m.prior);
    put64(out, dbits(m.beta1));
    put64(out, dbits(m.beta2));
    put64(out, dbits(m.eps));
    put64(out, dbits(m.wd));
    put64(out, dbits(m.clip));
    put32(out, m.seed);
    put32(out, (uint32_t)id.cus);
    put64(out, fnv1a(P));
    put64(out, len);
    put32(out, crc32(text));
    put32(out, 0);
    out.insert(out.end(), id.name, id.name + kNameBytes);
    out.insert(out.end(), id.plan, id.plan + kPlanBytes);
    if (out.size() != kHeaderAdaptive) die("internal: adaptive header size");
    for (long s = 0; s < K; s++) put64(out, code_off[s + 1] - code_off[s]);
    out.insert(out.end(), code.begin(), code.begin() + code_off[K]);
    write_file(o.out, out);
    double sum = 0.0;
    for (double b : bits) sum += b;
    const double n = len ? (double)len : 1.0;
    printf("in %llu bytes, out %zu bytes, code %llu bytes in %ld streams, %lld trained blocks: %.5f bits/char (model %.5f bits/char)\n",
           (unsigned long long)len, out.size(), (unsigned long long)code_off[K], K,
           (long long)lstm_hip_adaptive_blocks((int32_t)m.S, (int32_t)m.B, off.data()), 8.0 * (double)code_off[K] / n, sum / n);
}

void decompress_adaptive(const Options &o) {
    std::vector<uint8_t> in;
    if (!read_file(o.in, in)) die("cannot read " + o.in);
    if (in.size() >= 4 && get32(&in[0]) == kMagic) die(o.in + ": a static lstm_compress file (LHAC): decode it with --load PREFIX -d");
    if (in.size() >= 4 && get32(&in[0]) == kMagicMixed)
        die(o.in + ": a mixed lstm_compress file (LHAM): decode it with --load PREFIX --guide PREFIX2 -d");
    if (in.size() < kHeaderAdaptive) die(o.in + ": truncated header (" + std::to_string(in.size()) + " bytes)");
    if (get32(&in[0]) != kMagicAdaptive) die(o.in + ": not an adaptive lstm_compress file (bad magic)");
    if (get32(&in[4]) != kFormatAdaptive)
        die(o.in + ": container format " + std::to_string(get32(&in[4])) + ", this program reads " + std::to_string(kFormatAdaptive));
    if (get32(&in[8]) != lstm_hip_coder_version())
        die(o.in + ": coder version " + std::to_string(get32(&in[8])) + ", this library codes version " + std::to_string(lstm_hip_coder_version()));
    if (get32(&in[12]) != lstm_hip_adaptive_version())
        die(o.in + ": adaptive version " + std::to_string(get32(&in[12])) + ", this library codes version " +
            std::to_string(lstm_hip_adaptive_version()));
    Adaptive m;
    m.N = get32(&in[16]), m.S = get32(&in[20]), m.B = get32(&in[24]), m.flags = get32(&in[28]);
    m.lr = bits_to_double(get64(&in[32]));
    m.opt = get32(&in[40]), m.prior = get32(&in[44]);
    m.beta1 = bits_to_double(get64(&in[48])), m.beta2 = bits_to_double(get64(&in[56]));
    m.eps = bits_to_double(get64(&in[64])), m.wd = bits_to_double(get64(&in[72]));
    m.clip = bits_to_double(get64(&in[80]));
    m.seed = get32(&in[88]);
    const uint32_t cus = get32(&in[92]), crc = get32(&in[112]);
    const uint64_t hash = get64(&in[96]), len = get64(&in[104]);
    if (m.N < 1 || m.N > 16384) die(o.in + ": hidden size " + std::to_string(m.N) + " outside [1, 16384]");
    if (m.S < 2 || m.S > (1u << 16)) die(o.in + ": window of " + std::to_string(m.S) + " columns outside [2, 65536]");
    if (m.B < 1 || m.B > 4096) die(o.in + ": stream count " + std::to_string(m.B) + " outside [1, 4096]");
    if ((m.flags & ~kKnownFlags) || !(m.flags & LSTM_HIP_PAD_HIDDEN)) die(o.in + ": unknown flags " + std::to_string(m.flags));
    if (!std::isfinite(m.lr) || m.lr < 0.0) die(o.in + ": corrupt learning rate");
    if (m.opt != LSTM_HIP_OPT_ADAGRAD && m.opt != LSTM_HIP_OPT_ADAM) die(o.in + ": unknown optimizer kind " + std::to_string(m.opt));
    if (m.prior > 1) die(o.in + ": corrupt prior field");
    if (std::isnan(m.clip) || m.clip < 0.0) die(o.in + ": corrupt clip norm");
    const uint32_t K = m.B;
    if (in.size() < kHeaderAdaptive + 8ull * K) die(o.in + ": truncated header (" + std::to_string(in.size()) + " bytes)");
    std::vector<uint64_t> code_off(K + 1, 0), text_off(K + 1);
    for (uint32_t s = 0; s < K; s++) {
        const uint64_t n = get64(&in[kHeaderAdaptive + 8 * s]);
        if (n > in.size()) die(o.in + ": corrupt code length");
        code_off[s + 1] = code_off[s] + n;
    }
    const uint64_t have = in.size() - kHeaderAdaptive - 8ull * K;
    if (code_off[K] != have) die(o.in + ": " + std::to_string(have) + " code bytes, the header says " + std::to_string(code_off[K]));
    for (uint32_t s = 0; s <= K; s++) text_off[s] = (uint64_t)((unsigned __int128)s * len / K);
    if (m.prior && o.load.empty()) die(o.in + ": coded with a checkpoint as prior: give it with --load PREFIX");
    if (!m.prior && !o.load.empty()) die(o.in + ": coded from the seeded initialisation, not from a checkpoint: drop --load");
    const std::vector<float> P = initial_params(m, o.load, o.in + ": coded with");
    if (fnv1a(P) != hash) die(o.in + ": the initial parameters differ from the coder's (parameter hash differs)");

    std::vector<uint8_t> text(len ? len : 1);
    Identity id;
    lstm_hip_t *h = make_adaptive_handle(m, P, o.device, id);
    char name[kNameBytes + 1] = {}, plan[kPlanBytes + 1] = {};
    memcpy(name, &in[120], kNameBytes);
    memcpy(plan, &in[120 + kNameBytes], kPlanBytes);
    if (strncmp(name, id.name, kNameBytes) != 0)
        die(o.in + ": coded on device name '" + name + "', this device is '" + id.name + "' (the training sums would differ)");
    if ((int32_t)cus != id.cus)
        die(o.in + ": coded with a CU count of " + std::to_string(cus) + ", this device has " + std::to_string(id.cus));
    if (strncmp(plan, id.plan, kPlanBytes) != 0)
        die(o.in + ": coded with plan identity '" + plan + "', this library and device choose '" + id.plan + "'");
    CK(lstm_hip_decode_adaptive(h, in.data() + kHeaderAdaptive + 8ull * K, code_off.data(), text_off.data(), m.lr, text.data()));
    CK(lstm_hip_destroy(h));
    text.resize(len);
    if (crc32(text) != crc) die(o.in + ": CRC32 of the decoded text differs; " + o.out + " not written");
    write_file(o.out, text);
}

} // namespace

int main(int argc, char **argv) {
    const Options o = parse(argc, argv);
    if (o.adapt) {
        if (o.mode == 'c') compress_adaptive(o);
        else decompress_adaptive(o);
        return 0;
    }
    if (!o.guides.empty()) {
        if (o.mode == 'c') compress_mixed(o);
        else decompress_mixed(o);
        return 0;
    }
    if (o.mode == 'c') compress(o);
    else decompress(o);
    return 0;
}
