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
#include "../../include/lstm_hip.h"
#include "checkpoint.h"

#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

const char *const kUsage = "usage: lstm_compress --load PREFIX (-c|-d) IN OUT [--streams K] [--fast-math] [--device D]\n";
constexpr uint32_t kMagic = 0x4341484Cu; // "LHAC"
constexpr uint32_t kFormat = 1;
constexpr size_t kHeader = 44;
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
        else if (a == "-c" || a == "-d") {
            if (o.mode) usage("give one of -c and -d");
            o.mode = a[1];
            if (i + 2 >= argc) usage(a + " needs IN and OUT");
            o.in = argv[++i];
            o.out = argv[++i];
        } else if (a == "--streams") o.streams = parse_int(a, val(), 1, 4096);
        else if (a == "--device") o.device = parse_int(a, val(), 0, 1 << 20);
        else if (a == "--fast-math") o.flags |= LSTM_HIP_FAST_MATH;
        else if (a == "-h" || a == "--help") {
            printf("%s", kUsage);
            exit(0);
        } else usage("unknown argument " + a);
    }
    if (o.load.empty()) usage("--load PREFIX is required");
    if (!o.mode) usage("nothing to do: give -c or -d");
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

} // namespace

int main(int argc, char **argv) {
    const Options o = parse(argc, argv);
    if (o.mode == 'c') compress(o);
    else decompress(o);
    return 0;
}
