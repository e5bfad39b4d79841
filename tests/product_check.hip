// product_check.hip -- driver of tests/test_products.py: runs the window's dense products and bf16 packers (csrc/gemm.hip,
// csrc/kernels.hip) on operands a test wrote, and writes back everything they touched.  No kernels of its own, no judgement of
// its own: it links liblstm_hip.so, calls the launch wrappers of csrc/kernels.h on the default stream and dumps whole
// allocations; every check is in Python (tests/product_cases.py).
//
//   product_check <dir>        reads <dir>/manifest.txt, writes <dir>/results.txt and <dir>/<id>.<buffer>.r<rep>
//
// A manifest line is `<kind> <id> key=value ...` (decimal integers; `sent` is hexadecimal).  Operands are raw little-endian
// files <dir>/<id>.A and <dir>/<id>.B, uploaded into allocations of exactly a_n / b_n elements.  Every output allocation is
//   [GUARD bytes][payload, rounded up to 4 bytes][GUARD bytes]
// filled with the 32-bit pattern `sent` before the call and written back whole afterwards, so rows M..ldc-1, unused slabs and
// both guards show whatever the call did to them.  rep > 1 repeats the job (fresh sentinels, output files .r0, .r1, ...).
// Kinds and their keys:
//   gemm                 TA TB M Nn K lda ldb ldc splits a_n b_n b_off slab_n      -> C (ldc*Nn floats), S (slab_n floats)
//   gemm_slabs           the same, and fold=0/1: gemm_fold over the slabs written  -> S, C when fold; ret = slabs written
//   gemm_fold            splits M Nn ldc stride a_n (A: the slabs)                 -> C
//   gemm_bf16            M Nn K lda ldb ldc splits a_n b_n b_off slab_n (bf16 A, B)-> C, S
//   transpose_pack_bf16  K R ld Kpad a_n                                           -> C (R*Kpad halfwords)
//   pack_bf16            n (a_n = n)                                               -> C (n halfwords)
//   pick_splits          bf16 TA TB M Nn K                                         -> pick0, pick1 (two calls)
// splits = -1: the count the library's shape rule picks for this device (recorded as `picked`).  b_off: elements added to B's
// base.  results.txt: `n_cus <n>` first, then `<id> <rep> <key> <value>` lines.
// On the first HIP error the driver prints the call and the error and exits with status 3 without launching anything more;
// a malformed manifest or a job whose outputs would not fit its allocations is status 2 (nothing of that job is launched).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>
#include "kernels.h"
#include "lstm_hip.h"

namespace {

constexpr size_t GUARD = 256; // bytes before and after every output payload (keeps the payload 16-byte aligned)
std::string g_dir, g_where;
FILE *g_res = nullptr;

[[noreturn]] void die(int status, const std::string &msg) {
    fprintf(stderr, "product_check: %s: %s\n", g_where.c_str(), msg.c_str());
    fflush(stderr);
    if (g_res) fclose(g_res);
    exit(status);
}
void hip_ok(hipError_t e, const char *call) {
    if (e != hipSuccess) die(3, std::string(call) + ": " + hipGetErrorString(e));
}
#define HIP_OK(x) hip_ok((x), #x)
// after a launch wrapper: the launch status, then the kernels' own
void launched(const char *call) {
    hip_ok(hipGetLastError(), call);
    hip_ok(hipStreamSynchronize(nullptr), call);
}

struct Job {
    std::string kind, id;
    std::map<std::string, long long> kv;
    long long get(const char *k) const {
        auto it = kv.find(k);
        if (it == kv.end()) die(2, std::string("missing key ") + k);
        return it->second;
    }
    long long get(const char *k, long long dflt) const {
        auto it = kv.find(k);
        return it == kv.end() ? dflt : it->second;
    }
};

void *upload(const Job &j, const char *suffix, size_t bytes) {
    if (bytes == 0) return nullptr;
    const std::string path = g_dir + "/" + j.id + "." + suffix;
    std::vector<char> host(bytes);
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) die(2, "cannot open " + path);
    const size_t got = fread(host.data(), 1, bytes, f);
    const bool more = fgetc(f) != EOF;
    fclose(f);
    if (got != bytes || more) die(2, path + ": size differs from the declared one");
    void *d = nullptr;
    HIP_OK(hipMalloc(&d, bytes));
    HIP_OK(hipMemcpy(d, host.data(), bytes, hipMemcpyHostToDevice));
    return d;
}

struct Out {
    char *base = nullptr;
    size_t bytes = 0, total = 0;
    void alloc(size_t payload_bytes) {
        bytes = payload_bytes;
        total = GUARD + (payload_bytes + 3) / 4 * 4 + GUARD;
        HIP_OK(hipMalloc(reinterpret_cast<void **>(&base), total));
    }
    void fill(unsigned sent) { HIP_OK(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(base), (int)sent, total / 4)); }
    template <class T> T *payload() const { return bytes ? reinterpret_cast<T *>(base + GUARD) : nullptr; }
    void dump(const Job &j, const char *suffix, int rep) const {
        if (!base) return;
        std::vector<char> host(total);
        HIP_OK(hipMemcpy(host.data(), base, total, hipMemcpyDeviceToHost));
        const std::string path = g_dir + "/" + j.id + "." + suffix + ".r" + std::to_string(rep);
        FILE *f = fopen(path.c_str(), "wb");
        if (!f || fwrite(host.data(), 1, total, f) != total) die(2, "cannot write " + path);
        fclose(f);
    }
    void release() {
        if (base) HIP_OK(hipFree(base));
        base = nullptr;
    }
};

void result(const Job &j, int rep, const char *key, long long v) {
    fprintf(g_res, "%s %d %s %lld\n", j.id.c_str(), rep, key, v);
    fflush(g_res);
}

void run_gemm(const Job &j, int n_cus, bool slabs_only, bool bf16) {
    const bool TA = !bf16 && j.get("TA"), TB = !bf16 && j.get("TB");
    const int M = (int)j.get("M"), Nn = (int)j.get("Nn"), K = (int)j.get("K");
    const int lda = (int)j.get("lda"), ldb = (int)j.get("ldb"), ldc = (int)j.get("ldc", M);
    const size_t a_n = (size_t)j.get("a_n"), b_n = (size_t)j.get("b_n"), b_off = (size_t)j.get("b_off", 0);
    const size_t slab_n = (size_t)j.get("slab_n", 0), esz = bf16 ? 2 : 4;
    const bool fold = slabs_only && j.get("fold", 0);
    int splits = (int)j.get("splits");
    const bool pick = splits < 0;
    if (pick) splits = bf16 ? lstmk::gemm_bf16_pick_splits(M, Nn, K) : lstmk::gemm_pick_splits(TA, TB, M, Nn, K, n_cus);
    if (M < 1 || Nn < 1 || K < 1 || ldc < M || b_off > b_n) die(2, "bad shape");
    if ((splits > 1 || slabs_only) && (size_t)(splits < 1 ? 1 : splits) * M * Nn > slab_n) die(2, "slabs do not fit slab_n");
    char *A = static_cast<char *>(upload(j, "A", a_n * esz)), *B = static_cast<char *>(upload(j, "B", b_n * esz));
    Out C, S;
    if (!slabs_only || fold) C.alloc(sizeof(float) * (size_t)ldc * Nn);
    if (slab_n) S.alloc(sizeof(float) * slab_n);
    const unsigned sent = (unsigned)j.get("sent");
    for (int rep = 0; rep < (int)j.get("rep", 1); rep++) {
        if (C.base) C.fill(sent);
        if (S.base) S.fill(sent);
        if (pick) result(j, rep, "picked", splits);
        if (bf16) {
            lstmk::gemm_bf16(M, Nn, K, reinterpret_cast<unsigned short *>(A), lda, reinterpret_cast<unsigned short *>(B) + b_off, ldb,
                             C.payload<float>(), ldc, splits, S.payload<float>(), nullptr);
            launched("gemm_bf16");
        } else if (slabs_only) {
            const int used = lstmk::gemm_slabs(TA, TB, M, Nn, K, reinterpret_cast<float *>(A), lda, reinterpret_cast<float *>(B) + b_off,
                                               ldb, S.payload<float>(), splits, nullptr);
            launched("gemm_slabs");
            result(j, rep, "ret", used);
            if (fold) {
                if (used < 1 || (size_t)used * M * Nn > slab_n) die(2, "gemm_slabs returned a count outside its allocation");
                lstmk::gemm_fold(S.payload<float>(), used, M, Nn, C.payload<float>(), ldc, nullptr, 0);
                launched("gemm_fold");
            }
        } else {
            lstmk::gemm(TA, TB, M, Nn, K, reinterpret_cast<float *>(A), lda, reinterpret_cast<float *>(B) + b_off, ldb,
                        C.payload<float>(), ldc, splits, S.payload<float>(), nullptr);
            launched("gemm");
        }
        C.dump(j, "C", rep);
        S.dump(j, "S", rep);
    }
    C.release();
    S.release();
    if (A) HIP_OK(hipFree(A));
    if (B) HIP_OK(hipFree(B));
}

void run_fold(const Job &j) {
    const int splits = (int)j.get("splits"), M = (int)j.get("M"), Nn = (int)j.get("Nn"), ldc = (int)j.get("ldc", M);
    const size_t stride = (size_t)j.get("stride", 0), a_n = (size_t)j.get("a_n");
    const size_t step = stride ? stride : (size_t)M * Nn;
    if (splits < 1 || M < 1 || Nn < 1 || ldc < M || (size_t)(splits - 1) * step + (size_t)M * Nn > a_n) die(2, "bad shape");
    float *A = static_cast<float *>(upload(j, "A", a_n * sizeof(float)));
    Out C;
    C.alloc(sizeof(float) * (size_t)ldc * Nn);
    for (int rep = 0; rep < (int)j.get("rep", 1); rep++) {
        C.fill((unsigned)j.get("sent"));
        lstmk::gemm_fold(A, splits, M, Nn, C.payload<float>(), ldc, nullptr, stride);
        launched("gemm_fold");
        C.dump(j, "C", rep);
    }
    C.release();
    HIP_OK(hipFree(A));
}

void run_pack(const Job &j, bool transpose) {
    size_t a_n, out_n;
    int K = 0, R = 0, ld = 0, Kpad = 0;
    if (transpose) {
        K = (int)j.get("K"), R = (int)j.get("R"), ld = (int)j.get("ld"), Kpad = (int)j.get("Kpad");
        a_n = (size_t)j.get("a_n");
        out_n = (size_t)R * Kpad;
        if (K < 1 || R < 1 || ld < R || Kpad < K || (size_t)(K - 1) * ld + R > a_n) die(2, "bad shape");
    } else {
        a_n = out_n = (size_t)j.get("n");
        if (a_n < 1) die(2, "bad shape");
    }
    float *A = static_cast<float *>(upload(j, "A", a_n * sizeof(float)));
    Out C;
    C.alloc(sizeof(unsigned short) * out_n);
    for (int rep = 0; rep < (int)j.get("rep", 1); rep++) {
        C.fill((unsigned)j.get("sent"));
        if (transpose) lstmk::transpose_pack_bf16(A, K, R, ld, C.payload<unsigned short>(), Kpad, nullptr);
        else lstmk::pack_bf16(A, a_n, C.payload<unsigned short>(), nullptr);
        launched(transpose ? "transpose_pack_bf16" : "pack_bf16");
        C.dump(j, "C", rep);
    }
    C.release();
    HIP_OK(hipFree(A));
}

} // namespace

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: product_check <dir>\n");
        return 2;
    }
    g_dir = argv[1];
    g_where = "start";
    std::ifstream mf(g_dir + "/manifest.txt");
    if (!mf) die(2, "no manifest.txt");
    std::vector<Job> jobs;
    for (std::string line; std::getline(mf, line);) {
        std::istringstream is(line);
        Job j;
        if (!(is >> j.kind >> j.id)) continue;
        for (std::string tok; is >> tok;) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) die(2, "bad token " + tok);
            const std::string key = tok.substr(0, eq);
            j.kv[key] = strtoll(tok.c_str() + eq + 1, nullptr, key == "sent" ? 16 : 10);
        }
        jobs.push_back(j);
    }
    g_res = fopen((g_dir + "/results.txt").c_str(), "w");
    if (!g_res) die(2, "cannot write results.txt");
    int32_t n_cus = 0;
    if (lstm_hip_device_info(0, nullptr, &n_cus, nullptr) != 0) die(3, std::string("lstm_hip_device_info: ") + lstm_hip_last_error());
    HIP_OK(hipSetDevice(0));
    fprintf(g_res, "n_cus %d\n", (int)n_cus);
    for (const Job &j : jobs) {
        g_where = j.kind + " " + j.id;
        if (j.kind == "gemm") run_gemm(j, n_cus, false, false);
        else if (j.kind == "gemm_slabs") run_gemm(j, n_cus, true, false);
        else if (j.kind == "gemm_bf16") run_gemm(j, n_cus, false, true);
        else if (j.kind == "gemm_fold") run_fold(j);
        else if (j.kind == "transpose_pack_bf16") run_pack(j, true);
        else if (j.kind == "pack_bf16") run_pack(j, false);
        else if (j.kind == "pick_splits") {
            const bool bf16 = j.get("bf16");
            const int M = (int)j.get("M"), Nn = (int)j.get("Nn"), K = (int)j.get("K");
            for (int r = 0; r < 2; r++)
                result(j, 0, r ? "pick1" : "pick0",
                       bf16 ? lstmk::gemm_bf16_pick_splits(M, Nn, K)
                            : lstmk::gemm_pick_splits(j.get("TA"), j.get("TB"), M, Nn, K, n_cus));
        } else
            die(2, "unknown kind");
    }
    fclose(g_res);
    g_res = nullptr;
    printf("product_check: %zu jobs done\n", jobs.size());
    return 0;
}
