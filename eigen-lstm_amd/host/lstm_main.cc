// lstm_main.cc -- the C++ host program: the reference's main() (R/lstm.cc:50-361, batched per
// OV/lstm_eigen_opt/lstm.cc:47-413) with its compile-time constants turned into a command line and
// the loop body handed to the MI355X through the C ABI (include/lstm_hip.h).  No HIP, no torch here.
//
//   lstm <text file> <hidden> <seq> <batch> <lr> [options]        (the reference's knobs, R/lstm.cc:53-63)
//   lstm --data F --hidden N --seq S --batch B --lr LR [--epochs E] [--seed K] [--gpus G]
//        [--windows W] [--sample C] [--lr-warmup-windows X] [--save PREFIX] [--load PREFIX]
//        [--eval-file F] [--stride K] [--forget-bias V] [--test-percent F] [--test-every SEC] [--log PREFIX]
//        [--fast-math] [--step-kernels] [--stable-softmax] [--clip-norm X] [--optimizer adagrad|adam]
//        [--adam-betas B1,B2] [--adam-eps E] [--weight-decay W] [--average ema|uniform] [--average-decay D]
//        [--average-every K] [--average-start W] [--weight-drop R] [--weight-drop-seed K] [--test-streams K]
//        [--accumulate K] [--accumulate-mean]
//        [--test-warmup W] [--records] [--record-delim B] [--shuffle-seed K] [--label-smoothing E] [--teacher PREFIX]
//        [--distill-alpha A] [--distill-temperature T] [--teacher-bf16] [--train-after B] [--quiet]
//
// stdout follows the reference: "Read N bytes (file)" (R/lstm.cc:398), the carriage-return progress
// line (OV/lstm_eigen_opt/lstm.cc:320-331), the epoch summary (R/lstm.cc:284-291: GFLOP uses 2^30,
// loss divided by S*length) and the "Generated text |...|" block (R/lstm.cc:352-356).
//
// --gpus G forks one process per GPU before anything touches HIP; batch streams are sharded
// rank-major, the RCCL unique id travels over a pipe, and every window ends with one SUM
// all-reduce of the flat gradient block inside the library.
// --test-percent F holds out the last F% of the text (OV/lstm_eigen_class_CUDA/lstm.cc:76-86); --log PREFIX keeps the
// reference's results log (class_CUDA lstm.cc:196-236): every --test-every seconds and at each epoch end a row
// [index, seconds since the last test, train error, test error, GFlOP/s] is appended to PREFIX.txt, the parameters go
// to PREFIX_{W,U,Why,b,by}.txt and 5000 sampled bytes to PREFIX_sample.txt.  --save / --load also carry the Adagrad
// memory (PREFIX_mem_*.txt) and the stream cursors (PREFIX_cursors.txt), which the reference's checkpoints lack.
// --lr-warmup-windows X applies lr = 0 for the first X windows (the reference's GPU driver uses
// X = 50*S, OV/lstm_eigen_class_CUDA/lstm.cc:364-367; 0 = the root file's behaviour).
// --clip-norm X clips the global gradient norm to X before every Adagrad step (lstm_hip_set_grad_clip; inf = measure only)
// and adds one line per epoch report: mean and max pre-clip norm and the number of clipped windows.
// --optimizer adam trains with Adam / AdamW (lstm_hip_set_optimizer; --adam-betas, default 0.9,0.999, --adam-eps, default
// 1e-8, --weight-decay, default 0) instead of Adagrad.  Its checkpoints carry PREFIX_adam_{m,v}_*.txt and
// PREFIX_adam_steps.txt in place of the Adagrad memory; each rule loads only its own state.
// --average ema|uniform keeps a running average of the weights (lstm_hip_set_averaging): --average-decay D (ema only, default
// 0.999), --average-every K (every K-th update, default 1), --average-start W (averaging is turned on once W windows of
// this run are done, default 0; a resumed average goes on at once).  Every held-out test then adds one line with the
// averaged model's bits/char; --save also writes the average as a checkpoint of its own, PREFIX_avg_{W,U,b,Why,by}.txt (so
// --load PREFIX_avg works in lstm_generate and lstm_compress), and PREFIX_avg_state.txt (kind, decay, every, seen, n);
// --load PREFIX with the same --average kind resumes both, another kind or no --average ignores them.
// --accumulate K (K >= 2) makes one update per K training windows on the sum of their gradients, --accumulate-mean on their
// mean (lstm_hip_set_grad_accumulation); one GPU only; the epoch line is unchanged.  --save also writes what is pending as a
// checkpoint-shaped block PREFIX_accum_{W,U,b,Why,by}.txt and PREFIX_accum_state.txt (every, mean, pending); --load PREFIX
// with the same K and mean resumes them, another setting or no --accumulate ignores them.
// --weight-drop R (0 < R < 1) trains with DropConnect on the hidden-to-hidden matrix U, one mask per window
// (lstm_hip_set_weight_drop; --weight-drop-seed K, default 0, picks the mask sequence).  Held-out tests, samples and saved
// parameters are those of the unmasked model.  --save also writes PREFIX_weight_drop.txt (rate, seed, t); --load PREFIX with
// --weight-drop again resumes the mask index t (and the seed, unless --weight-drop-seed is given).
// --test-streams K (1..65536) runs the held-out tests through lstm_hip_eval_texts: the held-out text is cut into K streams
// that are evaluated side by side on the training window's forward path (eval_split.h), each piece after the first starting
// from a zero state --test-warmup W bytes (default 0) before its first scored byte.  Every byte but the first is still scored
// exactly once; K = 1 is the one stream of the default path.  Without the option the tests run lstm_hip_eval_bits as before.
// --records trains on separate texts, each from its zero state (lstm_hip_train_text_windows): --data is cut after every
// delimiter byte (--record-delim B, 0..255, default 10); the delimiter stays the last byte of its record, so the model learns
// where a record ends, which is what lstm_generate --stop-byte reads.  Every epoch trains on all records in a new order
// (--shuffle-seed K, default 0, seeds the shuffle), placed on the batch lanes by lstm_hip_text_plan; --windows caps the
// windows of an epoch.  The epoch line's bits/char are prequential: every byte scored under the parameters its window had
// before its update.  --lr-warmup-windows, --average, --weight-drop, --clip-norm, --save and --load work as without it (the
// saved cursors are those of the flat text, which --records does not move).  One GPU only; --stride and the last-step losses
// do not apply.
// --records --train-after B (B a byte value 0..255) is completion-only training (lstm_hip_set_train_texts_weighted): in every
// record the bytes up to and including the first byte B are context -- fed, never a target that counts -- and every byte after
// it is learned with weight 1; a record without B trains nothing.  The epoch line's prequential figure is then the weighted
// bits over the weight-1 target bytes ("trained bytes").  Needs --records.
#include "../../include/lstm_hip.h"

// --label-smoothing E (0 <= E < 1) trains toward (1 - E) onehot + E / 256; --teacher PREFIX distils from the checkpoint
// PREFIX_{W,U,b,Why,by}.txt (lstm_hip_set_soft_targets): the teacher's hidden size is read from the checkpoint, its handle is
// padded like the student's and takes the student's fast-math setting, --teacher-bf16 runs it on the bf16 recurrence (hidden
// sizes up to 1024); --distill-alpha A (default 0.5) weighs the hard-target term, --distill-temperature T (default 1) is the
// temperature of the teacher's term.  Reported losses stay hard-target bits; with a teacher the epoch line, the test line and
// the rows of --log carry the mean teacher KL in bits/char as one more field.  One GPU only, not with --records.
// referenced weakly: the program still links against a library without them and refuses --clip-norm / --optimizer adam there
#pragma weak lstm_hip_set_grad_clip
#pragma weak lstm_hip_get_grad_norms
#pragma weak lstm_hip_set_optimizer
#pragma weak lstm_hip_get_optimizer_steps
#pragma weak lstm_hip_set_optimizer_steps
// ... and --accumulate
#pragma weak lstm_hip_set_grad_accumulation
#pragma weak lstm_hip_get_grad_accumulation
#pragma weak lstm_hip_get_grad_accumulator
#pragma weak lstm_hip_set_grad_accumulator
// ... and --average
#pragma weak lstm_hip_set_averaging
#pragma weak lstm_hip_get_average
#pragma weak lstm_hip_set_average
#pragma weak lstm_hip_get_averaging_counts
#pragma weak lstm_hip_set_averaging_counts
#pragma weak lstm_hip_set_inference_source
// ... and --weight-drop
#pragma weak lstm_hip_set_weight_drop
#pragma weak lstm_hip_get_weight_drop
// ... and --test-streams
#pragma weak lstm_hip_eval_texts
// ... and --label-smoothing / --teacher
#pragma weak lstm_hip_set_soft_targets
#pragma weak lstm_hip_get_teacher_kl
// ... and --records
#pragma weak lstm_hip_text_plan
#pragma weak lstm_hip_set_train_texts
#pragma weak lstm_hip_get_train_texts
#pragma weak lstm_hip_train_text_windows
#pragma weak lstm_hip_get_train_texts_bits
// ... and --train-after
#pragma weak lstm_hip_set_train_texts_weighted
#include "eval_split.h"
#include "checkpoint.h"
#include "matrix_io.h"
#include "rng.h"

#include <errno.h>
#include <poll.h>
#include <signal.h>
#include <sys/time.h>
#include <sys/wait.h>
#include <unistd.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

namespace {

struct Options {
    std::string data = "alice29.txt"; // R/lstm.cc:63
    int N = 64, S = 3, B = 1;         // R/lstm.cc:53-57, OV/lstm_eigen_opt/lstm.cc:56
    double lr = 1e-1;                 // R/lstm.cc:59
    long epochs = 1000;               // R/lstm.cc:60
    uint32_t seed = 1;
    int gpus = 1;
    long windows = -1;        // cap on windows per epoch (-1: length - S, R/lstm.cc:151)
    int sample = 1000;        // R/lstm.cc:295
    long lr_warmup = 0;
    int stride = 1;           // bytes per window per stream (lstm_segment.cc: S/2)
    double forget_bias = 0.0; // OV/lstm_eigen_class_batch/lstm.cc:81 uses 1
    std::string save, load, eval_file, log;
    int test_percent = 0;    // last F%% of the text held out (OV/lstm_eigen_class_CUDA/lstm.cc:76-86 uses 1)
    double test_every = 0.0; // seconds between held-out tests + log rows (class_CUDA: 900; 0 = at epoch end only)
    unsigned flags = 0;
    bool quiet = false;
    bool last_step_loss = false; // report forward_loss of OV/lstm_eigen_class_CUDA/lstm.h:200-221 (last step, nats)
    bool last_step_bits = false; // ... or cuLSTM::calculate_loss, cu_lstm.h:203-215 (last step, bits)
    double clip_norm = 0.0;      // --clip-norm: 0 = off
    bool adam = false;           // --optimizer adam
    double beta1 = 0.9, beta2 = 0.999, adam_eps = 1e-8, weight_decay = 0.0;
    int avg_kind = LSTM_HIP_AVG_OFF; // --average
    double avg_decay = 0.0;          // --average-decay (ema: default 0.999)
    int avg_every = 1;               // --average-every
    long avg_start = 0;              // --average-start
    int accumulate = 1;              // --accumulate (1: off)
    bool accumulate_mean = false;    // --accumulate-mean
    double wd_rate = 0.0;            // --weight-drop: 0 = off
    uint64_t wd_seed = 0;            // --weight-drop-seed
    bool wd_seed_given = false;
    long test_streams = 0;           // --test-streams: 0 = lstm_hip_eval_bits
    long test_warmup = -1;           // --test-warmup (-1: not given)
    bool records = false;            // --records: train on the records of --data, each from its zero state
    int record_delim = 10;           // --record-delim
    uint32_t shuffle_seed = 0;       // --shuffle-seed
    int train_after = -1;            // --train-after: the separator byte of completion-only training, -1: every byte is learned
    double smoothing = 0.0;          // --label-smoothing
    std::string teacher;             // --teacher: checkpoint prefix (empty: none)
    double distill_alpha = 0.5;      // --distill-alpha
    double distill_tau = 1.0;        // --distill-temperature
    bool teacher_bf16 = false;       // --teacher-bf16
};

[[noreturn]] void die(const std::string &m) {
    fprintf(stderr, "lstm: %s\n", m.c_str());
    exit(2);
}
#define CK(call)                                                          \
    do {                                                                  \
        int rc_ = (call);                                                 \
        if (rc_ != 0) die(std::string(#call) + ": " + lstm_hip_last_error()); \
    } while (0)

double now() { // Timer, R/timer.h:21-41
    timeval tv;
    gettimeofday(&tv, nullptr);
    return tv.tv_sec + 1e-6 * tv.tv_usec;
}

// rawread, R/lstm.cc:382-420
std::vector<uint8_t> rawread(const std::string &filename) {
    std::vector<uint8_t> v;
    if (FILE *fp = fopen(filename.c_str(), "rb")) {
        char buf[1 << 16];
        while (size_t len = fread(buf, 1, sizeof(buf), fp)) v.insert(v.end(), buf, buf + len);
        fclose(fp);
        if (!v.empty()) printf("Read %zu bytes (%s)\n", v.size(), filename.c_str());
        else printf("Empty file! (%s)\n", filename.c_str());
    } else {
        printf("fopen error: (%s)\n", filename.c_str());
    }
    return v;
}

// count_flops, OV/lstm_eigen_class_CUDA/lstm.cc:722-747 (the model behind the reference's GFlOP/s)
double count_flops(double M, double N, double S, double B) {
    return (S - 1) * ((N * M * B * 2) + (N * 4 * N * B) + (N * 4 * B * 2) + (5 * N * 4 * B) + (6 * N * B) + (M * N * B * 2) +
                      (8 * N * B) + (N * B) + (M * B * N * 3) + (N * B * 6) + (N * M * B * 4) + (N * B * 8) +
                      (N * 4 * B * M * 3) + (N * 4 * B * N * 3) + (N * 4 * B) + (N * 4 * N * B * 2) + (N * B)) +
           8 * (M * N + M + N * 4 * N + N * 4 * M + N * 4);
}

// Parameters::save_to_disk / load_from_disk (checkpoint.h), ending the program on an error
void save_params(const std::string &prefix, const std::vector<float> &P, int N, int M, int digits = 6) {
    std::string err;
    if (!checkpoint::save_params(prefix, P, N, M, digits, &err)) die(err);
}
bool load_params(const std::string &prefix, std::vector<float> &P, int N, int M) {
    std::string err;
    const int rc = checkpoint::load_params(prefix, P, N, M, &err);
    if (rc < 0) die(err);
    return rc > 0;
}

// results log, OV/lstm_eigen_class_CUDA/lstm.cc:203-226 + io.h:16-30: the whole 5-column matrix is rewritten after
// every test, in the same layout
void write_results(const std::string &path, const std::vector<std::vector<double>> &rows) {
    printf("Saving a matrix to %s... \n", path.c_str());
    if (!matrix_io::write_matrix(path, rows.size(), rows.empty() ? 0 : rows[0].size(),
                                 [&](size_t r, size_t c) { return (float)rows[r][c]; }))
        printf("file save error: (%s)\n", path.c_str());
}
void save_cursors(const std::string &prefix, const std::vector<uint64_t> &pos) {
    std::ofstream f(prefix + "_cursors.txt");
    if (!f) die("cannot write " + prefix + "_cursors.txt");
    for (uint64_t v : pos) f << v << "\n";
}
bool load_cursors(const std::string &prefix, std::vector<uint64_t> &pos, size_t length, int S) {
    std::ifstream f(prefix + "_cursors.txt");
    if (!f) return false;
    std::vector<uint64_t> v;
    uint64_t x;
    while (f >> x) v.push_back(x);
    if (v.size() != pos.size()) return false; // written for another batch size: fall back to the spread start
    for (uint64_t c : v)
        if (c < (uint64_t)S || c >= length) return false;
    pos = v;
    return true;
}

double finite_number(const std::string &opt, const std::string &v) {
    char *end = nullptr;
    const double x = strtod(v.c_str(), &end);
    if (end == v.c_str() || *end != '\0' || !std::isfinite(x)) die(opt + " needs a finite number, got " + v);
    return x;
}

long whole_number(const std::string &opt, const std::string &v, long least) {
    char *end = nullptr;
    errno = 0;
    const long x = strtol(v.c_str(), &end, 10);
    if (end == v.c_str() || *end != '\0' || errno != 0 || x < least)
        die(opt + " needs a whole number >= " + std::to_string(least) + ", got " + v);
    return x;
}
const char *avg_name(int kind) { return kind == LSTM_HIP_AVG_EMA ? "ema" : "uniform"; }

Options parse(int argc, char **argv) {
    Options o;
    std::vector<std::string> pos;
    std::string adam_opt; // the last Adam option given (refused without --optimizer adam)
    std::string avg_opt;  // the last averaging option given (refused without --average)
    bool avg_decay_given = false;
    std::string records_opt; // the last option given that needs --records
    std::string teacher_opt; // the last option given that needs --teacher
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto val = [&]() -> std::string {
            if (i + 1 >= argc) die("missing value for " + a);
            return argv[++i];
        };
        if (a == "--data") o.data = val();
        else if (a == "--hidden") o.N = atoi(val().c_str());
        else if (a == "--seq") o.S = atoi(val().c_str());
        else if (a == "--batch") o.B = atoi(val().c_str());
        else if (a == "--lr") o.lr = atof(val().c_str());
        else if (a == "--epochs") o.epochs = atol(val().c_str());
        else if (a == "--seed") o.seed = (uint32_t)strtoul(val().c_str(), nullptr, 10);
        else if (a == "--gpus") o.gpus = atoi(val().c_str());
        else if (a == "--windows") o.windows = atol(val().c_str());
        else if (a == "--sample") o.sample = atoi(val().c_str());
        else if (a == "--lr-warmup-windows") o.lr_warmup = atol(val().c_str());
        else if (a == "--stride") o.stride = atoi(val().c_str());
        else if (a == "--forget-bias") o.forget_bias = atof(val().c_str());
        else if (a == "--save") o.save = val();
        else if (a == "--load") o.load = val();
        else if (a == "--eval-file") o.eval_file = val();
        else if (a == "--log") o.log = val();
        else if (a == "--test-percent") o.test_percent = atoi(val().c_str());
        else if (a == "--test-every") o.test_every = atof(val().c_str());
        else if (a == "--fast-math") o.flags |= LSTM_HIP_FAST_MATH;
        else if (a == "--step-kernels") o.flags |= LSTM_HIP_STEP_KERNELS;
        else if (a == "--stable-softmax") o.flags |= LSTM_HIP_STABLE_SOFTMAX;
        else if (a == "--clip-norm") {
            const std::string v = val();
            char *end = nullptr;
            o.clip_norm = strtod(v.c_str(), &end);
            if (end == v.c_str() || *end != '\0' || std::isnan(o.clip_norm) || o.clip_norm < 0.0)
                die("--clip-norm needs a number >= 0 (0: off, inf: measure the norm only), got " + v);
            if (o.clip_norm > 0.0 && (lstm_hip_set_grad_clip == nullptr || lstm_hip_get_grad_norms == nullptr))
                die("--clip-norm: the loaded liblstm_hip has no lstm_hip_set_grad_clip / lstm_hip_get_grad_norms");
        }
        else if (a == "--optimizer") {
            const std::string v = val();
            if (v != "adagrad" && v != "adam") die("--optimizer needs adagrad or adam, got " + v);
            o.adam = v == "adam";
        } else if (a == "--adam-betas") {
            const std::string v = val();
            const size_t comma = v.find(',');
            if (comma == std::string::npos) die("--adam-betas needs B1,B2, got " + v);
            o.beta1 = finite_number(a, v.substr(0, comma));
            o.beta2 = finite_number(a, v.substr(comma + 1));
            if (o.beta1 < 0.0 || o.beta1 >= 1.0 || o.beta2 < 0.0 || o.beta2 >= 1.0) die("--adam-betas needs 0 <= B1, B2 < 1, got " + v);
            adam_opt = a;
        } else if (a == "--adam-eps") {
            o.adam_eps = finite_number(a, val());
            if (o.adam_eps <= 0.0) die("--adam-eps needs a number > 0");
            adam_opt = a;
        } else if (a == "--weight-decay") {
            o.weight_decay = finite_number(a, val());
            if (o.weight_decay < 0.0) die("--weight-decay needs a number >= 0");
            adam_opt = a;
        }
        else if (a == "--average") {
            const std::string v = val();
            if (v != "ema" && v != "uniform") die("--average needs ema or uniform, got " + v);
            o.avg_kind = v == "ema" ? LSTM_HIP_AVG_EMA : LSTM_HIP_AVG_UNIFORM;
        } else if (a == "--average-decay") {
            o.avg_decay = finite_number(a, val());
            if (o.avg_decay < 0.0 || o.avg_decay >= 1.0) die("--average-decay needs 0 <= D < 1");
            avg_decay_given = true;
            avg_opt = a;
        } else if (a == "--average-every") {
            const long k = whole_number(a, val(), 1);
            if (k > 2147483647L) die("--average-every is too large");
            o.avg_every = (int)k;
            avg_opt = a;
        } else if (a == "--accumulate") {
            const long k = whole_number(a, val(), 2);
            if (k > 2147483647L) die("--accumulate is too large");
            o.accumulate = (int)k;
        } else if (a == "--accumulate-mean") {
            o.accumulate_mean = true;
        } else if (a == "--average-start") {
            o.avg_start = whole_number(a, val(), 0);
            avg_opt = a;
        }
        else if (a == "--weight-drop") {
            const std::string v = val();
            o.wd_rate = finite_number(a, v);
            if (!(o.wd_rate > 0.0 && o.wd_rate < 1.0)) die("--weight-drop needs a rate 0 < R < 1, got " + v);
        } else if (a == "--weight-drop-seed") {
            const std::string v = val();
            char *end = nullptr;
            errno = 0;
            const unsigned long long k = strtoull(v.c_str(), &end, 10);
            if (end == v.c_str() || *end != '\0' || errno != 0 || v[0] == '-') die(a + " needs a whole number >= 0, got " + v);
            o.wd_seed = (uint64_t)k;
            o.wd_seed_given = true;
        }
        else if (a == "--test-streams") {
            o.test_streams = whole_number(a, val(), 1);
            if (o.test_streams > 65536) die("--test-streams must be at most 65536");
        } else if (a == "--test-warmup") o.test_warmup = whole_number(a, val(), 0);
        else if (a == "--records") o.records = true;
        else if (a == "--record-delim") {
            const long b = whole_number(a, val(), 0);
            if (b > 255) die("--record-delim needs a byte value 0..255");
            o.record_delim = (int)b;
            records_opt = a;
        } else if (a == "--shuffle-seed") {
            const long k = whole_number(a, val(), 0);
            if (k > 4294967295L) die("--shuffle-seed is too large");
            o.shuffle_seed = (uint32_t)k;
            records_opt = a;
        } else if (a == "--train-after") {
            const long b = whole_number(a, val(), 0);
            if (b > 255) die("--train-after needs a byte value 0..255");
            o.train_after = (int)b;
            records_opt = a;
        }
        else if (a == "--label-smoothing") {
            const std::string v = val();
            o.smoothing = atof(v.c_str());
            if (!(o.smoothing >= 0.0 && o.smoothing < 1.0)) die("--label-smoothing needs 0 <= E < 1, got " + v);
        } else if (a == "--teacher") {
            o.teacher = val();
            if (o.teacher.empty()) die("--teacher needs a checkpoint prefix");
        } else if (a == "--distill-alpha") {
            const std::string v = val();
            o.distill_alpha = atof(v.c_str());
            if (!(o.distill_alpha >= 0.0 && o.distill_alpha <= 1.0)) die("--distill-alpha needs 0 <= A <= 1, got " + v);
            teacher_opt = a;
        } else if (a == "--distill-temperature") {
            const std::string v = val();
            o.distill_tau = atof(v.c_str());
            if (!(o.distill_tau > 0.0) || !std::isfinite(o.distill_tau)) die("--distill-temperature needs a finite T > 0, got " + v);
            teacher_opt = a;
        } else if (a == "--teacher-bf16") {
            o.teacher_bf16 = true;
            teacher_opt = a;
        }
        else if (a == "--last-step-loss") o.last_step_loss = true;
        else if (a == "--last-step-loss-bits") o.last_step_bits = true;
        else if (a == "--quiet") o.quiet = true;
        else if (a == "-h" || a == "--help") {
            printf("usage: lstm <text file> <hidden> <seq> <batch> <lr> [--epochs E --seed K --gpus G --windows W --sample C\n"
                   "            --lr-warmup-windows X --save PREFIX --load PREFIX --eval-file F --stride K --forget-bias V\n"
                   "            --test-percent F --test-every SEC --log PREFIX --last-step-loss --last-step-loss-bits --fast-math --step-kernels\n"
                   "            --stable-softmax --clip-norm X --optimizer adagrad|adam --adam-betas B1,B2 --adam-eps E\n"
                   "            --weight-decay W --average ema|uniform --average-decay D --average-every K --average-start W\n"
                   "            --weight-drop R --weight-drop-seed K --test-streams K --test-warmup W\n"
                   "            --records --record-delim B --shuffle-seed K --label-smoothing E --teacher PREFIX\n"
                   "            --distill-alpha A --distill-temperature T --teacher-bf16 --train-after B\n"
                   "            --accumulate K --accumulate-mean --quiet]\n");
            exit(0);
        } else if (a.rfind("--", 0) == 0) die("unknown option " + a);
        else pos.push_back(a);
    }
    if (!adam_opt.empty() && !o.adam) die(adam_opt + " needs --optimizer adam");
    if (o.adam && (lstm_hip_set_optimizer == nullptr || lstm_hip_get_optimizer_steps == nullptr ||
                   lstm_hip_set_optimizer_steps == nullptr))
        die("--optimizer adam: the loaded liblstm_hip has no lstm_hip_set_optimizer / lstm_hip_get_optimizer_steps / "
            "lstm_hip_set_optimizer_steps");
    if (!avg_opt.empty() && o.avg_kind == LSTM_HIP_AVG_OFF) die(avg_opt + " needs --average ema|uniform");
    if (avg_decay_given && o.avg_kind != LSTM_HIP_AVG_EMA) die("--average-decay needs --average ema");
    if (o.avg_kind == LSTM_HIP_AVG_EMA && !avg_decay_given) o.avg_decay = 0.999;
    if (o.avg_kind != LSTM_HIP_AVG_OFF &&
        (lstm_hip_set_averaging == nullptr || lstm_hip_get_average == nullptr || lstm_hip_set_average == nullptr ||
         lstm_hip_get_averaging_counts == nullptr || lstm_hip_set_averaging_counts == nullptr ||
         lstm_hip_set_inference_source == nullptr))
        die("--average: the loaded liblstm_hip has no lstm_hip_set_averaging / lstm_hip_get_average / lstm_hip_set_average / "
            "lstm_hip_get_averaging_counts / lstm_hip_set_averaging_counts / lstm_hip_set_inference_source");
    if (o.accumulate_mean && o.accumulate == 1) die("--accumulate-mean needs --accumulate K");
    if (o.accumulate > 1 && o.gpus != 1) die("--accumulate runs on one GPU");
    if (o.accumulate > 1 && (lstm_hip_set_grad_accumulation == nullptr || lstm_hip_get_grad_accumulation == nullptr ||
                             lstm_hip_get_grad_accumulator == nullptr || lstm_hip_set_grad_accumulator == nullptr))
        die("--accumulate: the loaded liblstm_hip has no lstm_hip_set_grad_accumulation / lstm_hip_get_grad_accumulation / "
            "lstm_hip_get_grad_accumulator / lstm_hip_set_grad_accumulator");
    if (o.wd_seed_given && !(o.wd_rate > 0.0)) die("--weight-drop-seed needs --weight-drop R");
    if (o.test_warmup >= 0 && o.test_streams == 0) die("--test-warmup needs --test-streams K");
    if (o.test_streams > 0 && lstm_hip_eval_texts == nullptr) die("--test-streams: the loaded liblstm_hip has no lstm_hip_eval_texts");
    if (o.wd_rate > 0.0 && (lstm_hip_set_weight_drop == nullptr || lstm_hip_get_weight_drop == nullptr))
        die("--weight-drop: the loaded liblstm_hip has no lstm_hip_set_weight_drop / lstm_hip_get_weight_drop");
    if (!records_opt.empty() && !o.records) die(records_opt + " needs --records");
    if (!teacher_opt.empty() && o.teacher.empty()) die(teacher_opt + " needs --teacher PREFIX");
    if ((o.smoothing > 0.0 || !o.teacher.empty()) && (lstm_hip_set_soft_targets == nullptr || lstm_hip_get_teacher_kl == nullptr))
        die("--label-smoothing / --teacher: the loaded liblstm_hip has no lstm_hip_set_soft_targets / lstm_hip_get_teacher_kl");
    if (!o.teacher.empty() && o.gpus != 1) die("--teacher runs on one GPU (each rank would need a teacher of its own)");
    if (!o.teacher.empty() && o.records) die("--teacher does not go with --records (the text windows train on hard targets)");
    if (o.smoothing > 0.0 && o.gpus != 1) die("--label-smoothing runs on one GPU");
    if (o.smoothing > 0.0 && o.records) die("--label-smoothing does not go with --records (the text windows train on hard targets)");
    if (o.records && (lstm_hip_text_plan == nullptr || lstm_hip_set_train_texts == nullptr || lstm_hip_get_train_texts == nullptr ||
                      lstm_hip_train_text_windows == nullptr || lstm_hip_get_train_texts_bits == nullptr))
        die("--records: the loaded liblstm_hip has no lstm_hip_text_plan / lstm_hip_set_train_texts / lstm_hip_get_train_texts / "
            "lstm_hip_train_text_windows / lstm_hip_get_train_texts_bits");
    if (o.train_after >= 0 && lstm_hip_set_train_texts_weighted == nullptr)
        die("--train-after: the loaded liblstm_hip has no lstm_hip_set_train_texts_weighted");
    if (o.records && o.gpus != 1) die("--records runs on one GPU (every rank would have to run the same number of windows)");
    if (o.records && o.stride != 1) die("--records does not take --stride (a text window always advances by seq - 1)");
    if (o.records && (o.last_step_loss || o.last_step_bits)) die("--records reports the all-steps loss only");
    if (pos.size() > 0) o.data = pos[0];
    if (pos.size() > 1) o.N = atoi(pos[1].c_str());
    if (pos.size() > 2) o.S = atoi(pos[2].c_str());
    if (pos.size() > 3) o.B = atoi(pos[3].c_str());
    if (pos.size() > 4) o.lr = atof(pos[4].c_str());
    if (o.gpus < 1 || o.B % o.gpus != 0) die("--batch must be a multiple of --gpus");
    if (o.test_percent < 0 || o.test_percent > 50) die("--test-percent must be 0..50");
    return o;
}

// one rank = one GPU.  `up`/`down` are pipes to/from the parent when gpus > 1.
int run_rank(const Options &o, int rank, int up, int down) {
    const int M = LSTM_HIP_VOCAB, N = o.N, S = o.S, Bl = o.B / o.gpus;
    const bool lead = rank == 0;
    std::vector<uint8_t> data = rawread(o.data);
    std::vector<uint8_t> testdata;
    if (o.test_percent > 0) { // first (100-F)% trains, the rest is held out (OV/lstm_eigen_class_CUDA/lstm.cc:76-86)
        const size_t percent_size = data.size() / 100, cut = (size_t)(100 - o.test_percent) * percent_size;
        testdata.assign(data.begin() + cut, data.end());
        data.resize(cut);
        if (lead) printf("Train set size: %zu, Test set size: %zu, Total: %zu\n", data.size(), testdata.size(), data.size() + testdata.size());
    }
    if (data.size() <= (size_t)S + 1) die("text too short");
    const size_t length = data.size();

    // --teacher: the checkpoint is read before anything touches the GPU, so a bad one is refused at once
    int Nt = 0;
    std::vector<float> Pt;
    if (!o.teacher.empty()) {
        if (!std::ifstream(o.teacher + "_W.txt").good()) die("--teacher: no checkpoint at " + o.teacher + "_W.txt");
        std::string err;
        Nt = checkpoint::hidden_size(o.teacher, M, &err);
        if (Nt < 1) die("--teacher: " + err);
        if (o.teacher_bf16 && (Nt + 127) / 128 * 128 > 1024)
            die("--teacher-bf16: the bf16 recurrence runs hidden sizes up to 1024; the teacher's is " + std::to_string(Nt));
        Pt.assign(lstm_hip_param_count(Nt, M), 0.0f);
        const int got = checkpoint::load_params(o.teacher, Pt, Nt, M, &err);
        if (got < 0) die("--teacher: " + err);
        if (got == 0) die("--teacher: the checkpoint " + o.teacher + "_{W,U,b,Why,by}.txt is not complete");
    }
    // the reference takes any hidden size (R/lstm.cc:53): the library pads it internally; every shape here stays N
    lstm_hip_config cfg{N, M, S, Bl, rank, o.flags | LSTM_HIP_PAD_HIDDEN};
    lstm_hip_t *h = nullptr;
    CK(lstm_hip_create(&cfg, &h));
    if (o.clip_norm > 0.0) CK(lstm_hip_set_grad_clip(h, o.clip_norm)); // (every rank: each steps on the same all-reduced norm)
    if (o.adam) // (every rank: the same step with the same t on the all-reduced gradient)
        CK(lstm_hip_set_optimizer(h, LSTM_HIP_OPT_ADAM, o.beta1, o.beta2, o.adam_eps, o.weight_decay));
    if (o.gpus > 1) {
        uint8_t id[LSTM_HIP_UNIQUE_ID_BYTES];
        if (lead) {
            CK(lstm_hip_comm_unique_id(id));
            if (write(up, id, sizeof(id)) != (ssize_t)sizeof(id)) die("pipe write");
        }
        if (read(down, id, sizeof(id)) != (ssize_t)sizeof(id)) die("pipe read");
        CK(lstm_hip_comm_init(h, id, o.gpus, rank));
        CK(lstm_hip_set_global_batch(h, o.B));
    }

    // init: W, U, Why ~ N(0, 0.01) in that order, b = by = 0 (R/lstm.cc:113-119); same on all ranks
    const size_t np = lstm_hip_param_count(N, M);
    std::vector<float> P(np, 0.0f);
    SeededRng rng(o.seed);
    {
        auto bl = checkpoint::blocks(N, M);
        rng.randn(P.data() + bl[0].off, 4 * N, M, 0.0, 0.01);
        rng.randn(P.data() + bl[1].off, 4 * N, N, 0.0, 0.01);
        rng.randn(P.data() + bl[3].off, M, N, 0.0, 0.01);
        for (int j = 0; j < N; j++) P[bl[2].off + 2 * N + j] = (float)o.forget_bias; // f-gate bias
    }
    if (!o.load.empty()) {
        if (load_params(o.load, P, N, M)) {
            if (lead) printf("Loaded parameters from %s_{W,U,Why,b,by}.txt\n", o.load.c_str());
        } else if (lead) printf("fopen error: (%s_W.txt) -- keeping the random initialisation\n", o.load.c_str());
    }
    CK(lstm_hip_set_params(h, 0, P.data()));
    // soft targets: the teacher is a second handle with the student's S and B, borrowed by the student for every window
    lstm_hip_t *teacher = nullptr;
    if (!o.teacher.empty()) {
        lstm_hip_config tcfg{Nt, M, S, Bl, rank,
                             (o.flags & LSTM_HIP_FAST_MATH) | LSTM_HIP_PAD_HIDDEN | (o.teacher_bf16 ? LSTM_HIP_BF16_RECURRENCE : 0u)};
        CK(lstm_hip_create(&tcfg, &teacher));
        CK(lstm_hip_set_params(teacher, 0, Pt.data()));
        printf("Teacher: hidden %d from %s_{W,U,Why,b,by}.txt%s, alpha %g, temperature %g\n", Nt, o.teacher.c_str(),
               o.teacher_bf16 ? " (bf16 recurrence)" : "", o.distill_alpha, o.distill_tau);
    }
    if (teacher || o.smoothing > 0.0) {
        const lstm_hip_soft_targets st{(uint32_t)sizeof(lstm_hip_soft_targets), teacher ? o.distill_alpha : 1.0,
                                       teacher ? o.distill_tau : 1.0, o.smoothing};
        CK(lstm_hip_set_soft_targets(h, teacher, &st));
    }
    double kl_sum = 0.0;  // teacher KL of the epoch so far, summed over its windows
    long kl_windows = 0;
    auto kl_per_char = [&]() { return kl_windows > 0 ? kl_sum / ((double)(S - 1) * (double)kl_windows) : 0.0; };
    if (!o.load.empty() && o.adam) { // resume: Adam's moments and step count, when the checkpoint has them (never _mem_*)
        std::vector<float> m(np, 0.0f), v(np, 0.0f);
        long long t = -1;
        std::ifstream steps(o.load + "_adam_steps.txt");
        if (steps && (steps >> t) && t >= 0 && load_params(o.load + "_adam_m", m, N, M) && load_params(o.load + "_adam_v", v, N, M)) {
            CK(lstm_hip_set_params(h, 2, m.data()));
            CK(lstm_hip_set_params(h, 3, v.data()));
            CK(lstm_hip_set_optimizer_steps(h, t));
            if (lead) printf("Loaded Adam state (t = %lld) from %s_adam_{m,v}_{W,U,Why,b,by}.txt\n", t, o.load.c_str());
        }
    } else if (!o.load.empty()) { // resume: Adagrad memory, when the checkpoint has it (never _adam_*)
        std::vector<float> mem(np, 0.0f);
        if (std::ifstream(o.load + "_mem_W.txt").good() && load_params(o.load + "_mem", mem, N, M)) {
            CK(lstm_hip_set_params(h, 2, mem.data()));
            if (lead) printf("Loaded Adagrad memory from %s_mem_{W,U,Why,b,by}.txt\n", o.load.c_str());
        }
    }
    // the running average: resumed from a checkpoint of the same kind (on at once), else turned on after --average-start windows
    bool avg_on = false;
    if (o.avg_kind != LSTM_HIP_AVG_OFF && !o.load.empty()) {
        std::ifstream f(o.load + "_avg_state.txt");
        std::string key, kind;
        double decay = 0.0;
        long long every = 0, seen = -1, n = -1;
        if (f && (f >> key >> kind >> key >> decay >> key >> every >> key >> seen >> key >> n) && kind == avg_name(o.avg_kind) &&
            n >= 0 && n <= seen) {
            std::vector<float> a(np, 0.0f);
            if (n == 0 || load_params(o.load + "_avg", a, N, M)) {
                CK(lstm_hip_set_averaging(h, o.avg_kind, o.avg_decay, o.avg_every));
                if (n > 0) CK(lstm_hip_set_average(h, a.data()));
                CK(lstm_hip_set_averaging_counts(h, seen, n));
                avg_on = true;
                if (lead) printf("Loaded the %s average (seen = %lld, n = %lld) from %s_avg_{W,U,Why,b,by}.txt\n", kind.c_str(), seen, n, o.load.c_str());
            }
        }
    }
    if (o.accumulate > 1) { // gradient accumulation; what a checkpoint of the same setting had pending is resumed
        CK(lstm_hip_set_grad_accumulation(h, o.accumulate, o.accumulate_mean ? 1 : 0));
        if (!o.load.empty()) {
            std::ifstream f(o.load + "_accum_state.txt");
            std::string key;
            long long every = 0, mean = -1, pending = -1;
            std::vector<float> a(np, 0.0f);
            if (f && (f >> key >> every >> key >> mean >> key >> pending) && every == o.accumulate &&
                mean == (o.accumulate_mean ? 1 : 0) && pending > 0 && pending < every && load_params(o.load + "_accum", a, N, M)) {
                CK(lstm_hip_set_grad_accumulator(h, a.data(), (int32_t)pending));
                if (lead) printf("Loaded the gradient accumulator (every = %lld, pending = %lld) from %s_accum_{W,U,Why,b,by}.txt\n", every, pending, o.load.c_str());
            }
        }
    }
    if (o.wd_rate > 0.0) { // weight drop (every rank: the same three numbers); a checkpoint's mask index is resumed
        uint64_t seed = o.wd_seed, t = 0;
        if (!o.load.empty()) {
            std::ifstream f(o.load + "_weight_drop.txt");
            std::string key;
            double rate = 0.0;
            unsigned long long fseed = 0, ft = 0;
            if (f && (f >> key >> rate >> key >> fseed >> key >> ft)) {
                if (!o.wd_seed_given) seed = fseed;
                t = ft;
                if (lead) printf("Loaded weight drop (seed = %llu, t = %llu) from %s_weight_drop.txt\n", (unsigned long long)seed, ft, o.load.c_str());
            }
        }
        CK(lstm_hip_set_weight_drop(h, o.wd_rate, seed, t));
    }
    CK(lstm_hip_set_text(h, data.data(), length));

    // cursors: deterministic stand-in for rand() % (length - S) + S (OV/lstm_eigen_opt/lstm.cc:140-144)
    std::vector<uint64_t> start_all(o.B), pos(Bl); // start_all: every stream of the global batch, rank-major
    for (int b = 0; b < o.B; b++) start_all[b] = (uint64_t)S + ((uint64_t)b * (length - S)) / (uint64_t)o.B;
    if (!o.load.empty() && load_cursors(o.load, start_all, length, S) && lead) // resume: the streams' positions
        printf("Loaded stream cursors from %s_cursors.txt\n", o.load.c_str());
    std::copy(start_all.begin() + (size_t)rank * Bl, start_all.begin() + (size_t)(rank + 1) * Bl, pos.begin());
    CK(lstm_hip_set_cursors(h, pos.data()));
    CK(lstm_hip_reset_window(h));
    if (o.last_step_loss) CK(lstm_hip_set_loss_mode(h, LSTM_HIP_LOSS_LAST_STEP_NATS));
    if (o.last_step_bits) CK(lstm_hip_set_loss_mode(h, LSTM_HIP_LOSS_LAST_STEP_BITS));
    if (o.stride > 1) CK(lstm_hip_set_stride(h, o.stride, o.stride - 1)); // segment variant: carry from column seg-1

    const double flops_per_iteration = count_flops(M, N, S, o.B);

    // held-out text: --eval-file wins over the --test-percent split
    std::vector<uint8_t> evaldata = (lead && !o.eval_file.empty()) ? rawread(o.eval_file) : testdata;
    const std::string evalname = !o.eval_file.empty() ? o.eval_file : "last " + std::to_string(o.test_percent) + "% of " + o.data;
    std::vector<std::vector<double>> results;
    double last_test = now();
    SeededRng log_rng(o.seed + 7919u); // sampling for the log must not disturb the training stream
    EvalSplit split; // --test-streams: the held-out text cut once
    if (o.test_streams > 0 && evaldata.size() > 1)
        split.add(evaldata.data(), evaldata.size(), (size_t)o.test_streams, (size_t)std::max(o.test_warmup, 0L));
    auto heldout = [&](double *bits_per_char) { // bits/char of the held-out text under the current inference source
        if (o.test_streams == 0) return lstm_hip_eval_bits(h, evaldata.data(), evaldata.size(), bits_per_char);
        std::vector<double> bits;
        if (int rc = split.run(h, bits)) return rc;
        *bits_per_char = bits[0] / (double)(evaldata.size() - 1);
        return 0;
    };
    // test(p, testdata) + results row + checkpoint + sample file, OV/lstm_eigen_class_CUDA/lstm.cc:186-236 (lead rank only:
    // the evaluator and the sampler are local to one handle, the other ranks wait at the next all-reduce)
    auto test_and_log = [&](double train_error, double gflops) {
        const double test_time = now() - last_test;
        double test_error = NAN;
        if (evaldata.size() > 1) CK(heldout(&test_error));
        if (teacher) printf("\nTrain error: %g, Test error: %g, Teacher KL: %g\n", train_error, test_error, kl_per_char());
        else
        printf("\nTrain error: %g, Test error: %g\n", train_error, test_error);
        if (evaldata.size() > 1) printf("Test error: %.5f bits/char (%s)\n", test_error, evalname.c_str());
        if (avg_on && evaldata.size() > 1) { // the same text through the averaged model (the log keeps its columns)
            int64_t seen = 0, n = 0;
            CK(lstm_hip_get_averaging_counts(h, &seen, &n));
            if (n >= 1) {
                double avg_error = NAN;
                CK(lstm_hip_set_inference_source(h, LSTM_HIP_SRC_AVERAGE));
                CK(heldout(&avg_error));
                CK(lstm_hip_set_inference_source(h, LSTM_HIP_SRC_PARAMS));
                printf("Test error of the %s average (n = %lld): %.5f bits/char (%s)\n", avg_name(o.avg_kind), (long long)n, avg_error,
                       evalname.c_str());
            }
        }
        if (!o.log.empty()) {
            results.push_back({(double)results.size(), test_time, train_error, test_error, gflops});
            if (teacher) {
                results.back().push_back(kl_per_char());
                printf("%6g %6g %6g %6g %6g %6g\n\n", results.back()[0], test_time, train_error, test_error, gflops, results.back()[5]);
            } else
            printf("%6g %6g %6g %6g %6g\n\n", results.back()[0], test_time, train_error, test_error, gflops);
            write_results(o.log + ".txt", results);
            CK(lstm_hip_get_params(h, 0, P.data()));
            save_params(o.log, P, N, M);
            const int n = 5000; // class_CUDA lstm.cc:229
            std::vector<float> h0(N), c0(N);
            log_rng.randn(h0.data(), N, 1, 0.0, 0.1);
            log_rng.randn(c0.data(), N, 1, 0.0, 0.1);
            std::vector<double> u(n);
            for (double &x : u) x = log_rng.uniform();
            std::vector<uint8_t> text(n);
            CK(lstm_hip_sample(h, h0.data(), c0.data(), u.data(), n, text.data()));
            std::ofstream f(o.log + "_sample.txt", std::ios::out | std::ios::binary);
            f.write(reinterpret_cast<const char *>(text.data()), n);
        }
        last_test = now();
    };
    long windows_per_epoch = (o.windows > 0) ? o.windows : (long)((length - S + o.stride - 1) / o.stride);
    long done_windows = 0, flat_windows = 0; // updates of this run / those of them that moved the flat text's cursors
    // --records: the training text cut after every delimiter byte; a last record may lack its delimiter
    std::vector<uint64_t> rec_begin;
    if (o.records) {
        if (Bl > 4096) die("--records takes at most 4096 batch lanes");
        rec_begin.push_back(0);
        for (size_t i = 0; i + 1 < length; i++)
            if (data[i] == (uint8_t)o.record_delim) rec_begin.push_back(i + 1);
        if (rec_begin.size() > 2147483647u) die("--records: too many records");
        printf("Records: %zu, cut after byte %d\n", rec_begin.size(), o.record_delim);
    }
    const size_t n_rec = rec_begin.size();
    rec_begin.push_back(length);
    SeededRng shuffle_rng(o.shuffle_seed);
    std::vector<uint32_t> order(n_rec);
    for (size_t r = 0; r < n_rec; r++) order[r] = (uint32_t)r;
    std::vector<uint8_t> rec_text(o.records ? length : 0);
    std::vector<uint64_t> rec_off(n_rec + 1, 0);
    std::vector<int64_t> rec_first(n_rec);
    // --train-after: a weight per byte of rec_text, and per record the offset of its first separator (its length: none)
    std::vector<float> rec_weight(o.train_after >= 0 ? length : 0);
    std::vector<uint64_t> rec_sep(o.train_after >= 0 ? n_rec : 0);
    // scored bytes (steps) in the first w windows of the epoch's plan
    auto steps_in = [&](long w) {
        double steps = 0.0;
        for (size_t r = 0; r < n_rec; r++) {
            const uint64_t len = rec_off[r + 1] - rec_off[r];
            if (rec_first[r] < 0 || len < 2) continue;
            const int64_t room = ((int64_t)w - rec_first[r]) * (S - 1);
            steps += (double)std::min<int64_t>(std::max<int64_t>(room, 0), (int64_t)len - 1);
        }
        return steps;
    };
    // ... and the weight-1 targets among them (--train-after): the scored bytes behind the record's first separator
    auto trained_in = [&](long w) {
        double trained = 0.0;
        for (size_t r = 0; r < n_rec; r++) {
            const uint64_t len = rec_off[r + 1] - rec_off[r];
            if (rec_first[r] < 0 || len < 2) continue;
            const int64_t room = ((int64_t)w - rec_first[r]) * (S - 1);
            const int64_t scored = std::min<int64_t>(std::max<int64_t>(room, 0), (int64_t)len - 1); // targets: bytes 1 .. scored
            trained += (double)std::max<int64_t>(scored - (int64_t)rec_sep[r], 0);
        }
        return trained;
    };
    auto chars_in = [&](long w) { return o.train_after >= 0 ? trained_in(w) : steps_in(w); };
    std::vector<float> hs((size_t)N * o.B), cs((size_t)N * o.B);
    std::vector<double> losses, norms, kls;

    for (long e = 0; e < o.epochs; e++) {
        // epoch start: h[t], c[t] ~ N(0, 0.1) for every t (OV/lstm_eigen_opt/lstm.cc:176-181); drawn for
        // the GLOBAL batch so every rank consumes the same stream, each keeps its own columns
        for (int t = 0; t < S; t++) {
            rng.randn(hs.data(), N, o.B, 0.0, 0.1);
            rng.randn(cs.data(), N, o.B, 0.0, 0.1);
            CK(lstm_hip_set_state(h, t, hs.data() + (size_t)rank * Bl * N, cs.data() + (size_t)rank * Bl * N));
        }
        if (o.records) { // this epoch's order (Fisher-Yates on the shuffle's own generator), its texts and its plan
            for (size_t i = n_rec; i > 1; i--) std::swap(order[i - 1], order[shuffle_rng.u32() % i]);
            for (size_t r = 0; r < n_rec; r++) {
                const uint64_t a = rec_begin[order[r]], b = rec_begin[order[r] + 1];
                std::copy(data.begin() + a, data.begin() + b, rec_text.begin() + rec_off[r]);
                rec_off[r + 1] = rec_off[r] + (b - a);
            }
            if (o.train_after >= 0) { // (the weights of lstm_hip.completion_weights: 1 behind the record's first separator)
                for (size_t r = 0; r < n_rec; r++) {
                    const uint8_t *b = rec_text.data() + rec_off[r], *e = rec_text.data() + rec_off[r + 1];
                    rec_sep[r] = (uint64_t)(std::find(b, e, (uint8_t)o.train_after) - b);
                    for (uint64_t i = 0; i < (uint64_t)(e - b); i++) rec_weight[rec_off[r] + i] = i > rec_sep[r] ? 1.0f : 0.0f;
                }
                CK(lstm_hip_set_train_texts_weighted(h, (int32_t)n_rec, rec_text.data(), rec_off.data(), rec_weight.data()));
            } else
            CK(lstm_hip_set_train_texts(h, (int32_t)n_rec, rec_text.data(), rec_off.data()));
            int64_t plan_windows = 0;
            CK(lstm_hip_get_train_texts(h, &plan_windows, nullptr));
            if (plan_windows < 1) die("--records: no record has two bytes");
            if (lstm_hip_text_plan(S - 1, Bl, (int32_t)n_rec, rec_off.data(), nullptr, rec_first.data()) != plan_windows)
                die("--records: the plan of lstm_hip_text_plan is not the handle's");
            windows_per_epoch = o.windows > 0 ? (long)std::min<int64_t>(o.windows, plan_windows) : (long)plan_windows;
        }
        double epoch_loss = 0.0;
        kl_sum = 0.0, kl_windows = 0;
        long nan_windows = 0;
        double norm_sum = 0.0, norm_max = 0.0;
        long clipped = 0, norm_count = 0;
        const double t0 = now();
        double tf = t0;
        for (long i = 0; i < windows_per_epoch;) {
            long chunk = std::min<long>(100, windows_per_epoch - i); // progress every 100 iterations (opt:320)
            double lr = o.lr;
            if (done_windows < o.lr_warmup) {
                lr = 0.0;
                chunk = std::min<long>(chunk, o.lr_warmup - done_windows);
            }
            if (o.avg_kind != LSTM_HIP_AVG_OFF && !avg_on) { // (every rank: the same rule on the same parameters)
                if (done_windows >= o.avg_start) {
                    CK(lstm_hip_set_averaging(h, o.avg_kind, o.avg_decay, o.avg_every));
                    avg_on = true;
                } else
                    chunk = std::min<long>(chunk, o.avg_start - done_windows);
            }
            losses.resize(chunk);
            long updates = chunk; // (one norm per update: under --accumulate one per full cycle)
            if (o.accumulate > 1) {
                int32_t every = 1, mean = 0, pending = 0;
                CK(lstm_hip_get_grad_accumulation(h, &every, &mean, &pending));
                updates = (pending + chunk) / every;
            }
            if (o.records) CK(lstm_hip_train_text_windows(h, chunk, lr, losses.data(), nullptr));
            else CK(lstm_hip_train_windows(h, chunk, lr, losses.data(), nullptr));
            if (!o.records) flat_windows += chunk;
            if (o.clip_norm > 0.0) {
                norms.resize(updates);
                CK(lstm_hip_get_grad_norms(h, norms.data(), updates));
                for (double v : norms) { // (the rule of lstm_hip_set_grad_clip: scaled where the norm is finite and the float
                                         // coefficient below 1)
                    norm_sum += v;
                    norm_max = std::max(norm_max, v);
                    norm_count++;
                    if (std::isfinite(v) && (float)(o.clip_norm / (v + 1e-6)) < 1.0f) clipped++;
                }
            }
            if (teacher) {
                kls.resize(chunk);
                CK(lstm_hip_get_teacher_kl(h, kls.data(), chunk));
                for (double v : kls)
                    if (!std::isnan(v)) kl_sum += v, kl_windows++;
            }
            for (double v : losses) {
                if (!std::isnan(v)) epoch_loss += v; // NaN guard as OV/lstm_eigen_class_CUDA/lstm.cc:325-326
                else nan_windows++;
            }
            i += chunk;
            done_windows += chunk;
            // mid-epoch report (class_CUDA lstm.cc:186-188).  With several ranks the lead only has its own share of the loss
            // (local surprisal sum / GLOBAL batch); the ranks exchange sums once per epoch, not here, so the running figure is
            // the lead's share scaled by the rank count -- an estimate over its streams, labelled as what the reference prints
            if (lead && o.test_every > 0 && now() - last_test > o.test_every)
                test_and_log(o.records ? epoch_loss * (double)o.B / std::max(chars_in(i), 1.0)
                                       : epoch_loss * (double)o.gpus / ((double)S * (double)i),
                             (i * flops_per_iteration / std::pow(2.0, 30)) / (now() - t0));
            if (lead && !o.quiet) {
                const double t1 = now();
                printf("%9.2f%% %9.2f GFlOP/s\r", o.records ? 100.0 * (double)i / (double)windows_per_epoch : 100.0 * (double)(i + S) / (double)length,
                       (chunk * flops_per_iteration / std::pow(2.0, 30)) / (t1 - tf));
                fflush(stdout);
                tf = t1;
            }
        }
        const double epoch_time = now() - t0;
        if (o.gpus > 1) { // sum the ranks' partial losses (each already divided by the global batch)
            if (write(up, &epoch_loss, sizeof(double)) != (ssize_t)sizeof(double)) die("pipe write");
            if (read(down, &epoch_loss, sizeof(double)) != (ssize_t)sizeof(double)) die("pipe read");
        }
        if (lead) {
            const double rows = (double)(S - 1) * o.B * windows_per_epoch;
            const double chars = o.records ? steps_in(windows_per_epoch) : rows; // (a text window's rows are not all filled)
            // R/lstm.cc:290: loss/(S*length); --records: the prequential bits of the epoch over its scored bytes
            // (--train-after: the weighted bits over the weight-1 target bytes)
            const double trained = o.records ? chars_in(windows_per_epoch) : 0.0;
            const double train_bits = o.records ? epoch_loss * (double)o.B / std::max(trained, 1.0)
                                                : epoch_loss / ((double)S * (double)(windows_per_epoch + S));
            printf("\n====================================================================================\n");
            if (teacher)
                printf("Epoch %ld/%ld, t = %.3f s, est GFLOP/s = %.3f, avg loss = %.3f bits/char, teacher KL = %.5f bits/char\n", e + 1,
                       o.epochs, epoch_time, (flops_per_iteration * windows_per_epoch / std::pow(2.0, 30)) / epoch_time, train_bits,
                       kl_per_char());
            else
            printf("Epoch %ld/%ld, t = %.3f s, est GFLOP/s = %.3f, avg loss = %.3f bits/char\n", e + 1, o.epochs, epoch_time,
                   (flops_per_iteration * windows_per_epoch / std::pow(2.0, 30)) / epoch_time,
                   train_bits);
            if (o.records)
                printf("records: %zu texts in %ld windows, %.1f%% of the rows filled, %.5f prequential bits/char over %.0f %sbytes\n", n_rec,
                       windows_per_epoch, 100.0 * chars / rows, train_bits, trained, o.train_after >= 0 ? "trained " : "");
            printf("chars/s through fwd+BPTT = %.1f (%ld windows, %d GPU%s)\n", chars / epoch_time, windows_per_epoch, o.gpus,
                   o.gpus > 1 ? "s" : "");
            if (o.clip_norm > 0.0)
                printf("grad norm: mean %.4g, max %.4g, clipped %ld of %ld windows (--clip-norm %g)\n",
                       norm_count ? norm_sum / (double)norm_count : 0.0, norm_max, clipped, norm_count, o.clip_norm);
            if (nan_windows > 0) // the reference skips NaN losses silently; the unshifted softmax (R/lstm.cc:199) overflows when lr is too large
                printf("!!!! %ld of %ld windows had a NaN loss (skipped in the average): lower --lr or use --lr-warmup-windows%s\n",
                       nan_windows, windows_per_epoch,
                       (o.flags & LSTM_HIP_STABLE_SOFTMAX) ? "" : ". --stable-softmax keeps large logits finite.");
            if (evaldata.size() > 1 || !o.log.empty())
                test_and_log(train_bits,
                             (flops_per_iteration * windows_per_epoch / std::pow(2.0, 30)) / epoch_time);
            if (o.sample > 0) { // R/lstm.cc:293-356
                std::vector<float> h0(N), c0(N);
                rng.randn(h0.data(), N, 1, 0.0, 0.1);
                rng.randn(c0.data(), N, 1, 0.0, 0.1);
                std::vector<double> u(o.sample);
                for (double &x : u) x = rng.uniform();
                std::vector<uint8_t> text(o.sample);
                CK(lstm_hip_sample(h, h0.data(), c0.data(), u.data(), o.sample, text.data()));
                printf("\n\n************ Generated text |");
                fwrite(text.data(), 1, text.size(), stdout);
                printf("| Generated text END ************\n");
            } else { // keep the RNG stream aligned across ranks
            }
            if (!o.save.empty()) {
                CK(lstm_hip_get_params(h, 0, P.data()));
                save_params(o.save, P, N, M);
                std::vector<float> mem(np);
                CK(lstm_hip_get_params(h, 2, mem.data()));
                if (o.adam) { // (no _mem_* files: an Adagrad run would take m, which can be negative, as its memory)
                    save_params(o.save + "_adam_m", mem, N, M, 9);
                    CK(lstm_hip_get_params(h, 3, mem.data()));
                    save_params(o.save + "_adam_v", mem, N, M, 9);
                    int64_t t = 0;
                    CK(lstm_hip_get_optimizer_steps(h, &t));
                    std::ofstream f(o.save + "_adam_steps.txt");
                    if (!(f << (long long)t << "\n")) die("cannot write " + o.save + "_adam_steps.txt");
                } else
                    save_params(o.save + "_mem", mem, N, M, 9);
                if (avg_on) { // the average as a parameter checkpoint of its own (once it holds one) and its state
                    int64_t seen = 0, n = 0;
                    CK(lstm_hip_get_averaging_counts(h, &seen, &n));
                    if (n >= 1) {
                        CK(lstm_hip_get_average(h, mem.data()));
                        save_params(o.save + "_avg", mem, N, M, 9);
                    }
                    std::ofstream f(o.save + "_avg_state.txt");
                    char decay[40];
                    snprintf(decay, sizeof(decay), "%.17g", o.avg_decay);
                    if (!(f << "kind " << avg_name(o.avg_kind) << "\ndecay " << decay << "\nevery " << o.avg_every << "\nseen "
                            << (long long)seen << "\nn " << (long long)n << "\n"))
                        die("cannot write " + o.save + "_avg_state.txt");
                    printf("Saved the %s average (seen = %lld, n = %lld) to %s_avg_{W,U,Why,b,by}.txt\n", avg_name(o.avg_kind),
                           (long long)seen, (long long)n, o.save.c_str());
                }
                if (o.accumulate > 1) { // the pending sum as a checkpoint-shaped block (zeros when nothing is pending) and its state
                    int32_t every = 1, mean = 0, pending = 0;
                    CK(lstm_hip_get_grad_accumulation(h, &every, &mean, &pending));
                    CK(lstm_hip_get_grad_accumulator(h, mem.data()));
                    save_params(o.save + "_accum", mem, N, M, 9);
                    std::ofstream f(o.save + "_accum_state.txt");
                    if (!(f << "every " << every << "\nmean " << mean << "\npending " << pending << "\n"))
                        die("cannot write " + o.save + "_accum_state.txt");
                    printf("Saved the gradient accumulator (every = %d, mean = %d, pending = %d) to %s_accum_{W,U,Why,b,by}.txt\n", every,
                           mean, pending, o.save.c_str());
                }
                if (o.wd_rate > 0.0) { // weight drop: the three numbers a resumed run sets
                    double rate = 0.0;
                    uint64_t seed = 0, t = 0;
                    CK(lstm_hip_get_weight_drop(h, &rate, &seed, &t));
                    std::ofstream f(o.save + "_weight_drop.txt");
                    char r[40];
                    snprintf(r, sizeof(r), "%.17g", rate);
                    if (!(f << "rate " << r << "\nseed " << (unsigned long long)seed << "\nt " << (unsigned long long)t << "\n"))
                        die("cannot write " + o.save + "_weight_drop.txt");
                    printf("Saved weight drop (rate = %s, seed = %llu, t = %llu) to %s_weight_drop.txt\n", r, (unsigned long long)seed,
                           (unsigned long long)t, o.save.c_str());
                }
                std::vector<uint64_t> all(o.B); // every stream has advanced by the same number of bytes
                const uint64_t span = (uint64_t)(length - S), adv = (uint64_t)flat_windows * (uint64_t)o.stride;
                for (int b = 0; b < o.B; b++) all[b] = (uint64_t)S + ((start_all[b] - S) + adv) % span;
                std::vector<uint64_t> mine(Bl);
                CK(lstm_hip_get_cursors(h, mine.data()));
                for (int b = 0; b < Bl; b++)
                    if (mine[b] != all[(size_t)rank * Bl + b]) die("cursor bookkeeping out of step with the library");
                save_cursors(o.save, all);
                printf("Saved parameters to %s_{W,U,Why,b,by}.txt (+ %s, _cursors)\n", o.save.c_str(),
                       o.adam ? "_adam_m_*, _adam_v_*, _adam_steps" : "_mem_*");
            }
            fflush(stdout);
        }
        if (!lead && o.sample > 0) { // non-lead ranks consume the same draws so later epochs stay in step
            std::vector<float> tmp(N);
            rng.randn(tmp.data(), N, 1, 0.0, 0.1);
            rng.randn(tmp.data(), N, 1, 0.0, 0.1);
            for (int k = 0; k < o.sample; k++) (void)rng.uniform();
        }
    }
    CK(lstm_hip_destroy(h)); // (releases the teacher)
    if (teacher) CK(lstm_hip_destroy(teacher));
    return 0;
}

} // namespace

int main(int argc, char **argv) {
    Options o = parse(argc, argv);
    if (o.gpus == 1) return run_rank(o, 0, -1, -1);

    // one process per GPU, forked before any HIP call
    std::vector<int> up_r(o.gpus), down_w(o.gpus);
    std::vector<pid_t> kids(o.gpus);
    for (int r = 0; r < o.gpus; r++) {
        int up[2], down[2];
        if (pipe(up) != 0 || pipe(down) != 0) die("pipe");
        setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0", 0); // RCCL across processes needs dmabuf IPC on this driver
        pid_t pid = fork();
        if (pid < 0) die("fork");
        if (pid == 0) {
            close(up[0]);
            close(down[1]);
            if (r != 0) { // only rank 0 talks on stdout
                if (!freopen("/dev/null", "w", stdout)) _exit(3);
            }
            _exit(run_rank(o, r, up[1], down[0]));
        }
        close(up[1]);
        close(down[0]);
        up_r[r] = up[0];
        down_w[r] = down[1];
        kids[r] = pid;
    }
    signal(SIGPIPE, SIG_IGN); // a rank that died must show up as a failed write, not end the parent
    // relay the unique id, then one loss sum per epoch
    uint8_t id[LSTM_HIP_UNIQUE_ID_BYTES];
    if (read(up_r[0], id, sizeof(id)) != (ssize_t)sizeof(id)) die("rank 0 did not produce a unique id");
    for (int r = 0; r < o.gpus; r++)
        if (write(down_w[r], id, sizeof(id)) != (ssize_t)sizeof(id)) die("relay");
    // The relay never blocks on ONE rank's pipe: a rank that fails (a non-finite window, a hand-off time-out, a HIP error)
    // leaves the others blocked inside the next all-reduce, so its death must be noticed while its peers are silent.
    // poll() over all pipes with a short time-out, children reaped without blocking in between.
    bool relay_failed = false;
    std::vector<bool> done(o.gpus, false);
    int live = o.gpus, rc = 0;
    auto reap_nonblocking = [&]() {
        for (;;) {
            int st = 0;
            const pid_t p = waitpid(-1, &st, WNOHANG);
            if (p <= 0) break;
            for (int r = 0; r < o.gpus; r++)
                if (kids[r] == p && !done[r]) {
                    done[r] = true;
                    live--;
                    if (!WIFEXITED(st) || WEXITSTATUS(st) != 0) {
                        rc = 1;
                        relay_failed = true;
                    }
                }
        }
    };
    for (long e = 0; e < o.epochs && !relay_failed; e++) {
        double sum = 0.0;
        std::vector<double> part(o.gpus, 0.0);
        std::vector<bool> got(o.gpus, false);
        int missing = o.gpus;
        while (missing > 0 && !relay_failed) {
            std::vector<pollfd> fds;
            std::vector<int> who;
            for (int r = 0; r < o.gpus; r++)
                if (!got[r]) {
                    fds.push_back(pollfd{up_r[r], POLLIN, 0});
                    who.push_back(r);
                }
            const int n = poll(fds.data(), (nfds_t)fds.size(), 200);
            if (n < 0 && errno != EINTR) relay_failed = true;
            for (size_t k = 0; k < fds.size() && n > 0; k++) {
                if (!(fds[k].revents & (POLLIN | POLLHUP | POLLERR))) continue;
                double v = 0.0;
                if (read(fds[k].fd, &v, sizeof(v)) != (ssize_t)sizeof(v)) { // EOF: that rank is gone
                    relay_failed = true;
                    break;
                }
                part[who[k]] = v;
                got[who[k]] = true;
                missing--;
            }
            reap_nonblocking(); // a child that ended (badly, or before delivering) while its peers are blocked
            if (live < o.gpus && missing > 0) {
                for (int r = 0; r < o.gpus; r++)
                    if (done[r] && !got[r]) relay_failed = true; // it will never deliver
            }
        }
        if (relay_failed) break;
        for (int r = 0; r < o.gpus; r++) sum += part[r]; // rank order: the same sum on every run
        for (int r = 0; r < o.gpus; r++)
            if (write(down_w[r], &sum, sizeof(sum)) != (ssize_t)sizeof(sum)) relay_failed = true;
    }
    // Reap.  A rank that fails (a non-finite window, a hand-off time-out, a HIP error) leaves the others blocked inside the
    // next all-reduce: as soon as the relay breaks or any child ends badly, the remaining children are terminated instead
    // of waited for.
    bool failed = relay_failed;
    if (failed) rc = 1;
    while (live > 0) {
        if (failed)
            for (int r = 0; r < o.gpus; r++)
                if (!done[r]) kill(kids[r], SIGTERM);
        int st = 0;
        const pid_t p = waitpid(-1, &st, 0);
        if (p < 0) break;
        for (int r = 0; r < o.gpus; r++)
            if (kids[r] == p && !done[r]) {
                done[r] = true;
                live--;
                if (!WIFEXITED(st) || WEXITSTATUS(st) != 0) {
                    rc = 1;
                    failed = true;
                }
            }
    }
    return rc;
}
