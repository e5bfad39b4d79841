// checkpoint.h -- Parameters::save_to_disk / load_from_disk, OV/lstm_eigen_class_CUDA/lstm.h:83-101, io.h:16-74:
// five text files <prefix>_{W,U,Why,b,by}.txt in the reference's own layout (matrix_io.h), shared by the training
// program (lstm_main.cc) and the generator (generate_main.cc).  Errors come back as text; the programs decide how to end.
#pragma once
#include "matrix_io.h"

#include <fstream>
#include <string>
#include <vector>

namespace checkpoint {

struct Block {
    const char *name;
    size_t rows, cols, off;
};
inline std::vector<Block> blocks(int N, int M) {
    size_t o = 0;
    std::vector<Block> b;
    auto add = [&](const char *n, size_t r, size_t c) {
        b.push_back({n, r, c, o});
        o += r * c;
    };
    add("W", 4 * (size_t)N, M);
    add("U", 4 * (size_t)N, N);
    add("b", 4 * (size_t)N, 1);
    add("Why", M, N);
    add("by", M, 1);
    return b;
}
// false (and *err) when a file cannot be written
inline bool save_params(const std::string &prefix, const std::vector<float> &P, int N, int M, int digits, std::string *err) {
    for (const Block &b : blocks(N, M)) {
        const std::string path = prefix + "_" + b.name + ".txt";
        if (!matrix_io::write_matrix(path, b.rows, b.cols, [&](size_t r, size_t c) { return P[b.off + c * b.rows + r]; }, digits)) {
            *err = "cannot write " + path;
            return false;
        }
    }
    return true;
}
// 1: loaded; 0: a file is missing (nothing is reported); -1: a file is malformed or has the wrong shape (*err)
inline int load_params(const std::string &prefix, std::vector<float> &P, int N, int M, std::string *err) {
    for (const Block &b : blocks(N, M)) {
        const std::string path = prefix + "_" + b.name + ".txt";
        size_t rows = 0, cols = 0;
        if (!std::ifstream(path).good()) return 0;
        if (!matrix_io::read_matrix(path, [&](size_t r, size_t c, double v) {
                if (r < b.rows && c < b.cols) P[b.off + c * b.rows + r] = (float)v;
            }, &rows, &cols)) {
            *err = path + ": rows of different lengths";
            return -1;
        }
        if (rows != b.rows || cols != b.cols) {
            *err = path + ": " + std::to_string(rows) + " x " + std::to_string(cols) + ", expected " + std::to_string(b.rows) +
                   " x " + std::to_string(b.cols);
            return -1;
        }
    }
    return 1;
}
// the hidden size of a checkpoint: rows of <prefix>_W.txt / 4 (W is 4N x M).  0 with *err when it cannot be told.
inline int hidden_size(const std::string &prefix, int M, std::string *err) {
    const std::string path = prefix + "_W.txt";
    size_t rows = 0, cols = 0;
    if (!matrix_io::read_matrix(path, [](size_t, size_t, double) {}, &rows, &cols)) {
        *err = "cannot read " + path;
        return 0;
    }
    if (rows == 0 || rows % 4 != 0 || cols != (size_t)M) {
        *err = path + ": " + std::to_string(rows) + " x " + std::to_string(cols) + ", expected 4N x " + std::to_string(M);
        return 0;
    }
    return (int)(rows / 4);
}

} // namespace checkpoint
