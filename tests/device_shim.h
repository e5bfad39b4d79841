// device_shim.h -- what the host emulations of the inference heads (tests/*_head*_emulation.cc) need in order to compile
// eigen-lstm_amd/csrc/heads/*.inc, the text kernels.hip includes, with g++: the device qualifiers as empty words, threadIdx and
// blockIdx per std::thread, a std::barrier for __syncthreads, function-static arrays for static LDS, ordinary memory behind
// HEAD_DYNAMIC_LDS, a lock for the int atomics, cross-lane shuffles through a table, and run_blocks, the launch.  It checks a
// head's logic without a device; it says nothing about the GPU build.
#pragma once
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static
struct Dim { int x; };
inline thread_local Dim threadIdx, blockIdx;
inline std::barrier<> *g_bar;
inline void __syncthreads() { g_bar->arrive_and_wait(); }
inline std::mutex g_mu;
inline int atomicMax(int *p, int v) { std::lock_guard<std::mutex> l(g_mu); int o = *p; if (v > o) *p = v; return o; }
inline int atomicAdd(int *p, int v) { std::lock_guard<std::mutex> l(g_mu); int o = *p; *p = o + v; return o; }
alignas(8) inline unsigned char g_lane[256][8];
template <class T> T __shfl_xor(T v, int o, int) { // (every work-item of the group calls it: the kernels' rounds are uniform)
    memcpy(g_lane[threadIdx.x], &v, sizeof(T));
    g_bar->arrive_and_wait();
    T r;
    memcpy(&r, g_lane[threadIdx.x ^ o], sizeof(T));
    g_bar->arrive_and_wait();
    return r;
}
// (a template, so that an emulation which brings an atomicOr of its own keeps it: the plain function is the better match)
template <class T> T atomicOr(T *p, T v) { std::lock_guard<std::mutex> l(g_mu); T o = *p; *p = o | v; return o; }
template <class T> T __shfl_up(T v, int d, int) { // lane = work-item mod 64; lanes below d keep their own value
    memcpy(g_lane[threadIdx.x], &v, sizeof(T));
    g_bar->arrive_and_wait();
    T r = v;
    if ((threadIdx.x & 63) >= d) memcpy(&r, g_lane[threadIdx.x - d], sizeof(T));
    g_bar->arrive_and_wait();
    return r;
}
alignas(16) inline unsigned char g_dynamic_lds[64 * 1024]; // the most a head is granted
#define HEAD_DYNAMIC_LDS(T, name) T *name = reinterpret_cast<T *>(g_dynamic_lds)

template <typename T> std::vector<T> load(const char *path) {
    FILE *f = fopen(path, "rb"); if (!f) { perror(path); exit(1); }
    fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
    std::vector<T> v(n / sizeof(T)); if (fread(v.data(), 1, n, f) != (size_t)n) exit(1); fclose(f); return v;
}
template <typename T> void save(const char *path, const std::vector<T> &v) {
    FILE *f = fopen(path, "wb"); fwrite(v.data(), sizeof(T), v.size(), f); fclose(f);
}
// kernel() as a launch of `grid` workgroups of 256 work-items: one workgroup at a time, one std::thread per work-item
template <class F> void run_blocks(int grid, F kernel) {
    for (int b = 0; b < grid; b++) {
        std::barrier<> bar(256);
        g_bar = &bar;
        std::vector<std::thread> th;
        for (int m = 0; m < 256; m++)
            th.emplace_back([&, m, b]() {
                threadIdx.x = m; blockIdx.x = b;
                kernel();
                bar.arrive_and_drop();
            });
        for (auto &x : th) x.join();
    }
}
