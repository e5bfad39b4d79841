// Byte regular expressions and products of byte automata, compiled to minimal tables (include/lstm_hip.h: lstm_hip_dfa_regex,
// lstm_hip_dfa_intersect).  Plain C++ with no device code and no HIP header: dfa_regex.cpp also builds
// into a stand-alone host program.  The C ABI's entry points in lstm_hip_api.cpp are thin callers that hand `msg` to
// lstm_hip_last_error().
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

namespace dfa {

constexpr int MAX_STATES = 4096;         // of a result (the tables' 0xFFFF and the heads' uint16 states)
constexpr int MAX_REPEAT = 4095;         // the largest count of a {m,n} quantifier
constexpr int MAX_DEPTH = 200;           // nested groups
constexpr int NFA_LIMIT = 1 << 20;       // nodes of the Thompson automaton
constexpr int WORK_STATES = 32768;       // states of the subset construction / of a product before minimisation
constexpr long long WORK_STEPS = 1ll << 27; // node visits of the subset construction

// Both return the number of states Q (>= 1), or -1 with `msg` set (and *error_pos: the pattern byte, -1 where there is none).
// With next == nullptr && accept == nullptr nothing is written and cap is ignored; otherwise cap >= Q is required, next takes
// Q * 256 entries (a state, or 0xFFFF) and accept Q flags.
int32_t regex(const uint8_t *pattern, size_t len, int32_t stop_byte, uint16_t *next, uint8_t *accept, int32_t cap,
              int32_t *error_pos, std::string &msg);
int32_t intersect(const uint16_t *a, int32_t qa, const uint8_t *acc_a, const uint16_t *b, int32_t qb, const uint8_t *acc_b,
                  uint16_t *next, uint8_t *accept, int32_t cap, std::string &msg);

} // namespace dfa
