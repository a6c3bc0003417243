// simplyp_weighted.h -- the integer rules of the weighted bands, in plain C++ (no HIP, no context): what a probability's
// threshold is under integer weights, which element of a row it selects, and what the weighted entries' arguments must
// satisfy.  The entries of simplyp_hip.hip and a host program (tests/weighted_host_main.cpp) share it;
// simplyp_amd/weighted.py states the same rules with Python integers.
//
// One row over its member axis, weights q_i the integers simplyp_pf_weights writes (0 <= q_i <= 2^40, 1 <= E <= 2^22):
//   a member takes part iff its include flag is set and q_i > 0;  T = the sum of the participating weights <= 2^62
//   the members are ordered as simplyp_quantiles orders them: NaN after +inf, -0.0 and +0.0 equal
//   C_i = the inclusive running sum of the weights in that order
//   t   = max(1, ceil(p T)) for a probability p, exactly: p = m 2^e with m < 2^53, so m T < 2^115 fits 128 bits and t is a
//         shift with a ceiling
//   the result is the value of the first member in that order with C_i >= t: the order statistic of rank t - 1 (zero-based) of
//   the multiset in which member i occurs q_i times -- numpy's method='inverted_cdf' with weights=.
// Nothing is rounded, so every implementation of the rule returns the same element of the row.  T = 0: NaN.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "simplyp_table.h"

namespace simplyp_weighted {

constexpr int WEIGHT_BITS = 40;                    // a weight is at most 2^40: what simplyp_pf_weights gives the heaviest particle
constexpr uint64_t MAX_WEIGHT = 1ull << WEIGHT_BITS;
constexpr int MAX_E = 1 << 22;                     // keeps T below 2^62
constexpr int MAX_K = 16;                          // probabilities per call

// t = max(1, ceil(p T)) for 0 <= p <= 1 and T <= 2^62, exactly.
inline uint64_t weighted_threshold(double p, uint64_t T)
{
    if (!(p > 0.0) || T == 0) return 1;
    int ex = 0;
    const double f = std::frexp(p, &ex);           // p = f 2^ex, 0.5 <= f < 1 (subnormals too)
    const uint64_t m = (uint64_t)std::ldexp(f, 53);    // an integer below 2^53, exactly
    const int s = 53 - ex;                         // p = m 2^-s, s >= 52 since p <= 1
    const unsigned __int128 prod = (unsigned __int128)m * T;
    if (s >= 128) return 1;                        // 0 < p T < 1
    const uint64_t whole = (uint64_t)(prod >> s);
    const bool rest = (prod & ((((unsigned __int128)1) << s) - 1)) != 0;
    return std::max<uint64_t>(1, whole + (rest ? 1 : 0));
}

// simplyp_quantiles' order of fp64 values as unsigned integers: every NaN one key above +inf's.
inline uint64_t order_key(double x)
{
    if (x != x) return 0xFFF8000000000000ull;
    uint64_t b;
    std::memcpy(&b, &x, sizeof b);
    if (b == 0x8000000000000000ull) b = 0;         // -0.0 and +0.0 compare equal
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// The sum of the weights that take part in a row (include == nullptr: all flags set).
inline uint64_t row_total(const uint64_t* w, const uint8_t* include, int n)
{
    uint64_t T = 0;
    for (int i = 0; i < n; ++i) if (!include || include[i]) T += w[i];
    return T;
}

// The reference selection of one row: stable sort by key, running sum, first C_i >= t.  NaN when nobody takes part.
inline double select_row(const double* x, const uint64_t* w, const uint8_t* include, int n, double p)
{
    std::vector<std::pair<uint64_t, int>> order;
    for (int i = 0; i < n; ++i)
        if ((!include || include[i]) && w[i] > 0) order.emplace_back(order_key(x[i]), i);
    const uint64_t t = weighted_threshold(p, row_total(w, include, n));
    std::stable_sort(order.begin(), order.end(), [](const std::pair<uint64_t, int>& a, const std::pair<uint64_t, int>& b) { return a.first < b.first; });
    uint64_t C = 0;
    for (const auto& o : order) {
        C += w[o.second];
        if (C >= t) return x[o.second];
    }
    return std::numeric_limits<double>::quiet_NaN();
}

// What both weighted entries check of the selection's own arguments before anything is touched.
inline int check_selection(const char* me, int64_t E, const void* weights, const double* q, int32_t K, const void* order_stats,
                           std::string& msg)
{
    if (E < 1 || E > MAX_E) return simplyp_table::reject(msg, me, "E must be in [1, 2^22] (got %lld)", (long long)E);
    if (!weights) return simplyp_table::reject(msg, me, "weights must not be NULL");
    if (!order_stats) return simplyp_table::reject(msg, me, "order_stats must not be NULL");
    return simplyp_table::check_probabilities(me, q, K, MAX_K, msg);
}

// simplyp_weighted_quantiles' arguments.
inline int check_table(const char* me, int64_t E, int64_t n_rows, const void* table, const void* weights, const double* q, int32_t K,
                       const void* order_stats, std::string& msg)
{
    if (E < 1 || E > MAX_E || n_rows < 0)
        return simplyp_table::reject(msg, me, "E must be in [1, 2^22] and n_rows >= 0 (got E = %lld, n_rows = %lld)", (long long)E, (long long)n_rows);
    if (!table) return simplyp_table::reject(msg, me, "table must not be NULL");
    return check_selection(me, E, weights, q, K, order_stats, msg);
}

// What the prepare kernel found: a weight above 2^40 is an argument error.
inline int check_weights(const char* me, int n_bad, std::string& msg)
{
    if (n_bad > 0) return simplyp_table::reject(msg, me, "%d weights exceed 2^40: not what simplyp_pf_weights writes", n_bad);
    return SIMPLYP_OK;
}

}  // namespace simplyp_weighted
