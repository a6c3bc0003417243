// simplyp_score.h -- the rules by which an ensemble forecast is scored against observations, in plain C++ (no HIP, no
// context): the continuous ranked probability score split into its accuracy and spread terms, the two weighted counts the
// probability integral transform is made of, and what the scoring entries' arguments must satisfy.  The entries of
// simplyp_hip.hip, the kernels of simplyp_score.hip.h (the two term functions) and a host program (tests/score_host_main.cpp)
// share it; simplyp_amd/score.py states the same rules in Python integers and fractions.
//
// One row over its member axis, values x_j, one observation y.  Participation and order are simplyp_weighted.h's: member j
// takes part iff its include flag is set and its integer weight q_j > 0 (no weights: q_j = 1), T is the sum of the participating
// weights, the key order has NaN after +inf and -0.0 equal to +0.0.
//   below       = sum q_j [x_j < y]      at_or_below = sum q_j [x_j <= y]       exact; a NaN member is above every y
//   abs_err  A  = (1/T) sum q_j |x_j - y|
//   spread   B  = (1/T^2) sum_k (x_(k+1) - x_(k)) C_k (T - C_k)                 x_(k) in key order, C_k the inclusive running weight
//   CRPS        = A - B  (the caller's subtraction)
// below / T and at_or_below / T are F(y-) and F(y) of the weighted empirical CDF whose inverse simplyp_weighted_quantiles
// returns.  B is half the expected distance of two independent draws, written over the gaps so that every term is >= 0.
// A row whose y is NaN is not scored (sums NaN, counts 0); an infinite y is an argument error; a participating non-finite
// value makes A and B NaN and leaves the counts exact; T == 0 gives NaN and 0.
//
// Every term of A and B is non-negative and costs at most 8 roundings, so a sum of them is accurate relative to itself.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "simplyp_weighted.h"

#if defined(__HIPCC__)
#define SIMPLYP_SCORE_HD __host__ __device__
#else
#define SIMPLYP_SCORE_HD
#endif

namespace simplyp_score {

constexpr int SCORE_TILE = 4096;                   // (key, weight) pairs one workgroup sorts in LDS: 64 KiB

// One term of A: |x - y| q / T.  The quotient is at most 1, so the product cannot overflow where A does not.
SIMPLYP_SCORE_HD inline double abs_err_term(double x, double y, uint64_t q, uint64_t T)
{
    return fabs(x - y) * ((double)q / (double)T);
}

// One term of B: the gap above the k-th value in key order times C_k (T - C_k) / T^2, each quotient at most 1.
SIMPLYP_SCORE_HD inline double spread_term(double lo, double hi, uint64_t C, uint64_t T)
{
    return (hi - lo) * (((double)C / (double)T) * ((double)(T - C) / (double)T));
}

struct RowScore {
    double abs_err, spread;
    uint64_t below, at_or_below, T;
};

// The reference scoring of one row: stable sort by key, serial sums in long double.  w == nullptr: every weight is 1.
inline RowScore score_row(const double* x, const uint64_t* w, const uint8_t* include, int n, double y)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    RowScore s{nan, nan, 0, 0, 0};
    if (y != y) return s;
    std::vector<std::pair<uint64_t, int>> order;
    for (int i = 0; i < n; ++i)
        if ((!include || include[i]) && (w ? w[i] : 1) > 0) order.emplace_back(simplyp_weighted::order_key(x[i]), i);
    for (const auto& o : order) s.T += w ? w[o.second] : 1;
    if (s.T == 0) return s;
    std::stable_sort(order.begin(), order.end(), [](const std::pair<uint64_t, int>& a, const std::pair<uint64_t, int>& b) { return a.first < b.first; });
    bool finite = true;
    long double A = 0.0L, B = 0.0L;
    uint64_t C = 0;
    for (size_t k = 0; k < order.size(); ++k) {
        const int i = order[k].second;
        const uint64_t q = w ? w[i] : 1;
        C += q;
        if (x[i] < y) s.below += q;
        if (x[i] <= y) s.at_or_below += q;
        finite = finite && std::isfinite(x[i]);
        if (!finite) continue;
        A += fabsl((long double)x[i] - (long double)y) * (long double)q;
        if (k + 1 < order.size() && std::isfinite(x[order[k + 1].second]))
            B += ((long double)x[order[k + 1].second] - (long double)x[i]) * ((long double)C / (long double)s.T) * (long double)(s.T - C);
    }
    if (finite) {
        s.abs_err = (double)(A / (long double)s.T);
        s.spread = (double)(B / (long double)s.T);
    }
    return s;
}

// The rows of an observation array that are scored: those whose y is not NaN.  An infinite observation is an argument error.
inline int scored_rows(const char* me, const double* y, int64_t n_rows, std::vector<int64_t>& rows, std::string& msg)
{
    rows.clear();
    for (int64_t r = 0; r < n_rows; ++r) {
        if (y[r] != y[r]) continue;
        if (std::isinf(y[r])) return simplyp_table::reject(msg, me, "observation %lld is infinite: NaN stands for no observation", (long long)r);
        rows.push_back(r);
    }
    return SIMPLYP_OK;
}

// What both scoring entries check of the scores' own arguments before anything is touched.
inline int check_outputs(const char* me, int64_t E, const void* y, const void* sums, const void* counts, std::string& msg)
{
    if (E < 1 || E > simplyp_weighted::MAX_E) return simplyp_table::reject(msg, me, "E must be in [1, 2^22] (got %lld)", (long long)E);
    if (!y) return simplyp_table::reject(msg, me, "the observations must not be NULL");
    if (!sums || !counts) return simplyp_table::reject(msg, me, "sums and counts must not be NULL");
    return SIMPLYP_OK;
}

// simplyp_scores' arguments.
inline int check_table(const char* me, int64_t E, int64_t n_rows, const void* table, const void* y, const void* sums, const void* counts,
                       std::string& msg)
{
    if (int rc = check_outputs(me, E, y, sums, counts, msg)) return rc;
    if (n_rows < 0) return simplyp_table::reject(msg, me, "n_rows must be >= 0 (got %lld)", (long long)n_rows);
    if (!table) return simplyp_table::reject(msg, me, "table must not be NULL");
    return SIMPLYP_OK;
}

// Scored rows a chunk of the workspace holds: `row_bytes` each in `budget` bytes (one row when a row is larger), or the fewer
// that SIMPLYP_SCORE_CHUNK_ROWS says (> 0): the environment can shorten a chunk, never grow it past the budget.
inline int64_t chunk_rows(int64_t n_scored, uint64_t row_bytes, uint64_t budget, const char* env)
{
    int64_t rows = (int64_t)std::max<uint64_t>(1, budget / std::max<uint64_t>(row_bytes, 1));
    if (env) {
        const long long v = atoll(env);
        if (v > 0) rows = std::min<int64_t>(rows, v);
    }
    return std::max<int64_t>(1, std::min<int64_t>(rows, std::max<int64_t>(n_scored, 1)));
}

// ---- the probability integral transform ----------------------------------------------------------------------------------
// The mid-point of the observation's interval [below / T, at_or_below / T] of the forecast CDF; NaN when T == 0.
inline double pit(uint64_t below, uint64_t at_or_below, uint64_t T)
{
    if (T == 0) return std::numeric_limits<double>::quiet_NaN();
    return (double)((long double)(below + at_or_below) / (2.0L * (long double)T));
}

// Adds one observation to a rank histogram of n_bins equal bins over [0, 1]: its interval spread uniformly over the bins it
// overlaps; below == at_or_below is a point mass at below / T, and 1.0 goes into the last bin.
inline void pit_histogram_add(uint64_t below, uint64_t at_or_below, uint64_t T, int n_bins, double* hist)
{
    if (T == 0 || n_bins < 1) return;
    const long double lo = (long double)below / (long double)T, hi = (long double)at_or_below / (long double)T;
    if (below == at_or_below) {
        // floor(below n_bins / T) in integers: below <= T <= 2^62 and n_bins < 2^31 fit 128 bits
        const uint64_t b = (uint64_t)(((unsigned __int128)below * (unsigned)n_bins) / T);
        hist[std::min<uint64_t>(b, (uint64_t)n_bins - 1)] += 1.0;
        return;
    }
    for (int b = 0; b < n_bins; ++b) {
        const long double a = std::max(lo, (long double)b / n_bins), z = std::min(hi, (long double)(b + 1) / n_bins);
        if (z > a) hist[b] += (double)((z - a) / (hi - lo));
    }
}

}  // namespace simplyp_score
