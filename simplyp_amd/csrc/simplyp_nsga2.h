// simplyp_nsga2.h -- NSGA-II's variation of one dimension of one child pair and what the four simplyp_nsga2_* entries' arguments
// must satisfy, in plain C++ (no HIP, no context).  The kernels of simplyp_nsga2.hip.h and a host program
// (tests/nsga2_host_main.cpp) compile this text; simplyp_amd/nsga2.py states the same rule in NumPy and is its definition.
//
// Deb's bounded SBX and bounded polynomial mutation with eta = 2^k - 1, k in 1 .. 5: (.)^(eta + 1) is k squarings (powk) and
// (.)^(1 / (eta + 1)) is k nested square roots (rootk).  Only + - * / sqrt and comparisons in fp64, every one written out in
// its order: with -ffp-contract=off and correctly rounded / and sqrt the host and the device return the same bits.  The
// uniforms are arguments -- Philox stays in simplyp_predictive.hip.h.
//
//   SBX of a dimension that takes part (cross, u_take < 1/2, x1 != x2), y1 = min, y2 = max, dy = y2 - y1:
//     bq(beta): alpha = 2 - 1 / beta^(eta+1);  ua = u alpha;  bq = ua^(1/(eta+1)) if u <= 1 / alpha, else (1 / (2 - ua))^(1/(eta+1))
//     c1 = 0.5 ((y1 + y2) - bq(1 + 2 (y1 - lo) / dy) dy),  c2 = 0.5 ((y1 + y2) + bq(1 + 2 (hi - y2) / dy) dy), both clipped;
//     child A = c1, child B = c2, swapped iff u_swap < 1/2.  A dimension that does not take part hands x1 to A and x2 to B.
//   mutation of a child c iff u_do < p_mut, w = hi - lo:
//     u <= 1/2: xy = 1 - (c - lo) / w;  val = 2u + (1 - 2u) xy^(eta+1);              dq = val^(1/(eta+1)) - 1
//     u >  1/2: xy = 1 - (hi - c) / w;  val = 2 (1 - u) + (2 (u - 1/2)) xy^(eta+1);  dq = 1 - val^(1/(eta+1))
//     c <- clip(c + dq w)
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SIMPLYP_NSGA2_HD __host__ __device__ __forceinline__
#else
#include <cmath>
#define SIMPLYP_NSGA2_HD inline
#endif

#include <string>

#include "simplyp_table.h"

namespace simplyp_nsga2 {

constexpr int MAX_DIM = 16;
constexpr int MAX_OBJ = SIMPLYP_PARETO_MAX_OBJ;
constexpr int MIN_POP = 4, MAX_POP = 65536;
constexpr int MAX_SET = 2 * MAX_POP;               // the combined set of parents and children
constexpr int MAX_K = 5;                           // eta = 2^k - 1 <= 31
constexpr int MAX_ROWS = 64;                       // rows simplyp_nsga2_select gathers

SIMPLYP_NSGA2_HD double powk(double x, int k)
{
    for (int i = 0; i < k; ++i) x = x * x;
    return x;
}

SIMPLYP_NSGA2_HD double rootk(double x, int k)
{
#if defined(__HIP_DEVICE_COMPILE__)
    for (int i = 0; i < k; ++i) x = __builtin_sqrt(x);
#else
    for (int i = 0; i < k; ++i) x = std::sqrt(x);
#endif
    return x;
}

SIMPLYP_NSGA2_HD double clip(double c, double lo, double hi)
{
    return c < lo ? lo : (c > hi ? hi : c);
}

SIMPLYP_NSGA2_HD double bq(double beta, double u, int k)
{
    const double alpha = 2.0 - 1.0 / powk(beta, k);
    const double ua = u * alpha;
    return u <= 1.0 / alpha ? rootk(ua, k) : rootk(1.0 / (2.0 - ua), k);
}

SIMPLYP_NSGA2_HD void sbx(double x1, double x2, double lo, double hi, int k, bool cross, double u, double u_take, double u_swap,
                          double& a, double& b)
{
    a = x1; b = x2;
    if (!(cross && u_take < 0.5 && x1 != x2)) return;
    const double y1 = x1 < x2 ? x1 : x2, y2 = x1 < x2 ? x2 : x1;
    const double dy = y2 - y1;
    const double c1 = clip(0.5 * ((y1 + y2) - bq(1.0 + 2.0 * (y1 - lo) / dy, u, k) * dy), lo, hi);
    const double c2 = clip(0.5 * ((y1 + y2) + bq(1.0 + 2.0 * (hi - y2) / dy, u, k) * dy), lo, hi);
    const bool swap = u_swap < 0.5;
    a = swap ? c2 : c1;
    b = swap ? c1 : c2;
}

SIMPLYP_NSGA2_HD double mutate(double c, double lo, double hi, int k, double p_mut, double u_do, double u)
{
    if (!(u_do < p_mut)) return c;
    const double w = hi - lo;
    const bool low = u <= 0.5;
    const double xy = 1.0 - (low ? c - lo : hi - c) / w;
    const double p = powk(xy, k);
    const double t = 2.0 * u;
    const double val = low ? t + (1.0 - t) * p : 2.0 * (1.0 - u) + (2.0 * (u - 0.5)) * p;
    const double r = rootk(val, k);
    const double dq = low ? r - 1.0 : 1.0 - r;
    return clip(c + dq * w, lo, hi);
}

// One dimension of one pair: SBX, then the mutation of either child.
SIMPLYP_NSGA2_HD void vary_dim(double x1, double x2, double lo, double hi, int k_c, int k_m, double p_mut, bool cross,
                               double u, double u_take, double u_swap, double u_do_a, double u_a, double u_do_b, double u_b,
                               double& child_a, double& child_b)
{
    double a, b;
    sbx(x1, x2, lo, hi, k_c, cross, u, u_take, u_swap, a, b);
    child_a = mutate(a, lo, hi, k_m, p_mut, u_do_a, u_a);
    child_b = mutate(b, lo, hi, k_m, p_mut, u_do_b, u_b);
}

// ---- the entries' arguments, before anything is touched -----------------------------------------------------------------------
inline int check_pop(const char* me, int64_t N, int64_t n_dim, std::string& msg)
{
    if (N < MIN_POP || N > MAX_POP || (N & 1))
        return simplyp_table::reject(msg, me, "N must be even and in [%d, %d] (got %lld)", MIN_POP, MAX_POP, (long long)N);
    if (n_dim < 1 || n_dim > MAX_DIM) return simplyp_table::reject(msg, me, "n_dim must be in [1, %d] (got %lld)", MAX_DIM, (long long)n_dim);
    return SIMPLYP_OK;
}

inline int check_init(const char* me, int64_t N, int64_t n_dim, const void* theta, std::string& msg)
{
    if (int rc = check_pop(me, N, n_dim, msg)) return rc;
    if (!theta) return simplyp_table::reject(msg, me, "theta must not be NULL");
    return SIMPLYP_OK;
}

inline int check_offspring(const char* me, int64_t N, int64_t n_dim, int64_t k_c, int64_t k_m, double p_cross, double p_mut,
                           const void* theta, const void* rank, const void* crowd, const void* child, std::string& msg)
{
    if (int rc = check_pop(me, N, n_dim, msg)) return rc;
    if (k_c < 1 || k_c > MAX_K || k_m < 1 || k_m > MAX_K)
        return simplyp_table::reject(msg, me, "k_c and k_m must be in [1, %d]: eta = 2^k - 1 (got %lld, %lld)", MAX_K, (long long)k_c, (long long)k_m);
    if (!(p_cross >= 0.0 && p_cross <= 1.0)) return simplyp_table::reject(msg, me, "p_cross must be in [0, 1] (got %g)", p_cross);
    if (!(p_mut >= 0.0 && p_mut <= 1.0)) return simplyp_table::reject(msg, me, "p_mut must be in [0, 1] (got %g)", p_mut);
    if (!theta || !rank || !crowd || !child) return simplyp_table::reject(msg, me, "theta, rank, crowd and child must not be NULL");
    return SIMPLYP_OK;
}

inline int check_crowding(const char* me, int64_t n, int64_t M, const void* obj, const int32_t* sense, const void* rank,
                          const void* crowd, std::string& msg)
{
    if (n < 1 || n > MAX_SET) return simplyp_table::reject(msg, me, "n must be in [1, %d] (got %lld)", MAX_SET, (long long)n);
    if (M < 1 || M > MAX_OBJ) return simplyp_table::reject(msg, me, "M must be in [1, %d] (got %lld)", MAX_OBJ, (long long)M);
    if (!obj || !sense || !rank || !crowd) return simplyp_table::reject(msg, me, "obj, sense, rank and crowd must not be NULL");
    for (int m = 0; m < M; ++m)
        if (sense[m] != 1 && sense[m] != -1) return simplyp_table::reject(msg, me, "sense[%d] must be +1 or -1 (got %d)", m, (int)sense[m]);
    return SIMPLYP_OK;
}

inline int check_select(const char* me, int64_t n, int64_t N, const void* rank, const void* crowd, const void* position,
                        const void* survivor, int64_t n_rows, const void* rows_in, const void* rows_out, std::string& msg)
{
    if (N < MIN_POP || N > MAX_POP || (N & 1))
        return simplyp_table::reject(msg, me, "N must be even and in [%d, %d] (got %lld)", MIN_POP, MAX_POP, (long long)N);
    if (n < N || n > 2 * N) return simplyp_table::reject(msg, me, "n must be in [N, 2 N] (got n = %lld, N = %lld)", (long long)n, (long long)N);
    if (!rank || !crowd || !position || !survivor) return simplyp_table::reject(msg, me, "rank, crowd, position and survivor must not be NULL");
    if (n_rows < 0 || n_rows > MAX_ROWS) return simplyp_table::reject(msg, me, "n_rows must be in [0, %d] (got %lld)", MAX_ROWS, (long long)n_rows);
    if (n_rows > 0 && (!rows_in || !rows_out)) return simplyp_table::reject(msg, me, "rows_in and rows_out must not be NULL when n_rows > 0");
    return SIMPLYP_OK;
}

}  // namespace simplyp_nsga2
