// simplyp_resample.h -- the integer rules of the particle filter's resampling step, in plain C++ (no HIP beyond the qualifier
// macro below): how a normalised weight becomes an integer, how the Philox word becomes the offset, and which ancestor a
// particle takes.  The resampling kernel (simplyp_particle.hip.h) and a host program (tests/particle_host_main.cpp) share it;
// simplyp_amd/particle.py states the same rules with Python integers.
//
// Systematic resampling of E particles with integer weights q_i, 0 <= q_i <= 2^40, 1 <= E <= 2^22:
//   C_i = q_0 + ... + q_i, T = C_{E-1} <= 2^62
//   r   = the high 64 bits of x T for a 64-bit word x, so 0 <= r < T
//   the ancestor of particle k is the smallest i with E C_i > k T + r
// Both sides of the comparison are exact integers below 2^85, carried here as two 64-bit halves.  Nothing is rounded, so every
// implementation of the rule gives the same ancestors; they do not decrease with k, and particle i is taken floor(E q_i / T) or
// ceil(E q_i / T) times.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SIMPLYP_RS_HD __host__ __device__
#else
#define SIMPLYP_RS_HD
#endif

namespace simplyp_resample {

constexpr int WEIGHT_BITS = 40;                    // the filter resolves normalised weights to 2^-40
constexpr int MAX_LOG2_E = 22;                     // E <= 2^22 keeps T below 2^62 and the products below 2^85
constexpr int MAX_E = 1 << MAX_LOG2_E;

struct U128 {
    uint64_t hi, lo;
};

// a b, all 128 bits, from 32-bit limbs
SIMPLYP_RS_HD inline U128 mul_64x64(uint64_t a, uint64_t b)
{
    const uint64_t M = 0xFFFFFFFFull;
    const uint64_t a0 = a & M, a1 = a >> 32, b0 = b & M, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (p01 & M) + (p10 & M);             // < 3 2^32
    return U128{p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32), (p00 & M) | (mid << 32)};
}

SIMPLYP_RS_HD inline U128 add_64(U128 a, uint64_t b)
{
    const uint64_t lo = a.lo + b;
    return U128{a.hi + (lo < b ? 1u : 0u), lo};
}

SIMPLYP_RS_HD inline bool greater(U128 a, U128 b)
{
    return a.hi != b.hi ? a.hi > b.hi : a.lo > b.lo;
}

// floor(w 2^40) of a normalised weight 0 <= w <= 1: the scaling is exact, the conversion truncates.  A NaN gives 0.
SIMPLYP_RS_HD inline uint64_t quantise(double w)
{
    return w > 0.0 ? (uint64_t)(w * 1099511627776.0) : 0u;
}

// r of the 64-bit word x: the high half of x T
SIMPLYP_RS_HD inline uint64_t offset(uint64_t x, uint64_t T)
{
    return mul_64x64(x, T).hi;
}

// E C > k T + r
SIMPLYP_RS_HD inline bool points_past(uint64_t E, uint64_t C, uint64_t k, uint64_t T, uint64_t r)
{
    return greater(mul_64x64(E, C), add_64(mul_64x64(k, T), r));
}

// The ancestor of particle k: the smallest i in [0, E) with E C[i] > k T + r, by bisection over the non-decreasing C.
// T = C[E - 1] > 0 and r < T make i = E - 1 qualify for every k < E.
SIMPLYP_RS_HD inline int32_t ancestor(const uint64_t* C, int32_t E, int32_t k, uint64_t T, uint64_t r)
{
    const U128 rhs = add_64(mul_64x64((uint64_t)k, T), r);
    int32_t lo = 0, hi = E - 1;                    // the answer lies in [lo, hi]
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (greater(mul_64x64((uint64_t)E, C[mid]), rhs)) hi = mid; else lo = mid + 1;
    }
    return lo;
}

}  // namespace simplyp_resample
