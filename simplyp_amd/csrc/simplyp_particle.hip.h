// simplyp_particle.hip.h -- sequential importance resampling over the joint (state, parameter) space on the device (gfx950):
// what a particle filter does between two model runs, without the states or the parameter arrays leaving HBM.
//
// One assimilation window is
//   (simplyp_run)                     the window's days from every particle's state and parameters, state in and state out
//   simplyp_pf_loglik_kernel          the window's Gaussian log-likelihood with sigma = m sim, added to the log weights
//   simplyp_pf_max_* / _weights_*     w = exp(lw - max lw), q = floor(w 2^40), their sums: effective sample size and evidence
//   simplyp_pf_scan_* / _search_*     systematic resampling in integers (simplyp_resample.h): prefix sum of q, one ancestor each
//   simplyp_gather_members_kernel     dst[row][k] = src[row][ancestor[k]] for the state and every array a particle owns
//   simplyp_pf_jitter_kernel          the rejuvenation move: shrink towards a centre, add a normal of the predictive stream
//
// Likelihood: for a pair (variable v, output reach r) with observation days d_1 < ... < d_n in the window,
//   SL = sum ln sim_d, SR = sum (obs_d / sim_d - 1)^2, term = -0.5 n ln(2 pi) - n ln(m) - SL - SR / (2 m m)
// in that order of operations; sim is the df_R series as tq_value forms it (simplyp_time_quantile.hip.h: the reference's
// expressions operation for operation).  This is visualise_results.loglik without its more-than-10-observations rule.  A NaN
// simulated value on an observation day makes the sum NaN, which becomes -inf: a particle may not skip an observation.
//
// Weights: a particle more than 40 ln 2 below the maximum gets q = 0 -- the filter resolves weights to 2^-40.  The sum of q is a
// 64-bit integer, exact in any order; the sums of w and w^2 are added in a fixed order (per block, then over the blocks).
//
// Layout: lane = particle (slot for the table, member for everything a particle owns), every array SoA with the particle axis
// fastest, so each load and store of a wave is one contiguous segment; the ancestors do not decrease with k, so the gather's
// reads are neighbouring or equal words.  The scan is wave64 cross-lane, then the block's four waves through LDS, then the block
// sums in one workgroup.  No per-lane arrays.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simplyp.h"
#include "simplyp_kernels.hip.h"           // sp_log
#include "simplyp_time_quantile.hip.h"     // TqSeries, tq_series, tq_value
#include "simplyp_predictive.hip.h"        // philox4x32_10, philox_normal
#include "simplyp_mcmc.hip.h"              // MCMC_MAX_DIM, MCMC_MAX_PAIRS, MCMC_TARGET_*, mcmc_count
#include "simplyp_resample.h"

namespace simplyp {

constexpr int PF_THREADS = 256;
constexpr int PF_WAVES = PF_THREADS / WAVE;
constexpr int PF_MAX_PAIRS = MCMC_MAX_PAIRS;
constexpr int PF_MAX_DIM = MCMC_MAX_DIM;
constexpr int PF_BATCH = 4;                            // observation days whose loads are issued together
constexpr int PF_GATHER_ROWS = 8;                      // rows a lane moves per step with its one ancestor
constexpr uint32_t PF_STREAM_RESAMPLE = 0x50465253u;   // "PFRS": the counter's fourth word
constexpr uint32_t PF_STREAM_JITTER = 0x50464A54u;     // "PFJT"

// What the entries leave for the host, at the head of the context's workspace (zeroed before every entry's launches).
struct PfResult {
    double lw_max, sum_w, sum_w2;
    unsigned long long T;
    unsigned n_alive, n_nan, n_unique, n_bad, n_outside, pad;
};

// ---- the window's log-likelihood ------------------------------------------------------------------------------------------------
struct PfLoglikArgs {
    int E, R, n_pairs, accumulate;
    const double* out;                     // [n_cols][D][R][E]
    long long col_stride;                  // D*R*E
    int col[4];                            // column slots of Qr, Msus_kg/day, TDP_kg/day, PP_kg/day
    int pair_var[PF_MAX_PAIRS], pair_reach[PF_MAX_PAIRS];
    int day_ptr[PF_MAX_PAIRS + 1];         // offsets of pair p's observation days in day / obs
    const int32_t* day;                    // device: the days of the window with an observation, ascending, pair after pair
    const double* obs;                     // device: the observations on those days
    const int32_t* reach_of;               // [R] device
    const int32_t* member_of_slot;         // [E] or nullptr
    const double* f_tdp;                   // [E] member order
    const double* a_catch;                 // [S][E] member order
    const double* err_m;                   // [n_pairs][E] member order
    const int32_t* status;                 // [E] member order, or nullptr
    double* lw;                            // [E] member order
    double* inc;                           // [E] member order, or nullptr
    PfResult* res;
};

__device__ __forceinline__ void pf_pair_add(double s, double o, double& SL, double& SR)
{
    const double ls = (s > 1e-290 && s < 1e290) ? sp_log(s) : log(s);      // as gof_add: IEEE results outside the ordinary range
    const double q = o / s - 1.0;
    SL += ls;
    SR += q * q;
}

template <int KIND>
__device__ __forceinline__ void pf_pair_sums(const TqSeries& sr, const int32_t* day, const double* obs, int kb, int ke,
                                             size_t day_stride, double& SL, double& SR)
{
    int k = kb;
    for (; k + PF_BATCH <= ke; k += PF_BATCH) {
        double a[PF_BATCH], b[PF_BATCH], c[PF_BATCH];
#pragma unroll
        for (int j = 0; j < PF_BATCH; ++j) {
            const size_t off = (size_t)day[k + j] * day_stride;
            a[j] = sr.p0[off];
            b[j] = KIND >= 2 ? sr.p1[off] : 0.0;
            c[j] = KIND == 3 ? sr.p2[off] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < PF_BATCH; ++j) pf_pair_add(tq_value<KIND>(sr, a[j], b[j], c[j]), obs[k + j], SL, SR);
    }
    for (; k < ke; ++k) {
        const size_t off = (size_t)day[k] * day_stride;
        pf_pair_add(tq_value<KIND>(sr, sr.p0[off], KIND >= 2 ? sr.p1[off] : 0.0, KIND == 3 ? sr.p2[off] : 0.0), obs[k], SL, SR);
    }
}

__global__ __launch_bounds__(PF_THREADS) void simplyp_pf_loglik_kernel(const PfLoglikArgs g)
{
    const int slot = blockIdx.x * PF_THREADS + threadIdx.x;
    if (slot >= g.E) return;                               // no barrier below
    int member = g.member_of_slot ? g.member_of_slot[slot] : slot;
    if ((unsigned)member >= (unsigned)g.E) member = slot;  // a map that is no permutation reads nothing out of bounds
    const size_t day_stride = (size_t)g.R * g.E;
    double sum = 0.0;
    bool m_ok = true;
    for (int p = 0; p < g.n_pairs; ++p) {
        const double m = g.err_m[(size_t)p * g.E + member];
        m_ok = m_ok && (m > 0.0);
        const int kb = g.day_ptr[p], ke = g.day_ptr[p + 1];
        if (kb == ke) continue;                            // no observation of this pair in the window: exactly nothing
        const int r = g.pair_reach[p], reach = g.reach_of[r];
        TqSeries sr;
        const int kind = tq_series(sr, -1 - g.pair_var[p], g.out, g.col_stride, g.col, (size_t)r * g.E + slot, g.a_catch, g.f_tdp,
                                   (size_t)reach * g.E + member, member);
        double SL = 0.0, SR = 0.0;
        if (kind == 1) pf_pair_sums<1>(sr, g.day, g.obs, kb, ke, day_stride, SL, SR);
        else if (kind == 2) pf_pair_sums<2>(sr, g.day, g.obs, kb, ke, day_stride, SL, SR);
        else pf_pair_sums<3>(sr, g.day, g.obs, kb, ke, day_stride, SL, SR);
        const double n = (double)(ke - kb);
        const double lm = m > 0.0 ? sp_log(m) : 0.0;
        // visualise_results.loglik, left to right (simplyp_mcmc_log_prob_kernel)
        const double term = (((-0.5 * n) * 1.8378770664093453) - n * lm - SL) - SR / ((2.0 * m) * m);
        sum = sum + term;
    }
    const bool finite_run = g.status ? (g.status[member] & SIMPLYP_STATUS_NONFINITE) == 0 : true;
    const bool is_nan = sum != sum;
    const double inc = (finite_run && m_ok && !is_nan) ? sum : -__builtin_huge_val();
    if (g.inc) g.inc[member] = inc;
    g.lw[member] = g.accumulate ? g.lw[member] + inc : inc;
    mcmc_count(&g.res->n_nan, is_nan);
}

// ---- block reductions ---------------------------------------------------------------------------------------------------------
// The block's maximum / sum in thread 0 (the waves' values combined in wave order); `s` is PF_WAVES values of LDS.
__device__ __forceinline__ double pf_block_max(double v, double* s)
{
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, WAVE));
    if ((threadIdx.x & (WAVE - 1)) == 0) s[threadIdx.x / WAVE] = v;
    __syncthreads();
    double r = s[0];
#pragma unroll
    for (int i = 1; i < PF_WAVES; ++i) r = fmax(r, s[i]);
    __syncthreads();
    return r;
}

__device__ __forceinline__ double pf_block_sum(double v, double* s)
{
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_down(v, o, WAVE);
    if ((threadIdx.x & (WAVE - 1)) == 0) s[threadIdx.x / WAVE] = v;
    __syncthreads();
    double r = s[0];
#pragma unroll
    for (int i = 1; i < PF_WAVES; ++i) r += s[i];
    __syncthreads();
    return r;
}

__device__ __forceinline__ unsigned long long pf_block_sum_u64(unsigned long long v, unsigned long long* s)
{
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_down(v, o, WAVE);
    if ((threadIdx.x & (WAVE - 1)) == 0) s[threadIdx.x / WAVE] = v;
    __syncthreads();
    unsigned long long r = s[0];
#pragma unroll
    for (int i = 1; i < PF_WAVES; ++i) r += s[i];
    __syncthreads();
    return r;
}

__device__ __forceinline__ bool pf_finite(double x) { return fabs(x) < __builtin_huge_val(); }      // false for a NaN

// ---- weights ----------------------------------------------------------------------------------------------------------------------
struct PfWeightsArgs {
    int E, n_blocks;
    const double* lw;                      // [E]
    double* w;                             // [E]
    unsigned long long* q;                 // [E]
    double* part_max;                      // [n_blocks]
    double* part_sum;                      // [2][n_blocks]: w, w^2
    PfResult* res;
};

__global__ __launch_bounds__(PF_THREADS) void simplyp_pf_max_kernel(const PfWeightsArgs g)
{
    __shared__ double s[PF_WAVES];
    const int i = blockIdx.x * PF_THREADS + threadIdx.x;
    const double x = i < g.E ? g.lw[i] : -__builtin_huge_val();
    const double v = pf_block_max(pf_finite(x) ? x : -__builtin_huge_val(), s);
    if (threadIdx.x == 0) g.part_max[blockIdx.x] = v;
}

// one workgroup
__global__ __launch_bounds__(PF_THREADS) void simplyp_pf_max_finish_kernel(const PfWeightsArgs g)
{
    __shared__ double s[PF_WAVES];
    double v = -__builtin_huge_val();
    for (int b = threadIdx.x; b < g.n_blocks; b += PF_THREADS) v = fmax(v, g.part_max[b]);
    v = pf_block_max(v, s);
    if (threadIdx.x == 0) g.res->lw_max = v;
}

__global__ __launch_bounds__(PF_THREADS) void simplyp_pf_weights_kernel(const PfWeightsArgs g)
{
    __shared__ double s[PF_WAVES];
    __shared__ unsigned long long su[PF_WAVES];
    const int i = blockIdx.x * PF_THREADS + threadIdx.x;
    const double lw_max = g.res->lw_max;                   // -inf: no entry is finite
    double w = 0.0;
    unsigned long long q = 0;
    if (i < g.E) {
        const double x = g.lw[i];
        const bool fin = pf_finite(x);
        if (fin && pf_finite(lw_max)) w = x == lw_max ? 1.0 : exp(x - lw_max);
        q = simplyp_resample::quantise(w);
        g.w[i] = w;
        g.q[i] = q;
        mcmc_count(&g.res->n_nan, !fin && !(x < 0.0));     // +inf and NaN; -inf is an ordinary dead particle
        mcmc_count(&g.res->n_alive, q > 0);
    }
    const double sw = pf_block_sum(w, s), sw2 = pf_block_sum(w * w, s);
    const unsigned long long sq = pf_block_sum_u64(q, su);
    if (threadIdx.x == 0) {
        g.part_sum[blockIdx.x] = sw;
        g.part_sum[(size_t)g.n_blocks + blockIdx.x] = sw2;
        if (sq) atomicAdd(&g.res->T, sq);                  // integers: exact in any order
    }
}

// one workgroup: the blocks' sums in a fixed order
__global__ __launch_bounds__(PF_THREADS) void simplyp_pf_sum_finish_kernel(const PfWeightsArgs g)
{
    __shared__ double s[PF_WAVES];
    double a = 0.0, b = 0.0;
    for (int k = threadIdx.x; k < g.n_blocks; k += PF_THREADS) { a += g.part_sum[k]; b += g.part_sum[(size_t)g.n_blocks + k]; }
    a = pf_block_sum(a, s);
    b = pf_block_sum(b, s);
    if (threadIdx.x == 0) { g.res->sum_w = a; g.res->sum_w2 = b; }
}

// ---- resampling -------------------------------------------------------------------------------------------------------------------
struct PfResampleArgs {
    int E, n_blocks;
    const unsigned long long* q;           // [E]
    unsigned long long* C;                 // [E] inclusive prefix sums
    unsigned long long* block_sum;         // [n_blocks]
    uint32_t key0, key1, t;
    int32_t* ancestors;                    // [E]
    int32_t* offspring;                    // [E] or nullptr (zeroed by the host)
    PfResult* res;
};

// The inclusive scan of the block's values: wave64 cross-lane, then the waves' totals through LDS.  Returns the block's total
// in every thread.
__device__ __forceinline__ unsigned long long pf_block_scan(unsigned long long& v, unsigned long long* s)
{
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const unsigned long long u = __shfl_up(v, o, WAVE);
        if (lane >= o) v += u;
    }
    if (lane == WAVE - 1) s[wave] = v;
    __syncthreads();
    unsigned long long before = 0, total = 0;
#pragma unroll
    for (int i = 0; i < PF_WAVES; ++i) { if (i < wave) before += s[i]; total += s[i]; }
    __syncthreads();
    v += before;
    return total;
}

__global__ __launch_bounds__(PF_THREADS) void simplyp_pf_scan_block_kernel(const PfResampleArgs g)
{
    __shared__ unsigned long long s[PF_WAVES];
    const int i = blockIdx.x * PF_THREADS + threadIdx.x;
    unsigned long long v = i < g.E ? g.q[i] : 0ull;
    const unsigned long long total = pf_block_scan(v, s);
    if (i < g.E) g.C[i] = v;
    if (threadIdx.x == 0) g.block_sum[blockIdx.x] = total;
}

// one workgroup: the block sums to exclusive offsets, PF_THREADS at a time with a carry
__global__ __launch_bounds__(PF_THREADS) void simplyp_pf_scan_sums_kernel(const PfResampleArgs g)
{
    __shared__ unsigned long long s[PF_WAVES];
    unsigned long long carry = 0;
    for (int b0 = 0; b0 < g.n_blocks; b0 += PF_THREADS) {
        const int b = b0 + threadIdx.x;
        const unsigned long long own = b < g.n_blocks ? g.block_sum[b] : 0ull;
        unsigned long long v = own;
        const unsigned long long total = pf_block_scan(v, s);
        if (b < g.n_blocks) g.block_sum[b] = carry + (v - own);
        carry += total;
    }
}

__global__ __launch_bounds__(PF_THREADS) void simplyp_pf_scan_add_kernel(const PfResampleArgs g)
{
    const int i = blockIdx.x * PF_THREADS + threadIdx.x;
    if (i >= g.E) return;
    const unsigned long long c = g.C[i] + g.block_sum[blockIdx.x];
    g.C[i] = c;
    if (i == g.E - 1) g.res->T = c;
}

__global__ __launch_bounds__(PF_THREADS) void simplyp_pf_search_kernel(const PfResampleArgs g)
{
    const int k = blockIdx.x * PF_THREADS + threadIdx.x;
    if (k >= g.E) return;
    const unsigned long long T = g.C[g.E - 1];
    if (T == 0) { g.ancestors[k] = k; return; }            // every particle is dead: the identity, and the caller's to report
    const Philox4 x = philox4x32_10(g.t, 0u, 0u, PF_STREAM_RESAMPLE, g.key0, g.key1);
    const uint64_t r = simplyp_resample::offset(((uint64_t)x.x0 << 32) | x.x1, T);
    g.ancestors[k] = simplyp_resample::ancestor((const uint64_t*)g.C, g.E, k, T, r);
}

// The first particle of every run of equal ancestors counts the run: n_unique, and the ancestor's offspring.
__global__ __launch_bounds__(PF_THREADS) void simplyp_pf_offspring_kernel(const PfResampleArgs g)
{
    const int k = blockIdx.x * PF_THREADS + threadIdx.x;
    if (k >= g.E || g.C[g.E - 1] == 0) return;
    const int a = g.ancestors[k];
    const bool first = k == 0 || g.ancestors[k - 1] != a;
    mcmc_count(&g.res->n_unique, first);
    if (!first || !g.offspring) return;
    int lo = k + 1, hi = g.E;                              // the first k' > k with another ancestor lies in [lo, hi]
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (g.ancestors[mid] != a) hi = mid; else lo = mid + 1;
    }
    g.offspring[a] = lo - k;
}

// ---- moving the particles ---------------------------------------------------------------------------------------------------------
struct PfGatherArgs {
    int E;
    long long n_rows;
    const int32_t* ancestors;              // [E]
    const unsigned long long* src;         // [n_rows][E] 8-byte words
    unsigned long long* dst;               // [n_rows][E]
    PfResult* res;
};

// grid: (particle blocks, row blocks of PF_GATHER_ROWS (strided))
__global__ __launch_bounds__(PF_THREADS) void simplyp_gather_members_kernel(const PfGatherArgs g)
{
    const int k = blockIdx.x * PF_THREADS + threadIdx.x;
    if (k >= g.E) return;
    const int a = g.ancestors[k];
    const bool ok = (unsigned)a < (unsigned)g.E;           // an ancestor outside [0, E) is never dereferenced
    if (blockIdx.y == 0) mcmc_count(&g.res->n_bad, !ok);
    const size_t from = ok ? (size_t)a : 0;
    for (long long r0 = (long long)blockIdx.y * PF_GATHER_ROWS; r0 < g.n_rows; r0 += (long long)gridDim.y * PF_GATHER_ROWS) {
        unsigned long long v[PF_GATHER_ROWS];
#pragma unroll
        for (int j = 0; j < PF_GATHER_ROWS; ++j) {
            const long long row = r0 + j < g.n_rows ? r0 + j : g.n_rows - 1;
            v[j] = g.src[(size_t)row * g.E + from];
        }
#pragma unroll
        for (int j = 0; j < PF_GATHER_ROWS; ++j)
            if (r0 + j < g.n_rows) g.dst[(size_t)(r0 + j) * g.E + k] = ok ? v[j] : 0x7ff8000000000000ull;
    }
}

struct PfJitterArgs {
    int E, n_dim;
    uint32_t key0, key1, t;
    double a;
    double centre[PF_MAX_DIM], scale[PF_MAX_DIM], lo[PF_MAX_DIM], hi[PF_MAX_DIM];
    int target[PF_MAX_DIM];
    double* theta;                         // [n_dim][E], in place
    double* member_params;                 // [NP_M][E]
    double* f_tdp;                         // [E]
    PfResult* res;
};

__device__ __forceinline__ double pf_jitter_value(const PfJitterArgs& g, int d, int k, double x)
{
    const double z = philox_normal((uint32_t)k, g.t, (uint32_t)d, PF_STREAM_JITTER, g.key0, g.key1);
    return (g.centre[d] + g.a * (x - g.centre[d])) + g.scale[d] * z;
}

__global__ __launch_bounds__(PF_THREADS) void simplyp_pf_jitter_kernel(const PfJitterArgs g)
{
    const int k = blockIdx.x * PF_THREADS + threadIdx.x;
    if (k >= g.E) return;
    bool in = true;
    for (int d = 0; d < g.n_dim; ++d) {
        const double y = pf_jitter_value(g, d, k, g.theta[(size_t)d * g.E + k]);
        in = in && (y >= g.lo[d]) && (y < g.hi[d]);        // NaN fails both
    }
    for (int d = 0; d < g.n_dim; ++d) {                    // the whole particle moves or stays
        const double x = g.theta[(size_t)d * g.E + k];
        const double v = in ? pf_jitter_value(g, d, k, x) : x;
        g.theta[(size_t)d * g.E + k] = v;
        const int tg = g.target[d];
        if (tg == MCMC_TARGET_F_TDP) g.f_tdp[k] = v;
        else if (tg != MCMC_TARGET_NONE) g.member_params[(size_t)tg * g.E + k] = v;
    }
    mcmc_count(&g.res->n_outside, !in);
}

}  // namespace simplyp
