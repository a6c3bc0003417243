// simplyp_mcmc.hip.h -- the affine-invariant stretch move (Goodman & Weare 2010) on the device (gfx950): what the reference's
// calibration notebook does with emcee.EnsembleSampler(n_walk, n_dim, log_posterior).run_mcmc (Development/2016/MCMC.ipynb, cell 10).
//
// W walkers (W even) in two halves of h = W / 2.  A step t moves half 0 against the positions of half 1, then half 1 against the
// new positions of half 0.  One half-step is three kernels with a model run between the first two:
//   simplyp_mcmc_propose_kernel   y = x_j + z (x_i - x_j), the prior box lo <= y < hi, the run point scattered into the run's arrays
//   (simplyp_run, simplyp_gof)    the model at the run point of every active walker: an ensemble of h members
//   simplyp_mcmc_log_prob_kernel  the Gaussian log-likelihood with sigma = m sim from the goodness-of-fit table
//   simplyp_mcmc_accept_kernel    accept iff inside and (n_dim - 1) ln z + lp_y - lp_i - ln u_a > 0
// The run point is the proposal where it lies inside the box and the walker's current position where it does not: the model never
// sees a point outside the prior's support, where it need not be defined (negative time constants, land-use fractions past 1).
//
// The draws are counter-based (Philox4x32-10, simplyp_predictive.hip.h), a pure function of (seed, walker, absolute step):
//   draw A   key (seed & 0xffffffff, seed >> 32), counter (i, t, 0, 0x4D434D43): u_z = uniform(x0, x1), partner j = c + ((x2 h) >> 32)
//            with c = (1 - half) h; s = (a - 1) u_z + 1, z = (s s) / a: emcee's g(z) on [1/a, a]
//   draw B   counter (i, t, 1, 0x4D434D43): u_a = uniform(x0, x1)
// Everything but ln z and ln u_a is integer arithmetic or + * / in fp64 (the library is built with -ffp-contract=off), so partner,
// z, y and the box test match simplyp_amd/mcmc.py bit for bit; the accept kernel recomputes z from the counter.
//
// Layout: lane = active walker; theta [n_dim][W], prop [n_dim][h] and the run's arrays are SoA, so every load and store of a wave
// is one contiguous segment; the partner read is a gather.  No LDS, no barrier, no per-lane arrays.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simplyp.h"
#include "../../include/simplyp_residuals.h"    // SIMPLYP_LAGSTAT_*
#include "simplyp_kernels.hip.h"           // sp_log
#include "simplyp_predictive.hip.h"        // philox4x32_10, philox_uniform

namespace simplyp {

constexpr int MCMC_MAX_DIM = 16;
constexpr int MCMC_MAX_PAIRS = 32;
constexpr int MCMC_THREADS = 256;
constexpr uint32_t MCMC_STREAM = 0x4D434D43u;          // "MCMC": the counter's fourth word
constexpr int MCMC_TARGET_F_TDP = -1, MCMC_TARGET_NONE = -2;

struct McmcMove {
    int W, h, n_dim, half;
    double a;
    uint32_t key0, key1, t;
};

struct McmcProposeArgs {
    McmcMove mv;
    double lo[MCMC_MAX_DIM], hi[MCMC_MAX_DIM];
    int target[MCMC_MAX_DIM];
    const double* theta;                   // [n_dim][W]
    double* prop;                          // [n_dim][h]
    int32_t* inside;                       // [h]
    double* member_params;                 // [NP_M][h]
    double* f_tdp;                         // [h]
    unsigned* counters;                    // [4]: inside, accepted, NaN
};

struct McmcLogProbArgs {
    int h, R, n_pairs;
    int pair_var[MCMC_MAX_PAIRS], pair_reach[MCMC_MAX_PAIRS];
    int m_dim[SIMPLYP_N_GOF_VARS];         // row of prop that holds the variable's m, or -1: m_const
    double m_const[SIMPLYP_N_GOF_VARS];
    const double* gof;                     // [N_GOF_STATS][N_GOF_VARS][R][h]
    const int32_t* status;                 // [h] or nullptr
    const int32_t* inside;                 // [h] or nullptr
    const double* prop;                    // [n_dim][h]
    double* lp_prop;                       // [h]
    unsigned* counters;
};

struct McmcAcceptArgs {
    McmcMove mv;
    const double* prop;                    // [n_dim][h]
    const int32_t* inside;                 // [h]
    const double* lp_prop;                 // [h]
    double* theta;                         // [n_dim][W]
    double* lp;                            // [W]
    int32_t* n_accept;                     // [W]
    double* chain_row;                     // [n_dim + 1][W] or nullptr
    unsigned* counters;
};

// The stretch factor of walker i at step t, and the partner's offset within the other half.
__device__ __forceinline__ double mcmc_stretch(const McmcMove& mv, uint32_t i, uint32_t& partner)
{
    const Philox4 x = philox4x32_10(i, mv.t, 0u, MCMC_STREAM, mv.key0, mv.key1);
    const double u_z = philox_uniform(x.x0, x.x1);
    partner = (uint32_t)(((unsigned long long)x.x2 * (unsigned long long)mv.h) >> 32);
    const double s = (mv.a - 1.0) * u_z + 1.0;
    return (s * s) / mv.a;
}

// The lanes that raise `flag`, counted (the compiler folds a wave's increments into one atomic).
__device__ __forceinline__ void mcmc_count(unsigned* counter, bool flag)
{
    if (flag) atomicAdd(counter, 1u);
}

__global__ __launch_bounds__(MCMC_THREADS) void simplyp_mcmc_propose_kernel(const McmcProposeArgs g)
{
    const int k = blockIdx.x * MCMC_THREADS + threadIdx.x;
    if (k >= g.mv.h) return;
    const int W = g.mv.W, h = g.mv.h;
    const int i = g.mv.half * h + k;
    uint32_t partner;
    const double z = mcmc_stretch(g.mv, (uint32_t)i, partner);
    const int j = (1 - g.mv.half) * h + (int)partner;      // partner < h: (x2 h) >> 32 with x2 < 2^32
    bool in = true;
    for (int d = 0; d < g.mv.n_dim; ++d) {
        const double xi = g.theta[(size_t)d * W + i], xj = g.theta[(size_t)d * W + j];
        const double y = xj + z * (xi - xj);
        g.prop[(size_t)d * h + k] = y;
        in = in && (y >= g.lo[d]) && (y < g.hi[d]);        // NaN fails both
    }
    g.inside[k] = in ? 1 : 0;
    for (int d = 0; d < g.mv.n_dim; ++d) {                 // the run point: y inside the box, the current position outside
        const int tg = g.target[d];
        if (tg == MCMC_TARGET_NONE) continue;
        const double xi = g.theta[(size_t)d * W + i], xj = g.theta[(size_t)d * W + j];
        const double y = xj + z * (xi - xj);
        const double v = in ? y : xi;
        if (tg == MCMC_TARGET_F_TDP) g.f_tdp[k] = v;
        else g.member_params[(size_t)tg * h + k] = v;
    }
    mcmc_count(g.counters + 0, in);
}

__global__ __launch_bounds__(MCMC_THREADS) void simplyp_mcmc_log_prob_kernel(const McmcLogProbArgs g)
{
    const int k = blockIdx.x * MCMC_THREADS + threadIdx.x;
    if (k >= g.h) return;
    const size_t var_stride = (size_t)g.R * g.h, stat_stride = (size_t)SIMPLYP_N_GOF_VARS * var_stride;
    double sum = 0.0;
    bool m_ok = true;
    for (int p = 0; p < g.n_pairs; ++p) {
        const int v = g.pair_var[p];
        const double m = g.m_dim[v] >= 0 ? g.prop[(size_t)g.m_dim[v] * g.h + k] : g.m_const[v];
        const size_t at = (size_t)v * var_stride + (size_t)g.pair_reach[p] * g.h + k;
        const double n = g.gof[(size_t)SIMPLYP_GOFSTAT_N_OBS * stat_stride + at];
        const double sls = g.gof[(size_t)SIMPLYP_GOFSTAT_SUM_LOG_SIM * stat_stride + at];
        const double srq = g.gof[(size_t)SIMPLYP_GOFSTAT_SUM_RELSQ * stat_stride + at];
        m_ok = m_ok && (m > 0.0);
        // visualise_results.loglik: -0.5 n ln(2 pi) - n ln m - sum_log_sim - sum_relsq / (2 m m), left to right
        const double lm = m > 0.0 ? sp_log(m) : 0.0;
        const double term = (((-0.5 * n) * 1.8378770664093453) - n * lm - sls) - srq / ((2.0 * m) * m);
        sum = p == 0 ? term : sum + term;
    }
    const bool in = g.inside ? g.inside[k] != 0 : true;
    const bool finite_run = g.status ? (g.status[k] & SIMPLYP_STATUS_NONFINITE) == 0 : true;
    const bool is_nan = sum != sum;
    g.lp_prop[k] = (in && finite_run && m_ok && !is_nan) ? sum : -__builtin_huge_val();
    mcmc_count(g.counters + 0, in);
    mcmc_count(g.counters + 2, is_nan);
}

// The same with an AR(1) error model along linked rows (simplyp_gof_lag.hip.h; simplyp_amd/residuals.py states it): per pair
//     s = (1 - phi)(1 + phi),  q = SUM_RELSQ + ((phi phi)(A + B) - (2 phi) C) / s,
//     -0.5 n ln(2 pi) - n ln m - sum_log_sim - q / (2 m m) - 0.5 n_link ln s,          left to right.
// At phi = 0: s = 1, q = SUM_RELSQ + 0 / 1 and sp_log(1) = +0 exactly (f = 0 makes every term of it 0), so the term has the bits
// of simplyp_mcmc_log_prob_kernel's.
struct McmcLogProbAr1Args {
    McmcLogProbArgs b;
    int phi_dim[SIMPLYP_N_GOF_VARS];       // row of prop that holds the variable's phi, or -1: phi_const
    double phi_const[SIMPLYP_N_GOF_VARS];
    const double* lag;                     // [N_LAG_STATS][N_GOF_VARS][R][h]
};

__global__ __launch_bounds__(MCMC_THREADS) void simplyp_mcmc_log_prob_ar1_kernel(const McmcLogProbAr1Args a)
{
    const McmcLogProbArgs& g = a.b;
    const int k = blockIdx.x * MCMC_THREADS + threadIdx.x;
    if (k >= g.h) return;
    const size_t var_stride = (size_t)g.R * g.h, stat_stride = (size_t)SIMPLYP_N_GOF_VARS * var_stride;
    double sum = 0.0;
    bool m_ok = true, phi_ok = true;
    for (int p = 0; p < g.n_pairs; ++p) {
        const int v = g.pair_var[p];
        const double m = g.m_dim[v] >= 0 ? g.prop[(size_t)g.m_dim[v] * g.h + k] : g.m_const[v];
        const double phi_in = a.phi_dim[v] >= 0 ? g.prop[(size_t)a.phi_dim[v] * g.h + k] : a.phi_const[v];
        const size_t at = (size_t)v * var_stride + (size_t)g.pair_reach[p] * g.h + k;
        const double n = g.gof[(size_t)SIMPLYP_GOFSTAT_N_OBS * stat_stride + at];
        const double sls = g.gof[(size_t)SIMPLYP_GOFSTAT_SUM_LOG_SIM * stat_stride + at];
        const double srq = g.gof[(size_t)SIMPLYP_GOFSTAT_SUM_RELSQ * stat_stride + at];
        const double nl = a.lag[(size_t)SIMPLYP_LAGSTAT_N_LINK * stat_stride + at];
        const double A = a.lag[(size_t)SIMPLYP_LAGSTAT_SQ_HEAD * stat_stride + at];
        const double B = a.lag[(size_t)SIMPLYP_LAGSTAT_SQ_TAIL * stat_stride + at];
        const double Cx = a.lag[(size_t)SIMPLYP_LAGSTAT_CROSS * stat_stride + at];
        const bool in_range = phi_in > -1.0 && phi_in < 1.0;          // NaN fails both
        m_ok = m_ok && (m > 0.0);
        phi_ok = phi_ok && in_range;
        const double phi = in_range ? phi_in : 0.0;
        const double lm = m > 0.0 ? sp_log(m) : 0.0;
        const double s = (1.0 - phi) * (1.0 + phi);
        const double q = srq + ((phi * phi) * (A + B) - (2.0 * phi) * Cx) / s;
        const double term = ((((-0.5 * n) * 1.8378770664093453) - n * lm - sls) - q / ((2.0 * m) * m)) - (0.5 * nl) * sp_log(s);
        sum = p == 0 ? term : sum + term;
    }
    const bool in = g.inside ? g.inside[k] != 0 : true;
    const bool finite_run = g.status ? (g.status[k] & SIMPLYP_STATUS_NONFINITE) == 0 : true;
    const bool is_nan = sum != sum;
    g.lp_prop[k] = (in && finite_run && m_ok && phi_ok && !is_nan) ? sum : -__builtin_huge_val();
    mcmc_count(g.counters + 0, in);
    mcmc_count(g.counters + 2, is_nan);
}

__global__ __launch_bounds__(MCMC_THREADS) void simplyp_mcmc_accept_kernel(const McmcAcceptArgs g)
{
    const int k = blockIdx.x * MCMC_THREADS + threadIdx.x;
    if (k >= g.mv.h) return;
    const int W = g.mv.W, h = g.mv.h;
    const int i = g.mv.half * h + k;
    uint32_t partner;
    const double z = mcmc_stretch(g.mv, (uint32_t)i, partner);
    const Philox4 xb = philox4x32_10((uint32_t)i, g.mv.t, 1u, MCMC_STREAM, g.mv.key0, g.mv.key1);
    const double u_a = philox_uniform(xb.x0, xb.x1);
    const bool in = g.inside[k] != 0;
    const double lp_y = g.lp_prop[k], lp_i = g.lp[i];
    const double margin = (double)(g.mv.n_dim - 1) * sp_log(z) + lp_y - lp_i - sp_log(u_a);
    const bool is_nan = lp_y != lp_y;
    const bool acc = in && !is_nan && margin > 0.0;
    for (int d = 0; d < g.mv.n_dim; ++d) {
        const double v = acc ? g.prop[(size_t)d * h + k] : g.theta[(size_t)d * W + i];
        if (acc) g.theta[(size_t)d * W + i] = v;
        if (g.chain_row) g.chain_row[(size_t)d * W + i] = v;
    }
    const double lp_new = acc ? lp_y : lp_i;
    if (acc) { g.lp[i] = lp_new; g.n_accept[i] += 1; }
    if (g.chain_row) g.chain_row[(size_t)g.mv.n_dim * W + i] = lp_new;
    mcmc_count(g.counters + 0, in);
    mcmc_count(g.counters + 1, acc);
    mcmc_count(g.counters + 2, is_nan);
}

}  // namespace simplyp
