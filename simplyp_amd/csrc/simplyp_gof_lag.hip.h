// simplyp_gof_lag.hip.h -- per-member lag-one sums of the relative residuals over the daily reach outputs (gfx950).
//
// What it serves: the autocorrelation check the reference's calibration notebook ends with (Development/2016/MCMC.ipynb, cell 21)
// for every member of an ensemble, and an AR(1) error model for the calibration calls (simplyp_mcmc_log_prob_ar1).  With
// r_t = obs_t / sim_t - 1 -- the quantity SIMPLYP_GOFSTAT_SUM_RELSQ squares -- a paired row t (observation and simulated value
// both non-NaN: simplyp_gof's rule) is LINKED when row t - 1 of the table is paired too, for this member and this variable.  Over
// the linked rows:
//     n_link,   A = sum r_t^2,   B = sum r_{t-1}^2,   C = sum r_t r_{t-1}.
// A paired row that is not linked starts a new segment: the model these sums serve treats segments as independent (the exact
// treatment of a gap of g days needs phi^g, which does not factorise into sums).  A NaN simulated value breaks the links on both
// sides of it, for that member only.
//
// Layout: simplyp_gof's.  Lane = member slot, so every wave load is one 512-byte row segment; the wave-uniform day lists are the
// ones simplyp_gof compacts, each entry with one more flag -- it is the calendar successor of the entry before it --; a discharge
// pass reads the Qr row only, a chemistry pass Qr and the three flux rows; the lists are cut into chunks along blockIdx.y by
// simplyp_gof's rule; partial sums go through a [chunk][reach][6 * 4][E] table that a finish kernel adds in chunk order.  A chunk
// is walked in day order with the previous row's r and its validity per lane and variable in registers, so inside a segment each
// row is read once; a chunk whose first entry is a successor loads the entry before it first -- one more row (four for chemistry)
// per chunk, the only re-read.  The simulated series and r come from simplyp_gof.hip.h's device functions: the same bits.
// The chemistry pass is one pass: 5 variables x (previous r, 4 sums) = 25 doubles per lane, far inside the 512 VGPRs a one-wave
// workgroup may use.  No atomics, no scratch, no LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simplyp_residuals.h"
#include "simplyp_gof.hip.h"         // GofArgs, gof_rel, gof_chem_sim, gof_q_scale, the batch sizes

namespace simplyp {

constexpr int LAG_NACC = SIMPLYP_N_LAG_STATS;

struct GofLagArgs {
    GofArgs g;                         // the table, the lists, the chunk counts; g.partial is [chunk][R][6 * 4][E] here, g.gof unused
    const int32_t* q_succ;             // per entry of g.q_day: 1 when it is the day after the entry before it (same reach)
    const int32_t* c_succ;             // the same for g.c_day
    double* lag;                       // [SIMPLYP_N_LAG_STATS][6][R][E], member order
};

struct LagAcc {
    double a[LAG_NACC];                // n_link, A, B, C
    double prev;                       // r of the entry before this one
    bool prev_ok;                      // ... which was paired
};

__device__ __forceinline__ void lag_clear(LagAcc& L)
{
#pragma unroll
    for (int j = 0; j < LAG_NACC; ++j) L.a[j] = 0.0;
    L.prev = 0.0; L.prev_ok = false;
}

// One entry of one variable.  have: the variable has an observation `o` here (wave-uniform); succ: the entry is the day after
// the previous entry (wave-uniform); s: simulated value (per lane; NaN drops the pair, as in gof_add).  ADD == false only carries
// r forward: a chunk's predecessor row.
template <bool ADD>
__device__ __forceinline__ void lag_step(LagAcc& L, bool have, bool succ, double o, double s)
{
    const bool ok = have && s == s;
    double r = 0.0;
    if (ok) {
        double ls;
        r = gof_rel(o, s, ls);
    }
    if (ADD && ok && succ && L.prev_ok) {
        L.a[SIMPLYP_LAGSTAT_N_LINK] += 1.0;
        L.a[SIMPLYP_LAGSTAT_SQ_HEAD] = __builtin_fma(r, r, L.a[SIMPLYP_LAGSTAT_SQ_HEAD]);
        L.a[SIMPLYP_LAGSTAT_SQ_TAIL] = __builtin_fma(L.prev, L.prev, L.a[SIMPLYP_LAGSTAT_SQ_TAIL]);
        L.a[SIMPLYP_LAGSTAT_CROSS] = __builtin_fma(r, L.prev, L.a[SIMPLYP_LAGSTAT_CROSS]);
    }
    L.prev = r; L.prev_ok = ok;
}

template <bool ADD>
__device__ __forceinline__ void lag_chem_day(LagAcc (&acc)[GOF_NV], const double* ob, bool succ, double qr, double ms, double td,
                                             double pp, double A, double f_tdp)
{
    double SS, TDP, PP, TP, SRP;
    gof_chem_sim(qr, ms, td, pp, A, f_tdp, SS, TDP, PP, TP, SRP);
    lag_step<ADD>(acc[SIMPLYP_GOF_SS], ob[0] == ob[0], succ, ob[0], SS);
    lag_step<ADD>(acc[SIMPLYP_GOF_TDP], ob[1] == ob[1], succ, ob[1], TDP);
    lag_step<ADD>(acc[SIMPLYP_GOF_PP], ob[2] == ob[2], succ, ob[2], PP);
    lag_step<ADD>(acc[SIMPLYP_GOF_TP], ob[3] == ob[3], succ, ob[3], TP);
    lag_step<ADD>(acc[SIMPLYP_GOF_SRP], ob[4] == ob[4], succ, ob[4], SRP);
}

// PART 0: discharge days; PART 1: chemistry days -- as simplyp_gof_partial_kernel, whose chunk bounds these are.
template <int PART>
__global__ __launch_bounds__(64) void simplyp_gof_lag_partial_kernel(const GofLagArgs a)
{
    const GofArgs& g = a.g;
    const int slot = blockIdx.x * 64 + threadIdx.x;
    const int chunk = blockIdx.y, r = blockIdx.z;
    if (slot >= g.E) return;
    const int member = g.member_of_slot ? g.member_of_slot[slot] : slot;
    const double A = g.a_catch ? g.a_catch[(size_t)g.reach_of[r] * g.E + member] : 86.4;
    const size_t day_stride = (size_t)g.R * g.E;
    const double* qr_col = g.out + (size_t)g.col[0] * g.col_stride + (size_t)r * g.E + slot;
    double* p = g.partial + ((size_t)chunk * g.R + r) * (GOF_NV * LAG_NACC) * g.E + slot;

    if constexpr (PART == 0) {
        LagAcc acc;
        lag_clear(acc);
        const long long k0 = g.q_ptr[r], n = g.q_ptr[r + 1] - k0;
        const int kb = (int)(k0 + n * chunk / g.n_chunks_q), ke = (int)(k0 + n * (chunk + 1) / g.n_chunks_q);
        const double q_scale = gof_q_scale(g.a_catch != nullptr, A);
        // a successor implies an entry before it in this reach's list (the host clears the flag of a list's first entry)
        if (kb < ke && a.q_succ[kb])
            lag_step<false>(acc, true, false, g.q_obs[4 * (kb - 1)], qr_col[(size_t)g.q_day[kb - 1] * day_stride] * q_scale);
        int k = kb;
        for (; k + GOF_BATCH_Q <= ke; k += GOF_BATCH_Q) {          // all row loads of a batch before the first is consumed, as in simplyp_gof
            double qv[GOF_BATCH_Q];
#pragma unroll
            for (int j = 0; j < GOF_BATCH_Q; ++j) qv[j] = qr_col[(size_t)g.q_day[k + j] * day_stride];
#pragma unroll
            for (int j = 0; j < GOF_BATCH_Q; ++j)
                lag_step<true>(acc, true, a.q_succ[k + j] != 0, g.q_obs[4 * (k + j)], qv[j] * q_scale);
        }
        for (; k < ke; ++k)
            lag_step<true>(acc, true, a.q_succ[k] != 0, g.q_obs[4 * k], qr_col[(size_t)g.q_day[k] * day_stride] * q_scale);
#pragma unroll
        for (int j = 0; j < LAG_NACC; ++j) p[(size_t)(SIMPLYP_GOF_Q * LAG_NACC + j) * g.E] = acc.a[j];
    } else {
        const double f_tdp = g.f_tdp[member];
        const double* ms_col = g.out + (size_t)g.col[1] * g.col_stride + (size_t)r * g.E + slot;
        const double* td_col = g.out + (size_t)g.col[2] * g.col_stride + (size_t)r * g.E + slot;
        const double* pp_col = g.out + (size_t)g.col[3] * g.col_stride + (size_t)r * g.E + slot;
        LagAcc acc[GOF_NV];
#pragma unroll
        for (int v = 1; v < GOF_NV; ++v) lag_clear(acc[v]);
        const long long k0 = g.c_ptr[r], n = g.c_ptr[r + 1] - k0;
        const int kb = (int)(k0 + n * chunk / g.n_chunks_c), ke = (int)(k0 + n * (chunk + 1) / g.n_chunks_c);
        if (kb < ke && a.c_succ[kb]) {
            const size_t off = (size_t)g.c_day[kb - 1] * day_stride;
            lag_chem_day<false>(acc, g.c_obs + (size_t)(kb - 1) * 20, false, qr_col[off], ms_col[off], td_col[off], pp_col[off], A, f_tdp);
        }
        int k = kb;
        for (; k + GOF_BATCH_C <= ke; k += GOF_BATCH_C) {
            double qv[GOF_BATCH_C], mv[GOF_BATCH_C], tv[GOF_BATCH_C], pv[GOF_BATCH_C];
#pragma unroll
            for (int j = 0; j < GOF_BATCH_C; ++j) {
                const size_t off = (size_t)g.c_day[k + j] * day_stride;
                qv[j] = qr_col[off]; mv[j] = ms_col[off]; tv[j] = td_col[off]; pv[j] = pp_col[off];
            }
#pragma unroll
            for (int j = 0; j < GOF_BATCH_C; ++j)
                lag_chem_day<true>(acc, g.c_obs + (size_t)(k + j) * 20, a.c_succ[k + j] != 0, qv[j], mv[j], tv[j], pv[j], A, f_tdp);
        }
        for (; k < ke; ++k) {
            const size_t off = (size_t)g.c_day[k] * day_stride;
            lag_chem_day<true>(acc, g.c_obs + (size_t)k * 20, a.c_succ[k] != 0, qr_col[off], ms_col[off], td_col[off], pp_col[off], A, f_tdp);
        }
#pragma unroll
        for (int v = 1; v < GOF_NV; ++v)
#pragma unroll
            for (int j = 0; j < LAG_NACC; ++j) p[(size_t)(v * LAG_NACC + j) * g.E] = acc[v].a[j];
    }
}

__global__ __launch_bounds__(64) void simplyp_gof_lag_finish_kernel(const GofLagArgs a)
{
    const GofArgs& g = a.g;
    const int slot = blockIdx.x * 64 + threadIdx.x;
    const int r = blockIdx.y, v = blockIdx.z;
    if (slot >= g.E) return;
    const int member = g.member_of_slot ? g.member_of_slot[slot] : slot;
    double s[LAG_NACC];
#pragma unroll
    for (int j = 0; j < LAG_NACC; ++j) s[j] = 0.0;
    const int n_chunks = v == SIMPLYP_GOF_Q ? g.n_chunks_q : g.n_chunks_c;
    for (int c = 0; c < n_chunks; ++c) {
        const double* p = g.partial + (((size_t)c * g.R + r) * (GOF_NV * LAG_NACC) + (size_t)v * LAG_NACC) * g.E + slot;
#pragma unroll
        for (int j = 0; j < LAG_NACC; ++j) s[j] += p[(size_t)j * g.E];
    }
    const bool use = g.n_obs[r * GOF_NV + v] > 10.0;                 // simplyp_gof's rule (visualise_results.py:430)
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
#pragma unroll
    for (int j = 0; j < LAG_NACC; ++j)
        a.lag[(((size_t)j * GOF_NV + v) * g.R + r) * g.E + member] = use ? s[j] : nan;
}

}  // namespace simplyp
