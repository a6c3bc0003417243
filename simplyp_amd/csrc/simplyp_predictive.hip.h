// simplyp_predictive.hip.h -- the series a predictive band is selected from, with the error model drawn on the device (gfx950).
//
// The reference's ensemble caller (Development/2016/MCMC.ipynb, get_uncertainty_intervals) returns two bands per series: the
// percentiles over the members of the simulated series ("param_only"), and the same after sim + norm.rvs(loc=0, scale=m*sim)
// has been added to every member's series ("overall").  This kernel writes those series for a block of days into a table
// [n_series][days][R][E] in slot order -- the layout quantile_sort_kernel / quantile_select_kernel read -- or the normals alone.
//
// A series is a column of the run's table as it stands, or one of the six df_R series computed with tq_value<KIND>
// (simplyp_time_quantile.hip.h): the reference's expressions, operation for operation.
//
// The draw is counter-based: z is a pure function of (seed, member, absolute day, model reach, series id) and of nothing else --
// not of the launch shape, the slot the member sits in, the chunk of days, the window or the time.
//   generator  Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11)
//   key        (seed & 0xffffffff, seed >> 32)
//   counter    (member id, day0 + d, out_reaches[r], series id as passed: SIMPLYP_OUT_c or SIMPLYP_TQ_DERIVED + SIMPLYP_GOF_v)
//   uniforms   h1 = ((x0 << 32) | x1) >> 12, u1 = (h1 + 0.5) 2^-52; h2, u2 from x2, x3: exact in fp64, u in (0, 1)
//   normal     z = sqrt(-2 ln u1) cospi(2 u2): one per call (the sine branch is not kept), |z| <= 8.58
//   model      v' = v + (m v) z: two multiplies and an add (the library is built with -ffp-contract=off)
// The Philox state is 32-bit integer arithmetic on six registers; simplyp_amd/predictive.py restates all of it in NumPy.
//
// Layout: lane = member slot, one (day, series, reach) row segment per workgroup step, so every load and store of a wave is a
// full 512-byte segment; member_of_slot, f_tdp, A_catch and err_m are read once per lane, in member order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simplyp.h"
#include "simplyp_kernels.hip.h"           // sp_log
#include "simplyp_time_quantile.hip.h"     // TqSeries, tq_series, tq_value

namespace simplyp {

constexpr int PRED_MAX_SERIES = TQ_MAX_SERIES;
constexpr int PRED_THREADS = 256;
constexpr int PRED_BATCH = 4;              // day rows whose loads are issued together

struct PredArgs {
    int E, R, n_series;
    int d_lo, n_days;                      // the block of days [d_lo, d_lo + n_days) of the run's table
    const double* out;                     // [n_cols][D][R][E]
    long long col_stride;                  // D*R*E
    int col[4];                            // column slots of Qr, Msus_kg/day, TDP_kg/day, PP_kg/day (derived series only)
    int series[PRED_MAX_SERIES];           // >= 0: column slot; < 0: derived, -1 - SIMPLYP_GOF_*
    uint32_t series_id[PRED_MAX_SERIES];   // the id as passed: the counter's fourth word
    const int32_t* member_of_slot;         // [E] or nullptr
    const double* f_tdp;                   // [E] member order (derived only)
    const double* a_catch;                 // [S][E] member order (derived only)
    const double* err_m;                   // [n_series][E] member order, or nullptr: no draws
    const int32_t* reach_of;               // [R] device
    uint32_t key0, key1;
    uint32_t day0;                         // absolute index of the table's day 0
    int normals;                           // 1: write z instead of the values
    double* dst;                           // [n_series][n_days][R][E]
};

struct Philox4 { uint32_t x0, x1, x2, x3; };

__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1;
        c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    }
    return Philox4{c0, c1, c2, c3};
}

__device__ __forceinline__ double philox_uniform(uint32_t hi, uint32_t lo)
{
    const unsigned long long h = (((unsigned long long)hi << 32) | lo) >> 12;
    return ((double)h + 0.5) * 0x1p-52;                    // both exact: h < 2^52
}

__device__ __forceinline__ double philox_normal(uint32_t member, uint32_t day, uint32_t reach, uint32_t series, uint32_t k0, uint32_t k1)
{
    const Philox4 x = philox4x32_10(member, day, reach, series, k0, k1);
    const double u1 = philox_uniform(x.x0, x.x1), u2 = philox_uniform(x.x2, x.x3);
    return sqrt(-2.0 * sp_log(u1)) * cospi(2.0 * u2);
}

// One lane's (series, reach) through the block's days.  DRAW 0: v; 1: v + (m v) z; 2: z.
template <int KIND, int DRAW>
__device__ __forceinline__ void pred_days(const PredArgs& g, const TqSeries& sr, double m, uint32_t member, uint32_t reach,
                                          uint32_t series, double* dst)
{
    const size_t day_stride = (size_t)g.R * g.E;
    for (int d0 = blockIdx.y * PRED_BATCH; d0 < g.n_days; d0 += gridDim.y * PRED_BATCH) {
        double a[PRED_BATCH], b[PRED_BATCH], c[PRED_BATCH];
#pragma unroll
        for (int j = 0; j < PRED_BATCH; ++j) {
            const size_t off = (size_t)(g.d_lo + min(d0 + j, g.n_days - 1)) * day_stride;
            a[j] = DRAW != 2 ? sr.p0[off] : 0.0;
            b[j] = DRAW != 2 && KIND >= 2 ? sr.p1[off] : 0.0;
            c[j] = DRAW != 2 && KIND == 3 ? sr.p2[off] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < PRED_BATCH; ++j) {
            double v = DRAW != 2 ? tq_value<KIND>(sr, a[j], b[j], c[j]) : 0.0;
            if (DRAW != 0) {
                const double z = philox_normal(member, g.day0 + (uint32_t)(g.d_lo + d0 + j), reach, series, g.key0, g.key1);
                v = DRAW == 2 ? z : v + (m * v) * z;
            }
            if (d0 + j < g.n_days) dst[(size_t)(d0 + j) * day_stride] = v;
        }
    }
}

// grid: (member blocks of PRED_THREADS, day batches (strided), n_series * R)
__global__ __launch_bounds__(PRED_THREADS) void simplyp_predictive_kernel(const PredArgs g)
{
    const int slot = blockIdx.x * PRED_THREADS + threadIdx.x;
    if (slot >= g.E) return;                               // no barrier below
    const int si = blockIdx.z / g.R, r = blockIdx.z - si * g.R;
    const int code = g.series[si];
    const bool draw = g.err_m != nullptr;
    int member = g.member_of_slot && (code < 0 || draw) ? g.member_of_slot[slot] : slot;
    if ((unsigned)member >= (unsigned)g.E) member = slot;  // a map that is no permutation reads nothing out of bounds
    const int reach = g.reach_of[r];
    const size_t base = (size_t)r * g.E + slot;
    double* dst = g.dst + ((size_t)si * g.n_days * g.R + r) * g.E + slot;
    const double m = draw ? g.err_m[(size_t)si * g.E + member] : 0.0;
    const uint32_t sid = g.series_id[si];
    if (g.normals) {
        pred_days<0, 2>(g, TqSeries{}, m, (uint32_t)member, (uint32_t)reach, sid, dst);
        return;
    }
    TqSeries sr;
    const int kind = tq_series(sr, code, g.out, g.col_stride, g.col, base, g.a_catch, g.f_tdp, (size_t)reach * g.E + member, member);
    if (draw) {
        if (kind == 0) pred_days<0, 1>(g, sr, m, (uint32_t)member, (uint32_t)reach, sid, dst);
        else if (kind == 1) pred_days<1, 1>(g, sr, m, (uint32_t)member, (uint32_t)reach, sid, dst);
        else if (kind == 2) pred_days<2, 1>(g, sr, m, (uint32_t)member, (uint32_t)reach, sid, dst);
        else pred_days<3, 1>(g, sr, m, (uint32_t)member, (uint32_t)reach, sid, dst);
    } else {
        if (kind == 0) pred_days<0, 0>(g, sr, m, (uint32_t)member, (uint32_t)reach, sid, dst);
        else if (kind == 1) pred_days<1, 0>(g, sr, m, (uint32_t)member, (uint32_t)reach, sid, dst);
        else if (kind == 2) pred_days<2, 0>(g, sr, m, (uint32_t)member, (uint32_t)reach, sid, dst);
        else pred_days<3, 0>(g, sr, m, (uint32_t)member, (uint32_t)reach, sid, dst);
    }
}

}  // namespace simplyp
