// simplyp_forcing.hip.h -- forcing uncertainty: every member's own forcing set, drawn on the device (gfx950).
//
// The run kernels already read a forcing set per lane (run_slot: `set`, per day when forcing_of_member is given).  This kernel
// makes such sets: the table [E][rows][D] -- the layout `forcing` has with n_forcing_sets = E -- from the caller's base sets
// [n_sets][rows][D] and forcing_of_member, before the pilot and the main launches of the same run (run_async_body).
//
// The error model (simplyp_amd/forcing.py restates it in NumPy; include/simplyp.h, simplyp_opts.forcing_*), for member e, row r
// (0 = P or Precipitation, 1 = PET, 2 = T_air with the snow module) and day d of group g = group_of_day[r][d]:
//   z      = philox_normal(member0 + e, g, r, SIMPLYP_FORCING_STREAM)        the stream of simplyp_predictive.hip.h
//   rows 0, 1:  v' = (v * scale[e]) * sp_exp(sigma z - 0.5 sigma sigma)      mean-one lognormal multiplier
//   row 2:      v' = (v + offset[e]) + sigma z
// in that order of operations (the library is built with -ffp-contract=off).  sigma = 0: no draw; no shift: no multiply / add, so
// the base value passes through bit for bit.  A draw is a pure function of (seed, member id, group id, row): not of the launch
// shape, the lane slot, the balancing, the time chunks, the window or the device block.
//
// Seasonal change factors (shift_groups = G >= 1): scale / offset is [rows][G][E] and day d reads the entry of its shift group
// shift_group[d] in [0, G) (forcing_shift_at below, shared by both kernels); G = 0 reads [rows][E] exactly as before.
//
// Autocorrelated errors (rho[r] > 0, simplyp_forcing_ar1_kernel): z of a row follows an AR(1) over consecutive groups.  Day d
// starts a step when its group id differs from the previous day's (for d = 0: from the incoming noise state's, "none" = -1
// without one).  At a step, with eps the very draw above,
//   z = eps                                    when there is no previous z (stationary start)
//   z = (rho * z_prev) + (c * eps)             otherwise, c = sqrt(1 - rho rho) rounded once on the host
// two products and one sum, each rounded; days that start no step reuse z.  The recurrence is DEFINED sequentially and is
// evaluated so: a scan over affine maps would round differently with the tile shape, and "windows laid end to end are the one
// call, bit for bit" would be lost.  The noise state [6][E] -- rows 0-2: z of P, PET, T_air; rows 3-5: that row's last group
// id as an exact double, -1.0 = none; 0.0 / -1.0 for a row without rho -- is read before the first day and written after the
// last one by the one wave that owns (member, row), so the same buffer may serve as input and output.
//
// Layout, both kernels: lanes run along d, one value per thread and row, so a wave's base-row loads and table stores are full
// 512-byte segments; member, shift (G = 0) and set are wave-uniform.  Write-bound streaming: one pass, nothing read twice, no
// LDS, no barrier.  The independent kernel: one member per block, a thread per day.  The AR(1) kernel: one wave per (member,
// row), walking the row in tiles of 64 days; every lane that starts a step draws its eps (Philox, log, sqrt, cospi: the
// expensive part, fully parallel), then the wave walks the tile's steps in day order -- a ballot of the step flags, one lane
// broadcast of eps per step, two multiplies and an add on wave-uniform values -- and hands each lane the z of its day; the
// carry (z, whether there is one) crosses tiles in registers.  Monthly groups cost two or three steps per tile, daily ones 64.
// The thread of a member's day 0 also writes the identity member -> set map the run kernels then read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simplyp.h"
#include "simplyp_kernels.hip.h"           // sp_exp
#include "simplyp_predictive.hip.h"        // philox_normal

namespace simplyp {

constexpr int FORCING_THREADS = 256;

struct ForcingErrorArgs {
    int E, D, rows;                        // rows: 2, or 3 with the snow module
    int day_blocks;                        // ceil(D / FORCING_THREADS): blockIdx.x = e * day_blocks + day block
    const double* base;                    // [n_sets][rows][D]
    const int32_t* forcing_of_member;      // [E] or nullptr (set 0)
    const int32_t* group[3];               // [D] each; nullptr where sigma == 0
    const double* shift;                   // [shift_rows][E], or [shift_rows][shift_groups][E]; or nullptr
    int shift_rows;
    int shift_groups;                      // G: 0, or >= 1 with shift_group
    const int32_t* shift_group;            // [D], ids in [0, G) (ids outside read the nearest end)
    double rho[3], c[3];                   // AR(1) kernel only: rho, sqrt(1 - rho rho)
    const double* noise_in;                // [6][E] or nullptr (stationary start)
    double* noise_out;                     // [6][E] or nullptr; may be noise_in
    double sigma[3];
    uint32_t key0, key1, member0;
    double* table;                         // [E][rows][D]
    int32_t* ident;                        // [E]: e
};

// The scale / offset of (row r, member e, day d).
__device__ __forceinline__ double forcing_shift_at(const ForcingErrorArgs& g, int r, int e, int d)
{
    if (g.shift_groups < 1) return g.shift[(size_t)r * g.E + e];
    const int sg = min(max(g.shift_group[d], 0), g.shift_groups - 1);
    return g.shift[((size_t)r * g.shift_groups + sg) * g.E + e];
}

// v' of a row from v, the shift and z (sigma > 0).
__device__ __forceinline__ double forcing_perturbed(int r, double v, double sigma, double z)
{
    return r < 2 ? v * sp_exp(sigma * z - 0.5 * sigma * sigma) : v + sigma * z;
}

__global__ __launch_bounds__(FORCING_THREADS) void simplyp_forcing_error_kernel(const ForcingErrorArgs g)
{
    const int e = (int)(blockIdx.x / (unsigned)g.day_blocks);
    const int d = (int)(blockIdx.x - (unsigned)e * (unsigned)g.day_blocks) * FORCING_THREADS + (int)threadIdx.x;
    if (e >= g.E || d >= g.D) return;                      // no barrier below
    const size_t D = (size_t)g.D;
    const int set = g.forcing_of_member ? g.forcing_of_member[e] : 0;
    const double* src = g.base + (size_t)set * g.rows * D + d;
    double* dst = g.table + (size_t)e * g.rows * D + d;
    if (d == 0) g.ident[e] = e;
#pragma unroll                                             // (r a constant: the argument block's arrays are read, not indexed)
    for (int r = 0; r < 3; ++r) {
        if (r >= g.rows) break;
        double v = src[(size_t)r * D];
        if (r < g.shift_rows) {
            const double sh = forcing_shift_at(g, r, e, d);
            v = r < 2 ? v * sh : v + sh;
        }
        const double sigma = g.sigma[r];
        if (sigma > 0.0) {
            const double z = philox_normal(g.member0 + (uint32_t)e, (uint32_t)g.group[r][d], (uint32_t)r, SIMPLYP_FORCING_STREAM,
                                           g.key0, g.key1);
            v = forcing_perturbed(r, v, sigma, z);
        }
        dst[(size_t)r * D] = v;
    }
}

constexpr int FORCING_WAVE = 64;
constexpr int FORCING_AR1_WAVES = FORCING_THREADS / FORCING_WAVE;     // waves, so (member, row) pairs, per block

__device__ __forceinline__ double forcing_lane_value(double v, int lane)        // lane: wave-uniform
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

// One row of one member through all days; r is a constant at every call, so the argument block's arrays are read, not indexed.
__device__ __forceinline__ void forcing_ar1_row(const ForcingErrorArgs& g, const int r, const int e, const int lane)
{
    const size_t D = (size_t)g.D;
    const int set = g.forcing_of_member ? g.forcing_of_member[e] : 0;
    const double* src = g.base + ((size_t)set * g.rows + r) * D;
    double* dst = g.table + ((size_t)e * g.rows + r) * D;
    const double sigma = g.sigma[r], rho = g.rho[r], c = g.c[r];
    const bool ar = rho > 0.0;                             // (host: then sigma > 0 and the row has its group ids)
    const int32_t* grp = g.group[r];
    const uint32_t member = g.member0 + (uint32_t)e;
    // the carry, wave-uniform: z of the last step and the id of the day before the tile's first (-1: none, and no z either)
    double z = 0.0;
    int prev_id = -1;
    if (ar && g.noise_in) {
        prev_id = (int)g.noise_in[(size_t)(3 + r) * g.E + e];
        z = g.noise_in[(size_t)r * g.E + e];
    }
    bool have = prev_id >= 0;
    for (int d0 = 0; d0 < g.D; d0 += FORCING_WAVE) {       // uniform trip count: a ballot and lane broadcasts below
        const int d = d0 + lane;
        const bool live = d < g.D;
        double v = 0.0;
        if (live) {
            v = src[d];
            if (r < g.shift_rows) {
                const double sh = forcing_shift_at(g, r, e, d);
                v = r < 2 ? v * sh : v + sh;
            }
        }
        if (sigma > 0.0) {
            const int id = live ? grp[d] : 0;
            double zd;
            if (!ar) {
                zd = live ? philox_normal(member, (uint32_t)id, (uint32_t)r, SIMPLYP_FORCING_STREAM, g.key0, g.key1) : 0.0;
            } else {
                const int before = !live ? id : d == 0 ? prev_id : grp[d - 1];
                const bool step = live && id != before;
                const double eps = step ? philox_normal(member, (uint32_t)id, (uint32_t)r, SIMPLYP_FORCING_STREAM, g.key0, g.key1) : 0.0;
                zd = z;                                    // lanes before the tile's first step continue the carry
                for (unsigned long long todo = __ballot(step); todo != 0ull; todo &= todo - 1ull) {
                    const int l = __builtin_ctzll(todo);   // the tile's steps in day order
                    const double eps_l = forcing_lane_value(eps, l);
                    z = have ? (rho * z) + (c * eps_l) : eps_l;
                    have = true;
                    if (lane >= l) zd = z;
                }
            }
            if (live) v = forcing_perturbed(r, v, sigma, zd);
        }
        if (live) dst[d] = v;
    }
    if (g.noise_out && lane == 0) {
        g.noise_out[(size_t)r * g.E + e] = ar ? z : 0.0;
        g.noise_out[(size_t)(3 + r) * g.E + e] = ar ? (double)grp[g.D - 1] : -1.0;
    }
}

// Any call with some rho > 0.  Writes the whole table; a row without rho comes out as the independent kernel writes it.
__global__ __launch_bounds__(FORCING_THREADS) void simplyp_forcing_ar1_kernel(const ForcingErrorArgs g)
{
    const int lane = (int)(threadIdx.x & (FORCING_WAVE - 1));
    const long long w = (long long)blockIdx.x * FORCING_AR1_WAVES + (int)(threadIdx.x / FORCING_WAVE);    // (member, row), row fastest
    const int e = __builtin_amdgcn_readfirstlane((int)(w / g.rows));             // one wave, one (member, row): uniform
    if (e >= g.E) return;                                  // whole waves; no barrier below
    const int r = __builtin_amdgcn_readfirstlane((int)(w - (long long)e * g.rows));
    if (r == 0) {
        if (lane == 0) {
            g.ident[e] = e;
            if (g.rows < 3 && g.noise_out) { g.noise_out[(size_t)2 * g.E + e] = 0.0; g.noise_out[(size_t)5 * g.E + e] = -1.0; }
        }
        forcing_ar1_row(g, 0, e, lane);
    } else if (r == 1) {
        forcing_ar1_row(g, 1, e, lane);
    } else {
        forcing_ar1_row(g, 2, e, lane);
    }
}

}  // namespace simplyp
