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
// Layout: lanes run along d, one value per thread and row, so a wave's base-row loads and table stores are full 512-byte
// segments; member, shift and set are block-uniform.  Write-bound streaming: one pass, nothing read twice, no LDS, no barrier.
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
    const double* shift;                   // [shift_rows][E] or nullptr
    int shift_rows;
    double sigma[3];
    uint32_t key0, key1, member0;
    double* table;                         // [E][rows][D]
    int32_t* ident;                        // [E]: e
};

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
            const double sh = g.shift[(size_t)r * g.E + e];
            v = r < 2 ? v * sh : v + sh;
        }
        const double sigma = g.sigma[r];
        if (sigma > 0.0) {
            const double z = philox_normal(g.member0 + (uint32_t)e, (uint32_t)g.group[r][d], (uint32_t)r, SIMPLYP_FORCING_STREAM,
                                           g.key0, g.key1);
            v = r < 2 ? v * sp_exp(sigma * z - 0.5 * sigma * sigma) : v + sigma * z;
        }
        dst[(size_t)r * D] = v;
    }
}

}  // namespace simplyp
