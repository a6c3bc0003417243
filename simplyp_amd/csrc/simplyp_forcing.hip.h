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
    int pet_model;                         // != 0: row 1 is written as F, the row of a base PET of 1.0 (simplyp_forcing_pet_kernel)
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
        double v = r == 1 && g.pet_model ? 1.0 : src[(size_t)r * D];
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
            v = r == 1 && g.pet_model ? 1.0 : src[d];
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

// ---- Thornthwaite PET from each member's own T_air row (opts.forcing_pet_model = 1; include/simplyp.h states the rule and the
// plan, simplyp_amd/forcing.py thornthwaite_rows is its NumPy statement, operation for operation).  Runs after a generator
// above, which wrote the member's final T_air row and, into the PET row, F = the row of a base PET of 1.0 (pet_model there).
//
// One workgroup per member (the table is [E][3][D]: the snow module's layout), three stages with barriers between them:
//   1. monthly means.  The T_air row goes through LDS in tiles of PET_TILE_MONTHS whole months: all lanes load the tile's days
//      along d (full segments), then one lane per month adds its <= 31 days from LDS left to right -- the order the statement
//      fixes -- and leaves the clamped mean and its heat-index term (T_m / 5)^1.514 in LDS.
//   2. per year, one lane: I = the 12 terms added in order, and the exponent a; then per month, one lane: the node value
//      PET_m / N, written over the heat-index term.
//   3. lanes along d again: every day reads its two node values from LDS, interpolates, multiplies by F and stores in place --
//      full segments, the T_air row read once, the PET row read (only with a scale or a sigma) and written once.
// LDS: the tile (15.5 KB), two arrays of 12 x PET_YEARS_MAX doubles (12 KB) and two of PET_YEARS_MAX; no scratch.  Plan entries
// are clamped where they index memory: a plan that does not fit the run gives wrong numbers, never an access outside the row.
constexpr int PET_THREADS = 256;
constexpr int PET_YEARS_MAX = SIMPLYP_FORCING_PET_YEARS_MAX;
constexpr int PET_MONTHS_MAX = 12 * PET_YEARS_MAX;
constexpr int PET_TILE_MONTHS = 64;
constexpr int PET_TILE_DAYS = PET_TILE_MONTHS * 31;

struct ForcingPetArgs {
    int E, D, M, Y;                        // M = 12 Y months
    const int32_t* day;                    // [3][D]: j, k, n
    const int32_t* month;                  // [2][M]: first day, N
    const double* daylight;                // [M]: L
    double* table;                         // [E][3][D]
    int has_f;                             // the generator wrote an F other than 1.0: a PET scale or sigma
};

// x^y = exp(y log x) for x > 0; exactly 0 for x == 0 (either sign); NaN for a NaN (0 / 0 of a year with I = 0).
__device__ __forceinline__ double forcing_pow(double x, double y)
{
    const double p = sp_exp(y * sp_log(x > 0.0 ? x : 1.0));
    return x > 0.0 ? p : x == 0.0 ? 0.0 : __builtin_nan("");
}

__global__ __launch_bounds__(PET_THREADS) void simplyp_forcing_pet_kernel(const ForcingPetArgs g)
{
    __shared__ double tile[PET_TILE_DAYS];
    __shared__ double t_m[PET_MONTHS_MAX];                 // the clamped monthly mean
    __shared__ double val[PET_MONTHS_MAX];                 // the heat-index term, then the node value
    __shared__ double heat[PET_YEARS_MAX], expo[PET_YEARS_MAX];
    const int e = (int)blockIdx.x, tid = (int)threadIdx.x;     // (host: E blocks, M <= PET_MONTHS_MAX, Y <= PET_YEARS_MAX)
    const int D = g.D, M = g.M;
    const double* t_air = g.table + ((size_t)e * 3 + 2) * (size_t)D;
    double* pet = g.table + ((size_t)e * 3 + 1) * (size_t)D;
    const int32_t* first = g.month;
    const int32_t* ndays = g.month + M;

    for (int m0 = 0; m0 < M; m0 += PET_TILE_MONTHS) {      // uniform trip count: barriers inside
        const int base = min(max(first[m0], 0), D);
        const int count = min(PET_TILE_DAYS, D - base);
        for (int i = tid; i < count; i += PET_THREADS) tile[i] = t_air[base + i];
        __syncthreads();
        const int m = m0 + tid;
        if (tid < PET_TILE_MONTHS && m < M) {
            const unsigned off = (unsigned)first[m] - (unsigned)base;
            const int nd = min(max(ndays[m], 0), 31);
            double s = 0.0;
            for (int i = 0; i < nd; ++i) {
                const unsigned idx = off + (unsigned)i;
                if (idx < (unsigned)count) s = s + tile[idx];
            }
            const double t = s / (double)nd;
            const double adj = t * (t >= 0.0 ? 1.0 : 0.0);
            const double x = adj / 5.0;
            t_m[m] = adj;
            val[m] = x > 0.0 ? forcing_pow(x, 1.514) : 0.0;
        }
        __syncthreads();                                   // also: the tile is free for the next load
    }

    for (int y = tid; y < g.Y; y += PET_THREADS) {
        double I = 0.0;
        for (int j = 0; j < 12; ++j) I = I + val[y * 12 + j];
        const double I2 = I * I, I3 = I2 * I;
        heat[y] = I;
        expo[y] = (((6.75e-07 * I3) - (7.71e-05 * I2)) + (1.792e-02 * I)) + 0.49239;
    }
    __syncthreads();
    for (int m = tid; m < M; m += PET_THREADS) {
        const int y = m / 12;
        const double N = (double)min(max(ndays[m], 0), 31);
        const double p = forcing_pow((10.0 * t_m[m]) / heat[y], expo[y]);
        val[m] = ((((1.6 * (g.daylight[m] / 12.0)) * (N / 30.0)) * p) * 10.0) / N;
    }
    __syncthreads();

    const int32_t* node = g.day;
    const int32_t* pos = g.day + (size_t)D;
    const int32_t* len = g.day + 2 * (size_t)D;
    for (int d = tid; d < D; d += PET_THREADS) {
        const int j = min(max(node[d], 0), M - 1);
        const int k = pos[d];
        const double y0 = val[j], y1 = val[min(j + 1, M - 1)];
        const double th = k == 0 ? y0 : y0 + ((y1 - y0) / (double)len[d]) * (double)k;
        pet[d] = g.has_f ? th * pet[d] : th;
    }
}

}  // namespace simplyp
