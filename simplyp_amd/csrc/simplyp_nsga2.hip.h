// simplyp_nsga2.hip.h -- NSGA-II's own pieces on the device (gfx950): crowding distance, environmental selection, mating with
// variation, the initial population.  simplyp_amd/nsga2.py states the rule; simplyp_nsga2.h holds the variation of one
// dimension, compiled here and by a host program from one text.
//
//   nsga2_keys_kernel       y = sense x of every member as order-preserving keys key[M][n] (pareto_key: the two zeros one key).
//   nsga2_crowd_pairs_kernel  the all-pairs pass, in the shape of pareto_pairs_kernel.  A lane owns member i with its rank and
//                           its MP keys in registers (compiled for M padded to 1, 2, 3, 4, 6, 8); the j side is wave-uniform:
//                           a workgroup takes NSGA2_JSPLIT consecutive j, NSGA2_JTILE at a time staged in LDS with their ranks
//                           and read as a broadcast.  Per objective the lane keeps four running keys: the largest (key, j)
//                           below its own (key, i) within its front -- only the key is needed: it is the lane's own key when
//                           an equal member of lower index exists --, the smallest above, the front's min and max.  The j
//                           splits of the grid are combined with 64-bit atomicMax / atomicMin on the keys: exact in any
//                           order.  0 and ~0 are the keys of NaNs, which take no part: "none yet".
//   nsga2_crowd_finish_kernel  the keys back to doubles and the final arithmetic, ((0 + term_0) + term_1) + ..., m ascending.
//   nsga2_position_kernel   the same all-pairs shape on (rank, crowding key, index): how many members come before i; the j
//                           splits add int32 partial counts with integer atomics.
//   nsga2_gather_kernel     the members of position < N to their position: survivor, rank, crowding and the caller's rows.
//                           The order is strict and total, so the positions are a permutation and every slot is written once.
//   nsga2_offspring_kernel  one lane per child pair: two binary tournaments, then per dimension the gather of the parents'
//                           values, simplyp_nsga2::vary_dim, the SoA stores of child columns p and N/2 + p and the scatter into
//                           member_params / f_tdp through target[] (simplyp_mcmc_propose's convention).  Loops over d read
//                           memory; no per-lane arrays.
//   nsga2_init_kernel       one lane per member: clip(lo + (hi - lo) u) and the same scatter.
// Draws: Philox4x32-10, counter (pair or member, generation, code << 8 | d, "NSG2"); nsga2.py fixes the codes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simplyp.h"
#include "../../include/simplyp_nsga2.h"   // the entries' declarations
#include "simplyp_mcmc.hip.h"              // MCMC_TARGET_*, mcmc_count
#include "simplyp_nsga2.h"
#include "simplyp_pareto.hip.h"            // pareto_key
#include "simplyp_predictive.hip.h"        // philox4x32_10, philox_uniform

namespace simplyp {

constexpr int NSGA2_THREADS = 256;
constexpr int NSGA2_JTILE = 512;               // j staged in LDS at a time: MP x 4 KiB of keys and 2 KiB of ranks
constexpr int NSGA2_JSPLIT = 2048;             // consecutive j of one workgroup: the grid's second axis splits the j range
constexpr uint32_t NSGA2_STREAM = 0x4E534732u; // "NSG2": the counter's fourth word
enum { NSGA2_TOURNAMENT = 0, NSGA2_CROSS, NSGA2_SBX, NSGA2_MUTATE_A, NSGA2_MUTATE_B, NSGA2_INIT };
constexpr unsigned long long NSGA2_NONE_BELOW = 0ull, NSGA2_NONE_ABOVE = ~0ull;

struct Nsga2KeyArgs {
    int n, M;
    int sense[SIMPLYP_PARETO_MAX_OBJ];
    const double* obj;                         // [M][n]
    unsigned long long* key;                   // [M][n]
    unsigned long long* run;                   // [4][M][n]: prev, next, front min, front max -- set to "none yet"
};

__global__ __launch_bounds__(NSGA2_THREADS) void nsga2_keys_kernel(const Nsga2KeyArgs g)
{
    const int i = blockIdx.x * NSGA2_THREADS + threadIdx.x;
    if (i >= g.n) return;
    const size_t plane = (size_t)g.M * g.n;
    for (int m = 0; m < g.M; ++m) {
        const size_t at = (size_t)m * g.n + i;
        g.key[at] = pareto_key(g.obj[at], g.sense[m]);
        g.run[at] = NSGA2_NONE_BELOW;
        g.run[plane + at] = NSGA2_NONE_ABOVE;
        g.run[2 * plane + at] = NSGA2_NONE_ABOVE;
        g.run[3 * plane + at] = NSGA2_NONE_BELOW;
    }
}

template <int MP>
__global__ __launch_bounds__(NSGA2_THREADS) void nsga2_crowd_pairs_kernel(const unsigned long long* __restrict__ key, int M, int n,
                                                                          const int32_t* __restrict__ rank,
                                                                          unsigned long long* __restrict__ run)
{
    __shared__ unsigned long long tile[MP][NSGA2_JTILE];
    __shared__ int tile_rank[NSGA2_JTILE];
    const int idx = blockIdx.x * NSGA2_THREADS + threadIdx.x;
    const bool live = idx < n;
    const int i = live ? idx : 0;
    const int ri = live ? rank[i] : -1;
    unsigned long long ki[MP], prev[MP], next[MP], fmin[MP], fmax[MP];
#pragma unroll
    for (int m = 0; m < MP; ++m) {
        ki[m] = (live && m < M) ? key[(size_t)m * n + i] : 0ull;
        prev[m] = NSGA2_NONE_BELOW; next[m] = NSGA2_NONE_ABOVE; fmin[m] = NSGA2_NONE_ABOVE; fmax[m] = NSGA2_NONE_BELOW;
    }
    const int j_begin = blockIdx.y * NSGA2_JSPLIT;
    const int j_end = min(n, j_begin + NSGA2_JSPLIT);
    for (int j0 = j_begin; j0 < j_end; j0 += NSGA2_JTILE) {
        const int jn = min(NSGA2_JTILE, j_end - j0);
        __syncthreads();                                       // the tile before this one has been read
        for (int t = threadIdx.x; t < jn; t += NSGA2_THREADS) {
            tile_rank[t] = rank[j0 + t];
#pragma unroll
            for (int m = 0; m < MP; ++m) tile[m][t] = m < M ? key[(size_t)m * n + (j0 + t)] : 0ull;
        }
        __syncthreads();
#pragma unroll 2
        for (int t = 0; t < jn; ++t) {
            const int j = j0 + t;
            const bool same = ri >= 0 && tile_rank[t] == ri;   // i's front; i itself enters the front's min and max only
#pragma unroll
            for (int m = 0; m < MP; ++m) {
                const unsigned long long kj = tile[m][t];
                const bool below = kj < ki[m] || (kj == ki[m] && j < i);
                const bool above = kj > ki[m] || (kj == ki[m] && j > i);
                if (same) {
                    fmin[m] = kj < fmin[m] ? kj : fmin[m];
                    fmax[m] = kj > fmax[m] ? kj : fmax[m];
                    if (below) prev[m] = kj > prev[m] ? kj : prev[m];
                    if (above) next[m] = kj < next[m] ? kj : next[m];
                }
            }
        }
    }
    if (!live || ri < 0) return;
    const size_t plane = (size_t)M * n;
#pragma unroll
    for (int m = 0; m < MP; ++m) {
        if (m >= M) continue;
        const size_t at = (size_t)m * n + i;
        if (prev[m] != NSGA2_NONE_BELOW) atomicMax(&run[at], prev[m]);
        if (next[m] != NSGA2_NONE_ABOVE) atomicMin(&run[plane + at], next[m]);
        if (fmin[m] != NSGA2_NONE_ABOVE) atomicMin(&run[2 * plane + at], fmin[m]);
        if (fmax[m] != NSGA2_NONE_BELOW) atomicMax(&run[3 * plane + at], fmax[m]);
    }
}

// The double an order-preserving key stands for (a zero comes back as +0.0).
__device__ __forceinline__ double nsga2_value(unsigned long long k)
{
    const unsigned long long b = (k >> 63) ? (k ^ 0x8000000000000000ull) : ~k;
    return __longlong_as_double((long long)b);
}

__global__ __launch_bounds__(NSGA2_THREADS) void nsga2_crowd_finish_kernel(int n, int M, const int32_t* __restrict__ rank,
                                                                           const unsigned long long* __restrict__ run,
                                                                           double* __restrict__ crowd, unsigned* __restrict__ counters)
{
    const int i = blockIdx.x * NSGA2_THREADS + threadIdx.x;
    if (i >= n) return;
    if (rank[i] < 0) { crowd[i] = 0.0; return; }
    const size_t plane = (size_t)M * n;
    bool edge = false;
    double d = 0.0;
    for (int m = 0; m < M; ++m) {
        const size_t at = (size_t)m * n + i;
        const unsigned long long kp = run[at], kn = run[plane + at];
        edge = edge || kp == NSGA2_NONE_BELOW || kn == NSGA2_NONE_ABOVE;
        const double span = nsga2_value(run[3 * plane + at]) - nsga2_value(run[2 * plane + at]);
        const double term = span > 0.0 ? (nsga2_value(kn) - nsga2_value(kp)) / span : 0.0;
        d = d + (edge ? 0.0 : term);
    }
    crowd[i] = edge ? __builtin_huge_val() : d;
    atomicAdd(counters + 0, 1u);                               // the members with a rank
}

// A rank as the selection reads it: any negative rank (invalid) comes after every front.
__device__ __forceinline__ uint32_t nsga2_rank(int32_t r)
{
    return r < 0 ? 0xFFFFFFFFu : (uint32_t)r;
}

// Does (rank_a, crowding key ca, a) come before (rank_b, cb, b)?
__device__ __forceinline__ bool nsga2_before(uint32_t ra, unsigned long long ca, int a, uint32_t rb, unsigned long long cb, int b)
{
    return ra < rb || (ra == rb && (ca > cb || (ca == cb && a < b)));
}

__global__ __launch_bounds__(NSGA2_THREADS) void nsga2_position_kernel(int n, const int32_t* __restrict__ rank,
                                                                       const double* __restrict__ crowd, int32_t* __restrict__ position)
{
    __shared__ unsigned long long tile_c[NSGA2_JTILE];
    __shared__ uint32_t tile_r[NSGA2_JTILE];
    const int idx = blockIdx.x * NSGA2_THREADS + threadIdx.x;
    const bool live = idx < n;
    const int i = live ? idx : 0;
    const uint32_t ri = live ? nsga2_rank(rank[i]) : 0u;
    const unsigned long long ci = live ? pareto_key(crowd[i], 1) : 0ull;
    const int j_begin = blockIdx.y * NSGA2_JSPLIT;
    const int j_end = min(n, j_begin + NSGA2_JSPLIT);
    int count = 0;
    for (int j0 = j_begin; j0 < j_end; j0 += NSGA2_JTILE) {
        const int jn = min(NSGA2_JTILE, j_end - j0);
        __syncthreads();
        for (int t = threadIdx.x; t < jn; t += NSGA2_THREADS) {
            tile_r[t] = nsga2_rank(rank[j0 + t]);
            tile_c[t] = pareto_key(crowd[j0 + t], 1);
        }
        __syncthreads();
#pragma unroll 4
        for (int t = 0; t < jn; ++t) count += nsga2_before(tile_r[t], tile_c[t], j0 + t, ri, ci, i) ? 1 : 0;
    }
    if (live && count) atomicAdd(&position[i], count);
}

struct Nsga2GatherArgs {
    int n, N, n_rows;
    const int32_t* position;                   // [n]
    const int32_t* rank;                       // [n]
    const double* crowd;                       // [n]
    const double* rows_in;                     // [n_rows][n]
    int32_t* survivor;                         // [N]
    int32_t* rank_out;                         // [N] or nullptr
    double* crowd_out;                         // [N] or nullptr
    double* rows_out;                          // [n_rows][N]
};

__global__ __launch_bounds__(NSGA2_THREADS) void nsga2_gather_kernel(const Nsga2GatherArgs g)
{
    const int i = blockIdx.x * NSGA2_THREADS + threadIdx.x;
    if (i >= g.n) return;
    const int q = g.position[i];
    if (q < 0 || q >= g.N) return;
    g.survivor[q] = i;
    if (g.rank_out) g.rank_out[q] = g.rank[i];
    if (g.crowd_out) g.crowd_out[q] = g.crowd[i];
    for (int r = 0; r < g.n_rows; ++r) g.rows_out[(size_t)r * g.N + q] = g.rows_in[(size_t)r * g.n + i];
}

struct Nsga2VaryArgs {
    int N, n_dim, k_c, k_m;
    double p_cross, p_mut;
    uint32_t key0, key1, t;
    double lo[simplyp_nsga2::MAX_DIM], hi[simplyp_nsga2::MAX_DIM];
    int target[simplyp_nsga2::MAX_DIM];
    const double* theta;                       // [n_dim][N]
    const int32_t* rank;                       // [N]
    const double* crowd;                       // [N]
    double* child;                             // [n_dim][N]
    int32_t* parents;                          // [2][N] or nullptr
    double* member_params;                     // [NP_M][N]
    double* f_tdp;                             // [N]
    unsigned* counters;                        // [4]: children, pairs that crossed
};

__device__ __forceinline__ double nsga2_u32(uint32_t x)
{
    return ((double)x + 0.5) * 0x1p-32;
}

__device__ __forceinline__ void nsga2_scatter(const Nsga2VaryArgs& g, int d, int col, double v)
{
    const int tg = g.target[d];
    if (tg == MCMC_TARGET_NONE) return;
    if (tg == MCMC_TARGET_F_TDP) g.f_tdp[col] = v;
    else g.member_params[(size_t)tg * g.N + col] = v;
}

// The tournament between candidates a and b, both < N.
__device__ __forceinline__ int nsga2_winner(const Nsga2VaryArgs& g, int a, int b)
{
    const bool a_wins = a == b || nsga2_before(nsga2_rank(g.rank[a]), pareto_key(g.crowd[a], 1), a,
                                               nsga2_rank(g.rank[b]), pareto_key(g.crowd[b], 1), b);
    return a_wins ? a : b;
}

__global__ __launch_bounds__(NSGA2_THREADS) void nsga2_offspring_kernel(const Nsga2VaryArgs g)
{
    const int p = blockIdx.x * NSGA2_THREADS + threadIdx.x;
    const int N = g.N, h = N / 2;
    if (p >= h) return;
    const unsigned long long NN = (unsigned long long)N;
    const Philox4 x = philox4x32_10((uint32_t)p, g.t, (uint32_t)(NSGA2_TOURNAMENT << 8), NSGA2_STREAM, g.key0, g.key1);
    // (x N) >> 32 < N: x < 2^32
    const int p1 = nsga2_winner(g, (int)((x.x0 * NN) >> 32), (int)((x.x1 * NN) >> 32));
    const int p2 = nsga2_winner(g, (int)((x.x2 * NN) >> 32), (int)((x.x3 * NN) >> 32));
    const Philox4 xc = philox4x32_10((uint32_t)p, g.t, (uint32_t)(NSGA2_CROSS << 8), NSGA2_STREAM, g.key0, g.key1);
    const bool cross = philox_uniform(xc.x0, xc.x1) < g.p_cross;
    if (g.parents) {
        g.parents[p] = p1; g.parents[h + p] = p1;
        g.parents[N + p] = p2; g.parents[N + h + p] = p2;
    }
    for (int d = 0; d < g.n_dim; ++d) {
        const Philox4 s = philox4x32_10((uint32_t)p, g.t, (uint32_t)((NSGA2_SBX << 8) | d), NSGA2_STREAM, g.key0, g.key1);
        const Philox4 ma = philox4x32_10((uint32_t)p, g.t, (uint32_t)((NSGA2_MUTATE_A << 8) | d), NSGA2_STREAM, g.key0, g.key1);
        const Philox4 mb = philox4x32_10((uint32_t)p, g.t, (uint32_t)((NSGA2_MUTATE_B << 8) | d), NSGA2_STREAM, g.key0, g.key1);
        double a, b;
        simplyp_nsga2::vary_dim(g.theta[(size_t)d * N + p1], g.theta[(size_t)d * N + p2], g.lo[d], g.hi[d], g.k_c, g.k_m, g.p_mut, cross,
                                philox_uniform(s.x0, s.x1), nsga2_u32(s.x2), nsga2_u32(s.x3),
                                philox_uniform(ma.x0, ma.x1), philox_uniform(ma.x2, ma.x3),
                                philox_uniform(mb.x0, mb.x1), philox_uniform(mb.x2, mb.x3), a, b);
        g.child[(size_t)d * N + p] = a;
        g.child[(size_t)d * N + h + p] = b;
        nsga2_scatter(g, d, p, a);
        nsga2_scatter(g, d, h + p, b);
    }
    atomicAdd(g.counters + 0, 2u);
    mcmc_count(g.counters + 1, cross);
}

__global__ __launch_bounds__(NSGA2_THREADS) void nsga2_init_kernel(const Nsga2VaryArgs g)
{
    const int i = blockIdx.x * NSGA2_THREADS + threadIdx.x;
    if (i >= g.N) return;
    for (int d = 0; d < g.n_dim; ++d) {
        const Philox4 x = philox4x32_10((uint32_t)i, 0u, (uint32_t)((NSGA2_INIT << 8) | d), NSGA2_STREAM, g.key0, g.key1);
        const double v = simplyp_nsga2::clip(g.lo[d] + (g.hi[d] - g.lo[d]) * philox_uniform(x.x0, x.x1), g.lo[d], g.hi[d]);
        g.child[(size_t)d * g.N + i] = v;
        nsga2_scatter(g, d, i, v);
    }
    atomicAdd(g.counters + 0, 1u);
}

}  // namespace simplyp
