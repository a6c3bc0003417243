// simplyp_score.hip.h -- scoring an ensemble against observations across the member axis of a device table (gfx950): the
// weighted counts below / at or below the observation, the mean absolute error A and the spread B of simplyp_score.h, whose
// two term functions the kernels call.  Only the scored rows (those with an observation) are read or sorted.
//
//   score_ones_kernel          the unit weights of a call without weights: the unweighted case goes through the weighted path
//   score_rows_kernel          (predictive entry) the scored (series, day, reach) rows of the series simplyp_predictive_kernel
//                              would write, generated into a compact table [rows][E]: the same resolver, expressions and
//                              Philox counter, so the same bits
//   score_stream_kernel        counts and A: one workgroup per scored row, one streaming pass.  The counts are integer wave
//                              reductions; A is a per-lane partial (lane t adds members t, t + 1024, ...: at most 4096 terms
//                              for E <= 2^22) and a fixed tree over the 1024 partials in LDS
//   score_tile_sort_kernel     B, step 1: every tile of SCORE_TILE members of a row is sorted in LDS as (key, weight) pairs by
//                              bitonic_segments (a member that takes no part: the padding key, weight 0, so it sorts behind
//                              everything) and written to the workspace
//   score_merge_kernel         B, step 2 (rows longer than a tile): one stable merge pass over runs of length L -- every
//                              element finds its rank in the partner run by binary search (lower bound from the left run,
//                              upper bound from the right) and is written to its place in the other buffer; an odd run at
//                              the end is copied.  ceil(log2(ceil(E / SCORE_TILE))) passes
//   score_gap_kernel           B, step 3: one workgroup per row walks the sorted pairs 1024 at a time, scans the weights (wave
//                              scan, then the waves' totals, then the carry of the blocks before) to the inclusive running
//                              weight C_k, and adds spread_term(x_(k), x_(k+1), C_k, T) to the lane's partial; the same fixed
//                              tree ends it
// No floating-point atomics and no order that depends on arrival: a row's outputs are a function of the row, the weights and
// the observation alone -- not of the row's place in the table, the chunk it fell into or the call.  Equal keys may come out of
// the bitonic tile sort in any order: the gaps between them are zero, and the running weight behind the last of them is the
// same whatever their order, so B does not see it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "simplyp_predictive.hip.h"
#include "simplyp_quantile.hip.h"               // keys, bitonic_segments, wq_wave_sum
#include "simplyp_score.h"

namespace simplyp {

constexpr int SCORE_TILE = simplyp_score::SCORE_TILE;
constexpr int SCORE_THREADS = 1024;
constexpr int SCORE_WAVES = SCORE_THREADS / 64;

struct ScoreArgs {
    int E;
    int n_rows;                            // scored rows of this launch
    const double* table;                   // [*][E]
    const long long* row;                  // [n_rows] the table's row of every scored row, or nullptr: row i of the table
    const double* y;                       // [n_rows] observations (finite)
    const long long* dst;                  // [n_rows] the result's row
    const unsigned long long* w_slot;      // [E] in the table's column order
    unsigned long long T;                  // > 0
    double* sums;                          // [2][out_stride]: abs_err, spread
    unsigned long long* counts;            // [2][out_stride]: below, at_or_below
    long long out_stride;
    unsigned long long* keys[2];           // workspace, each [n_rows][E]: the sorted keys, and the merge's other buffer
    unsigned long long* wts[2];
};

__global__ __launch_bounds__(256) void score_ones_kernel(unsigned long long* w, int E)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < E) w[j] = 1ull;
}

__device__ __forceinline__ bool score_nonfinite(double x) { return !(fabs(x) < __longlong_as_double(0x7FF0000000000000ll)); }

// The sum of the block's 1024 partials, in one fixed shape; every lane returns it.  `s` holds SCORE_THREADS doubles.
__device__ __forceinline__ double score_block_sum(double v, double* s)
{
    const int tid = threadIdx.x;
    __syncthreads();
    s[tid] = v;
    for (int h = SCORE_THREADS / 2; h > 0; h >>= 1) {
        __syncthreads();
        if (tid < h) s[tid] += s[tid + h];
    }
    __syncthreads();
    return s[0];
}

// ---- the scored rows of the predictive series ---------------------------------------------------------------------------------
// grid: (member blocks of PRED_THREADS, scored rows (strided)); rows3[i] = (series index, day, output reach) of scored row i
template <int KIND, bool DRAW>
__device__ __forceinline__ double score_pred_value(const PredArgs& g, const TqSeries& sr, int d, double m, uint32_t member, uint32_t reach,
                                                   uint32_t series)
{
    const size_t off = (size_t)d * g.R * g.E;
    const double a = sr.p0[off];
    const double b = KIND >= 2 ? sr.p1[off] : 0.0;
    const double c = KIND == 3 ? sr.p2[off] : 0.0;
    double v = tq_value<KIND>(sr, a, b, c);
    if (DRAW) {
        const double z = philox_normal(member, g.day0 + (uint32_t)d, reach, series, g.key0, g.key1);
        v = v + (m * v) * z;
    }
    return v;
}

__global__ __launch_bounds__(PRED_THREADS) void score_rows_kernel(const PredArgs g, const int* rows3, int n_rows)
{
    const int slot = blockIdx.x * PRED_THREADS + threadIdx.x;
    if (slot >= g.E) return;                               // no barrier below
    const bool draw = g.err_m != nullptr;
    for (int i = blockIdx.y; i < n_rows; i += gridDim.y) {
        const int si = rows3[3 * i], d = rows3[3 * i + 1], r = rows3[3 * i + 2];
        const int code = g.series[si];
        int member = g.member_of_slot && (code < 0 || draw) ? g.member_of_slot[slot] : slot;
        if ((unsigned)member >= (unsigned)g.E) member = slot;
        const int reach = g.reach_of[r];
        const double m = draw ? g.err_m[(size_t)si * g.E + member] : 0.0;
        const uint32_t sid = g.series_id[si];
        TqSeries sr;
        const int kind = tq_series(sr, code, g.out, g.col_stride, g.col, (size_t)r * g.E + slot, g.a_catch, g.f_tdp,
                                   (size_t)reach * g.E + member, member);
        double v;
        if (draw) {
            if (kind == 0) v = score_pred_value<0, true>(g, sr, d, m, (uint32_t)member, (uint32_t)reach, sid);
            else if (kind == 1) v = score_pred_value<1, true>(g, sr, d, m, (uint32_t)member, (uint32_t)reach, sid);
            else if (kind == 2) v = score_pred_value<2, true>(g, sr, d, m, (uint32_t)member, (uint32_t)reach, sid);
            else v = score_pred_value<3, true>(g, sr, d, m, (uint32_t)member, (uint32_t)reach, sid);
        } else {
            if (kind == 0) v = score_pred_value<0, false>(g, sr, d, m, (uint32_t)member, (uint32_t)reach, sid);
            else if (kind == 1) v = score_pred_value<1, false>(g, sr, d, m, (uint32_t)member, (uint32_t)reach, sid);
            else if (kind == 2) v = score_pred_value<2, false>(g, sr, d, m, (uint32_t)member, (uint32_t)reach, sid);
            else v = score_pred_value<3, false>(g, sr, d, m, (uint32_t)member, (uint32_t)reach, sid);
        }
        g.dst[(size_t)i * g.E + slot] = v;
    }
}

// ---- counts and A: one streaming pass -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SCORE_THREADS) void score_stream_kernel(const ScoreArgs g)
{
    __shared__ double part[SCORE_THREADS];
    __shared__ unsigned long long s_lo[SCORE_WAVES], s_le[SCORE_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = blockIdx.x;
    const double* row = g.table + (size_t)(g.row ? g.row[r] : r) * g.E;
    const double y = g.y[r];
    unsigned long long lo = 0ull, le = 0ull;
    double a = 0.0;
    int bad = 0;
#pragma unroll 4
    for (int j = tid; j < g.E; j += SCORE_THREADS) {
        const unsigned long long w = g.w_slot[j];
        const double x = row[j];
        if (w > 0ull) {
            lo += x < y ? w : 0ull;                        // a NaN member is above every y
            le += x <= y ? w : 0ull;
            bad |= score_nonfinite(x);
            a += simplyp_score::abs_err_term(x, y, w, g.T);
        }
    }
    lo = wq_wave_sum(lo);
    le = wq_wave_sum(le);
    if (lane == 0) { s_lo[wave] = lo; s_le[wave] = le; }
    bad = __syncthreads_or(bad);
    const double A = score_block_sum(a, part);
    if (tid == 0) {
        unsigned long long below = 0ull, at = 0ull;
        for (int v = 0; v < SCORE_WAVES; ++v) { below += s_lo[v]; at += s_le[v]; }
        const long long o = g.dst[r];
        g.sums[o] = bad ? __longlong_as_double(0x7FF8000000000000ll) : A;
        g.counts[o] = below;
        g.counts[g.out_stride + o] = at;
    }
}

// ---- B, step 1: the tiles of a row, sorted in LDS ----------------------------------------------------------------------------
// grid: (tiles of a row, scored rows); P: the power of two the longest tile is padded to (2 <= P <= SCORE_TILE)
__global__ __launch_bounds__(SCORE_THREADS) void score_tile_sort_kernel(const ScoreArgs g, int P)
{
    __shared__ unsigned long long keys[SCORE_TILE];
    __shared__ unsigned long long wts[SCORE_TILE];
    const int tid = threadIdx.x, r = blockIdx.y;
    const int j0 = blockIdx.x * SCORE_TILE;
    const int len = min(SCORE_TILE, g.E - j0);             // >= 1: the grid has ceil(E / SCORE_TILE) tiles
    const double* row = g.table + (size_t)(g.row ? g.row[r] : r) * g.E + j0;
    for (int i = tid; i < P; i += SCORE_THREADS) {
        unsigned long long k = QKEY_PAD, w = 0ull;
        if (i < len) {
            w = g.w_slot[j0 + i];
            if (w > 0ull) k = quantile_key(row[i]);
        }
        keys[i] = k;
        wts[i] = w;
    }
    __syncthreads();
    bitonic_segments<SCORE_THREADS, true>(keys, wts, P, P);
    // the padding sorts last: the first `len` pairs are the tile's
    const size_t base = (size_t)r * g.E + j0;
    for (int i = tid; i < len; i += SCORE_THREADS) {
        g.keys[0][base + i] = keys[i];
        g.wts[0][base + i] = wts[i];
    }
}

// ---- B, step 2: one stable merge pass over runs of length L, buffer `src` to buffer 1 - src --------------------------------
// grid: (blocks of 1024 elements, scored rows)
__global__ __launch_bounds__(SCORE_THREADS) void score_merge_kernel(const ScoreArgs g, int L, int src)
{
    const int i = blockIdx.x * SCORE_THREADS + threadIdx.x;
    if (i >= g.E) return;                                  // no barrier below
    const size_t base = (size_t)blockIdx.y * g.E;
    const unsigned long long* keys = g.keys[src] + base;
    const unsigned long long key = keys[i], w = g.wts[src][base + i];
    const int run = i / L;
    const int left = (run & ~1) * L;                       // where the pair of runs begins; left + L <= E may fail for an odd run out
    const int mid = min(left + L, g.E), end = (int)min((long long)left + 2LL * L, (long long)g.E);
    int at;
    if (!(run & 1)) {                                      // from the left run: behind the partner's keys below mine
        int lo = mid, hi = end;
        while (lo < hi) {
            const int m = (lo + hi) >> 1;
            if (keys[m] < key) lo = m + 1; else hi = m;
        }
        at = i + (lo - mid);
    } else {                                               // from the right run: behind the partner's keys up to mine
        int lo = left, hi = mid;
        while (lo < hi) {
            const int m = (lo + hi) >> 1;
            if (keys[m] <= key) lo = m + 1; else hi = m;
        }
        at = (i - mid) + lo;
    }
    g.keys[src ^ 1][base + at] = key;
    g.wts[src ^ 1][base + at] = w;
}

// ---- B, step 3: running weights and the sum over the gaps, from buffer `src` ------------------------------------------------
__global__ __launch_bounds__(SCORE_THREADS) void score_gap_kernel(const ScoreArgs g, int src)
{
    __shared__ double part[SCORE_THREADS];
    __shared__ unsigned long long tot[2][SCORE_WAVES];     // the waves' totals of a block of 1024; two sets: one barrier per block
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = blockIdx.x;
    const unsigned long long* keys = g.keys[src] + (size_t)r * g.E;
    const unsigned long long* wts = g.wts[src] + (size_t)r * g.E;
    unsigned long long carry = 0ull;                       // the weight of the blocks before this one (uniform)
    double b = 0.0;
    int bad = 0, set = 0;
    for (int j0 = 0; j0 < g.E; j0 += SCORE_THREADS, set ^= 1) {        // uniform trip count: shuffles and barriers below
        const int i = j0 + tid;
        const unsigned long long k = i < g.E ? keys[i] : QKEY_PAD;
        const unsigned long long kn = i + 1 < g.E ? keys[i + 1] : QKEY_PAD;
        unsigned long long c = i < g.E ? wts[i] : 0ull;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long up = __shfl_up(c, o);
            if (lane >= o) c += up;
        }
        if (lane == 63) tot[set][wave] = c;
        __syncthreads();
        unsigned long long before = 0ull, all = 0ull;
#pragma unroll
        for (int v = 0; v < SCORE_WAVES; ++v) {
            const unsigned long long t = tot[set][v];
            before += v < wave ? t : 0ull;
            all += t;
        }
        if (k != QKEY_PAD) {
            const double x = quantile_value(k);
            bad |= score_nonfinite(x);
            if (kn != QKEY_PAD) b += simplyp_score::spread_term(x, quantile_value(kn), carry + before + c, g.T);
        }
        carry += all;
    }
    bad = __syncthreads_or(bad);
    const double B = score_block_sum(b, part);
    if (tid == 0) g.sums[g.out_stride + g.dst[r]] = bad ? __longlong_as_double(0x7FF8000000000000ll) : B;
}

}  // namespace simplyp
