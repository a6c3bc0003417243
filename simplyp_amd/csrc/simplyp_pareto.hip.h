// simplyp_pareto.hip.h -- Pareto dominance counts and non-dominated ranks of an ensemble's objectives (gfx950).
//
// simplyp_pareto.h states the rule.  The kernels compare 64-bit keys only and add int32 counters; no floating-point add anywhere.
//
//   pareto_flag_kernel     who takes part (include looked up through member_of_slot, no NaN objective): a flag per column and
//   pareto_scan_kernel     the count of every block of 256 columns; the block counts to exclusive offsets (one workgroup);
//   pareto_compact_kernel  the participants' keys, sense applied, to key[M][n] and their members to member_of[n], in column order
//                          (ballot + block offsets: stable, so the layout does not depend on timing).
//   pareto_pairs_kernel    the all-pairs pass.  A lane owns participant i with its M keys in registers (the kernel is compiled for
//                          M padded to 1, 2, 3, 4, 6, 8: a padding objective is equal for everybody and decides nothing).  The j
//                          side is wave-uniform: a workgroup takes PARETO_JSPLIT consecutive j, PARETO_JTILE at a time staged in
//                          LDS and read as a broadcast (MODE 0), or read straight from memory with wave-uniform addresses
//                          (MODE 1).  Per pair "j >= i in all" and "j <= i in all" give both directions: j dominates i iff the
//                          first holds without the second.  The j splits of the grid add their int32 partial counts with integer
//                          atomics, exact in any order.  MODE 2 is the peeling's subtraction: i runs over the list of members
//                          still alive, j over the list of the front just removed, and the count is taken off i's counter.
//   pareto_mark_kernel     one front of the peeling: of the members alive, those whose counter is 0 get the front's index as
//                          their rank and go to the front's list, the others to the next list of the living; two counters tell
//                          the host how long the lists are.  The lists' order depends on the blocks' arrival; nothing computed
//                          from them does.
//   pareto_fill_kernel, pareto_scatter_kernel   the outputs: -1 everywhere, then the participants' values in member order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simplyp.h"

namespace simplyp {

constexpr int PARETO_THREADS = 256;
constexpr int PARETO_WAVES = PARETO_THREADS / 64;
constexpr int PARETO_JTILE = 512;              // j keys staged in LDS at a time: M x 4 KiB
constexpr int PARETO_JSPLIT = 2048;            // consecutive j of one workgroup: the grid's second axis splits the j range

struct ParetoPrepArgs {
    int E, M, n_blocks;
    const double* obj;                         // [M][E] in column order
    const int32_t* member_of_slot;             // [E] or nullptr
    const uint8_t* include;                    // [E] member order, or nullptr
    int sense[SIMPLYP_PARETO_MAX_OBJ];
    uint8_t* flag;                             // [E]
    int* block_sum;                            // [n_blocks]: counts, then exclusive offsets
    int* n;                                    // the participants
    unsigned long long* key;                   // [M][E]: the first n of every plane are used
    int* member_of;                            // [n]
};

__device__ __forceinline__ unsigned long long pareto_key(double x, int sense)
{
    unsigned long long b = (unsigned long long)__double_as_longlong(x);
    if (sense < 0) b ^= 0x8000000000000000ull;
    if (b == 0x8000000000000000ull) b = 0ull;
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ bool pareto_takes_part(const ParetoPrepArgs& g, int j, int& member)
{
    member = g.member_of_slot ? g.member_of_slot[j] : j;
    bool ok = member >= 0 && member < g.E && (!g.include || g.include[member] != 0);
    for (int m = 0; m < g.M; ++m) {
        const double x = g.obj[(size_t)m * g.E + j];
        ok = ok && !(x != x);
    }
    return ok;
}

__global__ __launch_bounds__(PARETO_THREADS) void pareto_flag_kernel(const ParetoPrepArgs g)
{
    __shared__ int s[PARETO_WAVES];
    const int j = blockIdx.x * PARETO_THREADS + threadIdx.x;
    bool ok = false;
    if (j < g.E) {
        int member;
        ok = pareto_takes_part(g, j, member);
        g.flag[j] = ok ? 1 : 0;
    }
    const unsigned long long b = __ballot(ok);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x / 64] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < PARETO_WAVES; ++w) total += s[w];
        g.block_sum[blockIdx.x] = total;
    }
}

// The inclusive scan of the block's values; returns the block's total in every thread.
__device__ __forceinline__ int pareto_block_scan(int& v, int* s)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x / 64;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    if (lane == 63) s[wave] = v;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int i = 0; i < PARETO_WAVES; ++i) { if (i < wave) before += s[i]; total += s[i]; }
    __syncthreads();
    v += before;
    return total;
}

__global__ __launch_bounds__(PARETO_THREADS) void pareto_scan_kernel(const ParetoPrepArgs g)
{
    __shared__ int s[PARETO_WAVES];
    int carry = 0;
    for (int b0 = 0; b0 < g.n_blocks; b0 += PARETO_THREADS) {
        const int b = b0 + threadIdx.x;
        const int own = b < g.n_blocks ? g.block_sum[b] : 0;
        int v = own;
        const int total = pareto_block_scan(v, s);
        if (b < g.n_blocks) g.block_sum[b] = carry + (v - own);
        carry += total;
    }
    if (threadIdx.x == 0) *g.n = carry;
}

__global__ __launch_bounds__(PARETO_THREADS) void pareto_compact_kernel(const ParetoPrepArgs g)
{
    __shared__ int s[PARETO_WAVES];
    const int j = blockIdx.x * PARETO_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x / 64;
    const bool ok = j < g.E && g.flag[j] != 0;
    const unsigned long long b = __ballot(ok);
    if (lane == 0) s[wave] = __popcll(b);
    __syncthreads();
    int before = g.block_sum[blockIdx.x];
    for (int w = 0; w < PARETO_WAVES; ++w) if (w < wave) before += s[w];
    if (!ok) return;
    const int pos = before + __popcll(b & ((1ull << lane) - 1ull));      // < n <= E
    g.member_of[pos] = g.member_of_slot ? g.member_of_slot[j] : j;
    for (int m = 0; m < g.M; ++m) g.key[(size_t)m * g.E + pos] = pareto_key(g.obj[(size_t)m * g.E + j], g.sense[m]);
}

// MODE 0: both counts of participants [0, n_i) against j in [0, n_j), j tiles in LDS.  MODE 1: the same, j keys read from memory
// with wave-uniform addresses.  MODE 2: i = ilist[0 .. n_i), j = jlist[0 .. n_j); what dominates i is taken off by_count[i].
template <int MP, int MODE>
__global__ __launch_bounds__(PARETO_THREADS) void pareto_pairs_kernel(const unsigned long long* __restrict__ key, long long stride, int M,
                                                                      int n_i, const int* __restrict__ ilist,
                                                                      int n_j, const int* __restrict__ jlist,
                                                                      int* __restrict__ by_count, int* __restrict__ of_count)
{
    // every comparison leaves a 64-bit lane mask in scalar registers: 2 MP of them per pair, so the wider kernels unroll less
    constexpr int UNROLL = MP <= 2 ? 8 : MP <= 4 ? 4 : 2;
    __shared__ unsigned long long tile[MODE == 1 ? 1 : MP][MODE == 1 ? 1 : PARETO_JTILE];
    const int idx = blockIdx.x * PARETO_THREADS + threadIdx.x;
    const bool live = idx < n_i;
    const int i = live ? (MODE == 2 ? ilist[idx] : idx) : 0;
    unsigned long long ki[MP];
#pragma unroll
    for (int m = 0; m < MP; ++m) ki[m] = (live && m < M) ? key[(long long)m * stride + i] : 0ull;
    const int j_begin = blockIdx.y * PARETO_JSPLIT;
    const int j_end = min(n_j, j_begin + PARETO_JSPLIT);
    int by = 0, of = 0;
    for (int j0 = j_begin; j0 < j_end; j0 += PARETO_JTILE) {
        const int jn = min(PARETO_JTILE, j_end - j0);
        if (MODE != 1) {
            __syncthreads();                                   // the tile before this one has been read
            for (int t = threadIdx.x; t < jn; t += PARETO_THREADS) {
                const int j = MODE == 2 ? jlist[j0 + t] : j0 + t;
#pragma unroll
                for (int m = 0; m < MP; ++m) tile[m][t] = m < M ? key[(long long)m * stride + j] : 0ull;
            }
            __syncthreads();
        }
#pragma unroll UNROLL
        for (int t = 0; t < jn; ++t) {
            bool ge = true, le = true;
#pragma unroll
            for (int m = 0; m < MP; ++m) {
                unsigned long long kj;
                if (MODE == 1) kj = m < M ? key[(long long)m * stride + (j0 + t)] : 0ull;
                else kj = tile[m][t];
                ge = ge && kj >= ki[m];
                le = le && kj <= ki[m];
            }
            by += (ge && !le) ? 1 : 0;
            if (MODE != 2) of += (le && !ge) ? 1 : 0;
        }
    }
    if (!live) return;
    if (MODE == 2) {
        if (by) atomicSub(&by_count[i], by);
    } else {
        if (by) atomicAdd(&by_count[i], by);
        if (of) atomicAdd(&of_count[i], of);
    }
}

struct ParetoPeelArgs {
    int n_alive, front_index;
    const int* alive_in;                       // [n_alive] or nullptr = 0 .. n_alive - 1
    int* alive_out;                            // the members that stay
    int* front;                                // the members that leave
    const int* left;                           // [n] dominators not yet removed
    int* rank;                                 // [n] compact order
    int* counters;                             // [2]: the front's size, the members that stay (zero on entry)
    int* counters_next;                        // [2]: zeroed for the next front
};

__global__ __launch_bounds__(PARETO_THREADS) void pareto_mark_kernel(const ParetoPeelArgs g)
{
    __shared__ int s[2][PARETO_WAVES];
    __shared__ int base[2];
    const int idx = blockIdx.x * PARETO_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x / 64;
    const bool live = idx < g.n_alive;
    const int i = live ? (g.alive_in ? g.alive_in[idx] : idx) : 0;
    const bool leaves = live && g.left[i] == 0;
    const bool stays = live && !leaves;
    const unsigned long long bl = __ballot(leaves), bs = __ballot(stays);
    if (lane == 0) { s[0][wave] = __popcll(bl); s[1][wave] = __popcll(bs); }
    __syncthreads();
    if (threadIdx.x == 0) {
        int tl = 0, ts = 0;
        for (int w = 0; w < PARETO_WAVES; ++w) { tl += s[0][w]; ts += s[1][w]; }
        base[0] = tl ? atomicAdd(&g.counters[0], tl) : 0;
        base[1] = ts ? atomicAdd(&g.counters[1], ts) : 0;
        if (blockIdx.x == 0) { g.counters_next[0] = 0; g.counters_next[1] = 0; }
    }
    __syncthreads();
    int before_l = base[0], before_s = base[1];
    for (int w = 0; w < PARETO_WAVES; ++w) if (w < wave) { before_l += s[0][w]; before_s += s[1][w]; }
    const unsigned long long below = (1ull << lane) - 1ull;
    if (leaves) {
        g.rank[i] = g.front_index;
        g.front[before_l + __popcll(bl & below)] = i;          // < the front's size <= n_alive
    }
    if (stays) g.alive_out[before_s + __popcll(bs & below)] = i;
}

__global__ __launch_bounds__(PARETO_THREADS) void pareto_fill_kernel(int n, int value, int* a, int* b, int* c)
{
    const int i = blockIdx.x * PARETO_THREADS + threadIdx.x;
    if (i >= n) return;
    if (a) a[i] = value;
    if (b) b[i] = value;
    if (c) c[i] = value;
}

// The participants' values to member order: member_of[p] is in [0, E) by pareto_takes_part.
__global__ __launch_bounds__(PARETO_THREADS) void pareto_scatter_kernel(int n, const int* member_of, const int* by_count, const int* of_count,
                                                                        const int* rank_c, int* dominated_by, int* dominates, int* rank)
{
    const int p = blockIdx.x * PARETO_THREADS + threadIdx.x;
    if (p >= n) return;
    const int member = member_of[p];
    if (dominated_by) dominated_by[member] = by_count[p];
    if (dominates) dominates[member] = of_count[p];
    if (rank) rank[member] = rank_c[p];
}

}  // namespace simplyp
