// simplyp_weighted_quantile.hip.h -- exact quantiles under integer weights across the member axis of a device table
// [n_rows][E] (gfx950): the weighted twins of simplyp_quantile.hip.h's two selectors, which stay as they are.
//
// The rule is simplyp_weighted.h's: member j of the table's column order carries the integer w_slot[j] (0: it takes no part),
// T is their sum, and probability k asks for the first member in key order whose inclusive running weight reaches
// thr[k] = max(1, ceil(p_k T)) -- the host forms the thresholds exactly from the T the prepare kernel reads back.  One value
// per probability.  Everything here is integer arithmetic: no floating-point add, integer LDS atomics only, so the outputs do
// not depend on arrival order and the same call twice gives the same bits.
//
//   weighted_prepare_kernel   w_slot[j] = include[m] ? q[m] : 0 with m = member_of_slot[j] (or j); T, the members with
//                             w_slot > 0 and the weights above 2^40, in one launch of one workgroup.
//   weighted_sort_kernel      rows of <= WQSORT_MAX members: (key, weight) pairs of 2048 / P rows at a time are bitonic-sorted
//                             in LDS by key, the weights of every sorted segment are scanned, and each threshold is found by
//                             bisection of the running sums.
//   weighted_select_kernel    longer rows: one 1024-lane workgroup per row, radix select over the key, 8 bits per sweep.  A
//                             group's 256-bin histogram holds the bins' WEIGHTS (uint64) beside their member counts; a wanted
//                             rank is a remaining weight walked down the bins.  Lanes of a wavefront that hit the same bin are
//                             merged into one add of their weight sum (a masked wave reduction) and one of their count, twice,
//                             then one by one, as the unweighted kernel merges counts -- but a sum costs six shuffle steps where
//                             a count is a popcount, so a round merges only when WQ_MERGE_MIN lanes or more share the bin (the
//                             first sweeps, where the digit is sign and exponent).  Once every group's bucket holds <= WQLIST
//                             members one last sweep collects the buckets in LDS and the ranks are settled there by summing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "simplyp_quantile.hip.h"

namespace simplyp {

constexpr int WQ_MAX_K = 16;               // probabilities per call = groups of the select: one rank each
constexpr int WQSORT_MAX = 2048;           // longest row the LDS sort takes: 16 KB of keys and 16 KB of weights
constexpr int WQSORT_THREADS = 256;
constexpr int WQSORT_CHUNK = WQSORT_MAX / WQSORT_THREADS;     // consecutive elements a lane scans
constexpr int WQLIST = 32;                 // bucket size at which a group is finished by summing in LDS
constexpr unsigned long long WQ_MAX_WEIGHT = 1ull << 40;
#ifdef SIMPLYP_WQ_NO_MERGE                 // an experiment's build (tools/time_weighted_bands.py): every lane adds on its own
constexpr int WQ_MERGE_ROUNDS = 0;
#else
constexpr int WQ_MERGE_ROUNDS = 2;         // "twice, then one by one"
#endif
constexpr int WQ_MERGE_MIN = 8;            // lanes on one bin from which a round merges them

struct WqPrepared {                        // the head of the context's workspace
    unsigned long long T;
    int n_used, n_bad, n_passes, pad;
};

struct WQuantileArgs {
    int E;
    long long n_rows;
    const double* table;                   // [n_rows][E]
    const unsigned long long* w_slot;      // [E] in the table's column order
    int K;
    unsigned long long thr[WQ_MAX_K];      // 1 <= thr[k] <= T
    double* order_stats;                   // [K][out_stride]: row r of the table is row out_row0 + r of the result
    long long out_row0, out_stride;
    int* n_passes;
};

__global__ __launch_bounds__(1024) void weighted_prepare_kernel(int E, const unsigned long long* q, const uint8_t* include,
                                                                const int32_t* member_of_slot, unsigned long long* w_slot,
                                                                WqPrepared* res)
{
    __shared__ unsigned long long total;
    __shared__ int used, bad;
    if (threadIdx.x == 0) { total = 0ull; used = 0; bad = 0; }
    __syncthreads();
    unsigned long long mine = 0ull;
    int n = 0, b = 0;
    for (int j = threadIdx.x; j < E; j += blockDim.x) {
        const int m = member_of_slot ? member_of_slot[j] : j;
        unsigned long long w = 0ull;
        if (m >= 0 && m < E && (!include || include[m])) w = q[m];
        b += q[j] > WQ_MAX_WEIGHT;         // every weight of the vector is looked at once, whoever takes part
        if (w > WQ_MAX_WEIGHT) w = 0ull;   // the call is refused; keep the sums in range all the same
        w_slot[j] = w;
        mine += w;
        n += w > 0ull;
    }
    atomicAdd(&total, mine);
    atomicAdd(&used, n);
    atomicAdd(&bad, b);
    __syncthreads();
    if (threadIdx.x == 0) { res->T = total; res->n_used = used; res->n_bad = bad; res->n_passes = 0; res->pad = 0; }
}

// ---- short rows: bitonic sort of (key, weight) pairs, 2048 / P rows at a time -----------------------------------------------
__global__ __launch_bounds__(WQSORT_THREADS) void weighted_sort_kernel(const WQuantileArgs g, int P)
{
    __shared__ unsigned long long keys[WQSORT_MAX];
    __shared__ unsigned long long wts[WQSORT_MAX];             // the weights, then their running sums per segment
    __shared__ unsigned long long tot[2][WQSORT_THREADS];      // the lanes' chunk sums, scanned
    const int rows_per_block = WQSORT_MAX / P;
    const long long row0 = (long long)blockIdx.x * rows_per_block;
    const int E = g.E, tid = threadIdx.x;
    for (int i = tid; i < WQSORT_MAX; i += WQSORT_THREADS) {
        const int r = i / P, j = i - r * P;
        unsigned long long k = QKEY_PAD, w = 0ull;
        if (row0 + r < g.n_rows && j < E) {
            w = g.w_slot[j];
            if (w > 0ull) k = quantile_key(g.table[(size_t)(row0 + r) * E + j]);
        }
        keys[i] = k;
        wts[i] = w;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < WQSORT_MAX / 2; t += WQSORT_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                const bool asc = (k == P) || ((i & k) == 0);
                const unsigned long long a = keys[i], b = keys[l];
                if ((a > b) == asc) {
                    keys[i] = b; keys[l] = a;
                    const unsigned long long wa = wts[i];
                    wts[i] = wts[l]; wts[l] = wa;
                }
            }
            __syncthreads();
        }
    }
    // inclusive running sums inside every P-long segment: a lane's 8 consecutive elements, then the lanes' sums, then both
    const int base = tid * WQSORT_CHUNK;
    unsigned long long run = 0ull;
#pragma unroll
    for (int u = 0; u < WQSORT_CHUNK; ++u) {
        if (((base + u) & (P - 1)) == 0) run = 0ull;           // a segment begins here (P < 8: inside the chunk)
        run += wts[base + u];
        wts[base + u] = run;
    }
    if (P > WQSORT_CHUNK) {
        const int c = P / WQSORT_CHUNK, pos = tid & (c - 1);   // chunks per segment, this one's place among them
        tot[0][tid] = run;
        __syncthreads();
        int cur = 0;
        for (int d = 1; d < c; d <<= 1) {
            unsigned long long v = tot[cur][tid];
            if (pos >= d) v += tot[cur][tid - d];
            tot[cur ^ 1][tid] = v;
            cur ^= 1;
            __syncthreads();
        }
        const unsigned long long carry = pos > 0 ? tot[cur][tid - 1] : 0ull;
#pragma unroll
        for (int u = 0; u < WQSORT_CHUNK; ++u) wts[base + u] += carry;
    }
    __syncthreads();
    for (int i = tid; i < rows_per_block * g.K; i += WQSORT_THREADS) {
        const int r = i / g.K, k = i - r * g.K;
        if (row0 + r >= g.n_rows) continue;
        const unsigned long long* C = wts + r * P;
        const unsigned long long t = g.thr[k];
        int lo = 0, hi = P - 1;                                // the first C >= t lies in [lo, hi]: C[P - 1] = T >= t
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (C[mid] >= t) hi = mid; else lo = mid + 1;
        }
        g.order_stats[(size_t)k * g.out_stride + g.out_row0 + row0 + r] = quantile_value(keys[r * P + lo]);
    }
    if (blockIdx.x == 0 && tid == 0) atomicMax(g.n_passes, 1);
}

// ---- long rows: radix select on weights, one workgroup per row --------------------------------------------------------------
struct WQSelShared {
    unsigned long long whist[WQ_MAX_K * 256];      // per group: the bins' weights
    unsigned chist[WQ_MAX_K * 256];                // per group: the bins' members
    unsigned long long list_key[WQ_MAX_K * WQLIST];    // per group: the bucket's keys and weights (last sweep)
    unsigned long long list_w[WQ_MAX_K * WQLIST];
    unsigned list_n[WQ_MAX_K];
    unsigned long long prefix[WQ_MAX_K];           // per group: the key bits settled so far (right-aligned)
    unsigned count[WQ_MAX_K];                      // per group: members of the row under that prefix
    unsigned long long t_prefix[WQ_MAX_K];         // per rank, while regrouping
    unsigned t_count[WQ_MAX_K];
    unsigned long long rem[WQ_MAX_K];              // per rank: the weight still to pass inside its group's bucket
    int group[WQ_MAX_K];
    int G;
    int collect;
};

__device__ __forceinline__ unsigned long long wq_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <bool COLLECT>
__device__ __forceinline__ void weighted_sweep(const WQuantileArgs& g, const double* row, WQSelShared& s, int pass)
{
    const int E = g.E, G = s.G;
    const int shift = 56 - 8 * pass;
    const int lane = threadIdx.x & 63;
    for (int base = 0; base < E; base += QSEL_THREADS * QSEL_UNROLL) {     // uniform trip count: ballots and shuffles below
        double x[QSEL_UNROLL];
        unsigned long long w[QSEL_UNROLL];
#pragma unroll
        for (int u = 0; u < QSEL_UNROLL; ++u) {
            const int j = base + u * QSEL_THREADS + (int)threadIdx.x;
            w[u] = j < E ? g.w_slot[j] : 0ull;
            x[u] = j < E ? row[j] : 0.0;           // not waiting for the weight: both loads are in flight together
        }
#pragma unroll
        for (int u = 0; u < QSEL_UNROLL; ++u) {
            const unsigned long long key = quantile_key(x[u]);
            int grp = -1;
            if (w[u] > 0ull) {
                if (pass == 0) grp = 0;
                else {
                    const unsigned long long pre = key >> (shift + 8);
                    for (int q = 0; q < G; ++q) if (s.prefix[q] == pre) grp = q;
                }
            }
            if (COLLECT) {
                if (grp >= 0) {
                    const unsigned at = atomicAdd(&s.list_n[grp], 1u);     // < count[grp] <= WQLIST for a table nobody writes
                    if (at < (unsigned)WQLIST) {
                        s.list_key[grp * WQLIST + at] = key;
                        s.list_w[grp * WQLIST + at] = w[u];
                    }
                }
            } else {
                const unsigned bin = grp >= 0 ? (unsigned)(grp * 256 + (int)((key >> shift) & 0xFF)) : 0xFFFFFFFFu;
                bool pending = grp >= 0;
                // lanes of the wavefront on the same bin: one add of their weight sum and one of their count (twice; what is
                // left adds one by one)
#pragma unroll
                for (int it = 0; it < WQ_MERGE_ROUNDS; ++it) {
                    const unsigned long long m = __ballot(pending);
                    if (m != 0ull) {
                        const int leader = __ffsll((long long)m) - 1;
                        const unsigned b0 = (unsigned)__shfl((int)bin, leader);
                        const bool same = pending && bin == b0;
                        const unsigned long long sm = __ballot(same);
                        // few lanes on the leader's bin (uniform: sm is a ballot): the digits are spread, a reduction would cost
                        // more than the adds it saves, here and in the next round -- what is pending adds one by one
                        if (__popcll(sm) < WQ_MERGE_MIN) break;
                        const unsigned long long sum = wq_wave_sum(same ? w[u] : 0ull);
                        if (lane == leader) {
                            atomicAdd(&s.whist[b0], sum);
                            atomicAdd(&s.chist[b0], (unsigned)__popcll(sm));
                        }
                        if (same) pending = false;
                    }
                }
                if (pending) {
                    atomicAdd(&s.whist[bin], w[u]);
                    atomicAdd(&s.chist[bin], 1u);
                }
            }
        }
    }
}

__global__ __launch_bounds__(QSEL_THREADS) void weighted_select_kernel(const WQuantileArgs g)
{
    __shared__ WQSelShared s;
    const int K = g.K;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int max_sweeps = 0;
    for (long long r = blockIdx.x; r < g.n_rows; r += gridDim.x) {
        const double* row = g.table + (size_t)r * g.E;
        __syncthreads();                           // the previous row's state is no longer read
        if (tid < K) { s.rem[tid] = g.thr[tid] - 1ull; s.group[tid] = 0; }
        if (tid == 0) { s.G = 1; s.prefix[0] = 0ull; s.collect = 0; }
        __syncthreads();
        int sweeps = 0;
        bool done = false;
        for (int pass = 0; pass < 8 && !done; ++pass) {
            const int G = s.G;
            if (s.collect) {                       // uniform: written before the last barrier
                if (tid < G) s.list_n[tid] = 0u;
                __syncthreads();
                weighted_sweep<true>(g, row, s, pass);
                ++sweeps;
                __syncthreads();
                // a wavefront per rank: lane i places the bucket's i-th key by summing the weights below and beside it
                for (int t = wave; t < K; t += QSEL_THREADS / 64) {
                    const int q = s.group[t];
                    const unsigned n = s.count[q];
                    const unsigned long long want = s.rem[t];
                    if ((unsigned)lane < n) {
                        const unsigned long long mine = s.list_key[q * WQLIST + lane];
                        unsigned long long less = 0ull, equal = 0ull;
                        for (unsigned i = 0; i < n; ++i) {
                            const unsigned long long o = s.list_key[q * WQLIST + i], ow = s.list_w[q * WQLIST + i];
                            less += o < mine ? ow : 0ull;
                            equal += o == mine ? ow : 0ull;
                        }
                        if (less <= want && want < less + equal)       // lanes holding equal keys store the same value
                            g.order_stats[(size_t)t * g.out_stride + g.out_row0 + r] = quantile_value(mine);
                    }
                }
                done = true;
                break;
            }
            for (int i = tid; i < G * 256; i += QSEL_THREADS) { s.whist[i] = 0ull; s.chist[i] = 0u; }
            __syncthreads();
            weighted_sweep<false>(g, row, s, pass);
            ++sweeps;
            __syncthreads();
            // every rank walks its group's weights to its digit
            if (tid < K) {
                const int q = s.group[tid];
                const unsigned long long* h = s.whist + q * 256;
                unsigned long long rem = s.rem[tid];
                int d = 0;
                for (; d < 255; ++d) { const unsigned long long c = h[d]; if (rem < c) break; rem -= c; }
                s.rem[tid] = rem;
                s.t_prefix[tid] = (s.prefix[q] << 8) | (unsigned long long)d;
                s.t_count[tid] = s.chist[q * 256 + d];
            }
            __syncthreads();
            if (tid == 0) {                        // ranks with equal prefixes share a group from here on
                int n_groups = 0;
                unsigned biggest = 0;
                for (int t = 0; t < K; ++t) {
                    int q = 0;
                    while (q < n_groups && s.prefix[q] != s.t_prefix[t]) ++q;
                    if (q == n_groups) { s.prefix[q] = s.t_prefix[t]; s.count[q] = s.t_count[t]; ++n_groups; }
                    s.group[t] = q;
                    biggest = s.t_count[t] > biggest ? s.t_count[t] : biggest;
                }
                s.G = n_groups;
                s.collect = (biggest <= (unsigned)WQLIST) ? 1 : 0;
            }
            __syncthreads();
        }
        if (!done && tid < K)                      // all 64 bits settled: the prefix is the key
            g.order_stats[(size_t)tid * g.out_stride + g.out_row0 + r] = quantile_value(s.prefix[s.group[tid]]);
        max_sweeps = sweeps > max_sweeps ? sweeps : max_sweeps;
    }
    if (tid == 0 && max_sweeps > 0) atomicMax(g.n_passes, max_sweeps);
}

}  // namespace simplyp
