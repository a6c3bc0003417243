// simplyp_quantile.hip.h -- exact order statistics across the member axis of a device table [n_rows][E] (gfx950).
//
// What the reference's only ensemble caller does with its runs: for every day the 2.5 / 50 / 97.5 percentiles across the
// members (Development/2016/MCMC.ipynb, get_uncertainty_intervals: param_only.T.describe(percentiles=[...])).  For every
// row and each of K probabilities the kernels return the two order statistics x_(k_lo), x_(k_hi) that bracket numpy's
// 'linear' quantile (k_lo = floor(q (n - 1)), k_hi = min(k_lo + 1, n - 1)); the host interpolates.
//
// Ordering: an fp64 value maps to a 64-bit key that keeps order (sign bit flipped for non-negatives, all bits flipped for
// negatives); every NaN maps to one key above +inf's, as np.sort places it.  -0.0 and +0.0 get adjacent keys: which of the
// two comes back is decided by the rank alone, never by timing.
//
// Two kernels, both read-only on the table:
//   quantile_sort_kernel    rows of <= QSORT_MAX members: 4096 / P rows per workgroup (P = row length padded to a power of
//                           two) are loaded into LDS as keys and bitonic-sorted there; one sweep of the table.
//   quantile_select_kernel  longer rows: one 1024-lane workgroup owns a row from first digit to last and runs a most-
//                           significant-digit radix select over it, 8 bits per sweep.  The 2K wanted ranks are refined in
//                           the same sweep: ranks that still share a key prefix share one 256-bin LDS histogram ("group").
//                           Once every group's bucket holds <= QLIST members, one last sweep collects the buckets in LDS
//                           and the ranks are settled there by counting -- 4 sweeps for a row of 100 000 distinct doubles
//                           within a few binades, 8 (the whole key) for rows with heavy ties.  Histogram adds are LDS
//                           atomics on integers: the counts, and with them every output, do not depend on arrival order.
//                           Lanes of a wavefront that hit the same bin -- all of them in the first sweeps, where the
//                           digit is sign and exponent -- are merged into one add of their count first (64-wide ballot).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simplyp.h"

namespace simplyp {

constexpr int QUANT_MAX_K = 16;            // probabilities per call
constexpr int QUANT_MAX_T = 2 * QUANT_MAX_K;   // wanted ranks per row: lower and upper of each
constexpr int QSORT_MAX = 4096;            // longest row the LDS sort takes (32 KB of keys)
constexpr int QSORT_THREADS = 256;
constexpr int QSEL_THREADS = 1024;
constexpr int QSEL_UNROLL = 4;             // independent loads in flight per lane
constexpr int QLIST = 64;                  // bucket size at which a group is finished by counting in LDS (one lane each)
constexpr unsigned long long QKEY_NAN = 0xFFF8000000000000ull;   // above +inf's key 0xFFF0...
constexpr unsigned long long QKEY_PAD = 0xFFFFFFFFFFFFFFFFull;   // excluded members and padding of the LDS sort: after everything

struct QuantileArgs {
    int E;                                 // members = row length
    long long n_rows;
    const double* table;                   // [n_rows][E]
    const uint8_t* include_slot;           // [E] in the table's column order, or nullptr = all
    int T;                                 // 2K
    long long rank[QUANT_MAX_T];           // rank[2k] = k_lo, rank[2k+1] = k_hi of probability k; all < n_used
    double* order_stats;                   // [2][K][out_stride]: row r of the table is row out_row0 + r of the result
    long long out_row0, out_stride;        // (0, n_rows) for a table selected in one launch; a chunk of a larger result otherwise
    int* n_passes;                         // max over rows of the sweeps made (atomicMax)
};

__device__ __forceinline__ unsigned long long quantile_key(double x)
{
    if (x != x) return QKEY_NAN;
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ double quantile_value(unsigned long long k)
{
    const unsigned long long b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    return __longlong_as_double((long long)b);
}

// include_slot[j] = include[member_of_slot[j]] (or include[j]); *n_used = members that take part.  One workgroup.
__global__ __launch_bounds__(1024) void quantile_mask_kernel(int E, const uint8_t* include, const int32_t* member_of_slot,
                                                             uint8_t* include_slot, int* n_used)
{
    __shared__ int total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    int mine = 0;
    for (int j = threadIdx.x; j < E; j += blockDim.x) {
        const int m = member_of_slot ? member_of_slot[j] : j;
        const uint8_t v = (m >= 0 && m < E && include[m]) ? 1 : 0;
        include_slot[j] = v;
        mine += v;
    }
    atomicAdd(&total, mine);
    __syncthreads();
    if (threadIdx.x == 0) *n_used = total;
}

__global__ __launch_bounds__(256) void quantile_fill_nan_kernel(double* p, long long n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = __longlong_as_double(0x7FF8000000000000ll);
}

// ---- short rows: bitonic sort of 4096 / P rows at a time in LDS ---------------------------------------------------------
__global__ __launch_bounds__(QSORT_THREADS) void quantile_sort_kernel(const QuantileArgs g, int P)
{
    __shared__ unsigned long long keys[QSORT_MAX];
    const int rows_per_block = QSORT_MAX / P;
    const long long row0 = (long long)blockIdx.x * rows_per_block;
    const int E = g.E;
    for (int i = threadIdx.x; i < QSORT_MAX; i += QSORT_THREADS) {
        const int r = i / P, j = i - r * P;
        unsigned long long k = QKEY_PAD;
        if (row0 + r < g.n_rows && j < E && (!g.include_slot || g.include_slot[j]))
            k = quantile_key(g.table[(size_t)(row0 + r) * E + j]);
        keys[i] = k;
    }
    __syncthreads();
    // every P-long segment on its own: the standard network up to k = P, the last merge ascending in every segment
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < QSORT_MAX / 2; t += QSORT_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));      // lower index of the pair
                const int l = i | j;
                const bool asc = (k == P) || ((i & k) == 0);
                const unsigned long long a = keys[i], b = keys[l];
                if ((a > b) == asc) { keys[i] = b; keys[l] = a; }
            }
            __syncthreads();
        }
    }
    const int K = g.T / 2;
    for (int i = threadIdx.x; i < rows_per_block * g.T; i += QSORT_THREADS) {
        const int r = i / g.T, t = i - r * g.T;
        if (row0 + r < g.n_rows)
            g.order_stats[((size_t)(t & 1) * K + (t >> 1)) * g.out_stride + g.out_row0 + row0 + r] = quantile_value(keys[r * P + (int)g.rank[t]]);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicMax(g.n_passes, 1);
}

// ---- long rows: radix select, one workgroup per row --------------------------------------------------------------------
struct QSelShared {
    unsigned hist[QUANT_MAX_T * 256];              // per group
    unsigned long long list[QUANT_MAX_T * QLIST];  // per group: the bucket's keys (last sweep)
    unsigned list_n[QUANT_MAX_T];
    unsigned long long prefix[QUANT_MAX_T];        // per group: the key bits settled so far (right-aligned)
    unsigned count[QUANT_MAX_T];                   // per group: members of the row under that prefix
    unsigned long long t_prefix[QUANT_MAX_T];      // per rank, while regrouping
    unsigned t_count[QUANT_MAX_T];
    unsigned long long rem[QUANT_MAX_T];           // per rank: its rank inside its group's bucket
    int group[QUANT_MAX_T];                        // per rank
    int G;
    int collect;                                   // 1: the next sweep collects the buckets instead of counting digits
};

// One sweep over the row.  COLLECT = false: histogram of the next 8 key bits per group.  true: the groups' buckets to LDS.
template <bool COLLECT>
__device__ __forceinline__ void quantile_sweep(const QuantileArgs& g, const double* row, QSelShared& s, int pass)
{
    const int E = g.E, G = s.G;
    const int shift = 56 - 8 * pass;               // the digit's position; bits above shift + 8 are the prefix
    const int lane = threadIdx.x & 63;
    for (int base = 0; base < E; base += QSEL_THREADS * QSEL_UNROLL) {     // uniform trip count: ballots below
        double x[QSEL_UNROLL];
        bool on[QSEL_UNROLL];
#pragma unroll
        for (int u = 0; u < QSEL_UNROLL; ++u) {
            const int j = base + u * QSEL_THREADS + (int)threadIdx.x;
            on[u] = j < E && (!g.include_slot || g.include_slot[j]);
            x[u] = on[u] ? row[j] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < QSEL_UNROLL; ++u) {
            const unsigned long long key = quantile_key(x[u]);
            int grp = -1;
            if (on[u]) {
                if (pass == 0) grp = 0;
                else {
                    const unsigned long long pre = key >> (shift + 8);
                    for (int q = 0; q < G; ++q) if (s.prefix[q] == pre) grp = q;
                }
            }
            if (COLLECT) {
                if (grp >= 0) s.list[grp * QLIST + atomicAdd(&s.list_n[grp], 1u)] = key;
            } else {
                const unsigned bin = grp >= 0 ? (unsigned)(grp * 256 + (int)((key >> shift) & 0xFF)) : 0xFFFFFFFFu;
                bool pending = grp >= 0;
                // lanes of the wavefront on the same bin: one add of their count (twice; what is left adds one by one)
#pragma unroll
                for (int it = 0; it < 2; ++it) {
                    const unsigned long long m = __ballot(pending);
                    if (m != 0ull) {
                        const int leader = __ffsll((long long)m) - 1;
                        const unsigned b0 = (unsigned)__shfl((int)bin, leader);
                        const bool same = pending && bin == b0;
                        const unsigned long long sm = __ballot(same);
                        if (lane == leader) atomicAdd(&s.hist[b0], (unsigned)__popcll(sm));
                        if (same) pending = false;
                    }
                }
                if (pending) atomicAdd(&s.hist[bin], 1u);
            }
        }
    }
}

__global__ __launch_bounds__(QSEL_THREADS) void quantile_select_kernel(const QuantileArgs g)
{
    __shared__ QSelShared s;
    const int T = g.T, K = T / 2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int max_sweeps = 0;
    for (long long r = blockIdx.x; r < g.n_rows; r += gridDim.x) {
        const double* row = g.table + (size_t)r * g.E;
        __syncthreads();                           // the previous row's state is no longer read
        if (tid < T) { s.rem[tid] = (unsigned long long)g.rank[tid]; s.group[tid] = 0; }
        if (tid == 0) { s.G = 1; s.prefix[0] = 0ull; s.collect = 0; }
        __syncthreads();
        int sweeps = 0;
        bool done = false;
        for (int pass = 0; pass < 8 && !done; ++pass) {
            const int G = s.G;
            if (s.collect) {                       // uniform: written before the last barrier
                if (tid < G) s.list_n[tid] = 0u;
                __syncthreads();
                quantile_sweep<true>(g, row, s, pass);
                ++sweeps;
                __syncthreads();
                // a wavefront per rank: lane i ranks the bucket's i-th key by counting the smaller ones
                for (int t = wave; t < T; t += QSEL_THREADS / 64) {
                    const int q = s.group[t];
                    const unsigned n = s.count[q];
                    const unsigned long long want = s.rem[t];
                    if ((unsigned)lane < n) {
                        const unsigned long long mine = s.list[q * QLIST + lane];
                        unsigned less = 0, equal = 0;
                        for (unsigned i = 0; i < n; ++i) {
                            const unsigned long long o = s.list[q * QLIST + i];
                            less += o < mine; equal += o == mine;
                        }
                        if (less <= want && want < less + equal)       // lanes holding equal keys store the same value
                            g.order_stats[((size_t)(t & 1) * K + (t >> 1)) * g.out_stride + g.out_row0 + r] = quantile_value(mine);
                    }
                }
                done = true;
                break;
            }
            for (int i = tid; i < G * 256; i += QSEL_THREADS) s.hist[i] = 0u;
            __syncthreads();
            quantile_sweep<false>(g, row, s, pass);
            ++sweeps;
            __syncthreads();
            // every rank walks its group's histogram to its digit
            if (tid < T) {
                const unsigned* h = s.hist + s.group[tid] * 256;
                unsigned long long rem = s.rem[tid];
                int d = 0;
                for (; d < 255; ++d) { const unsigned c = h[d]; if (rem < c) break; rem -= c; }
                s.rem[tid] = rem;
                s.t_prefix[tid] = (s.prefix[s.group[tid]] << 8) | (unsigned long long)d;
                s.t_count[tid] = h[d];
            }
            __syncthreads();
            if (tid == 0) {                        // ranks with equal prefixes share a group from here on
                int n_groups = 0;
                unsigned biggest = 0;
                for (int t = 0; t < T; ++t) {
                    int q = 0;
                    while (q < n_groups && s.prefix[q] != s.t_prefix[t]) ++q;
                    if (q == n_groups) { s.prefix[q] = s.t_prefix[t]; s.count[q] = s.t_count[t]; ++n_groups; }
                    s.group[t] = q;
                    biggest = s.t_count[t] > biggest ? s.t_count[t] : biggest;
                }
                s.G = n_groups;
                s.collect = (biggest <= (unsigned)QLIST) ? 1 : 0;
            }
            __syncthreads();
        }
        if (!done && tid < T)                      // all 64 bits settled: the prefix is the key
            g.order_stats[((size_t)(tid & 1) * K + (tid >> 1)) * g.out_stride + g.out_row0 + r] = quantile_value(s.prefix[s.group[tid]]);
        max_sweeps = sweeps > max_sweeps ? sweeps : max_sweeps;
    }
    if (tid == 0 && max_sweeps > 0) atomicMax(g.n_passes, max_sweeps);
}

}  // namespace simplyp
