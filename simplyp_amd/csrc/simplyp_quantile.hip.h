// simplyp_quantile.hip.h -- exact order statistics across the member axis of a device table [n_rows][E] (gfx950), plain and
// under integer weights.  The radix select and the LDS bitonic network every member-axis reduction uses live here, once.
//
// Unweighted: what the reference's only ensemble caller does with its runs: for every day the 2.5 / 50 / 97.5 percentiles
// across the members (Development/2016/MCMC.ipynb, get_uncertainty_intervals: param_only.T.describe(percentiles=[...])).  For
// every row and each of K probabilities the kernels return the two order statistics x_(k_lo), x_(k_hi) that bracket numpy's
// 'linear' quantile (k_lo = floor(q (n - 1)), k_hi = min(k_lo + 1, n - 1)); the host interpolates.
//
// Weighted: the rule is simplyp_weighted.h's: member j of the table's column order carries the integer w_slot[j] (0: it takes
// no part), T is their sum, and probability k asks for the first member in key order whose inclusive running weight reaches
// thr[k] = max(1, ceil(p_k T)) -- the host forms the thresholds exactly from the T the prepare kernel reads back.  One value per
// probability.  Everything is integer arithmetic: no floating-point add, integer LDS atomics only, so the outputs do not depend
// on arrival order and the same call twice gives the same bits.
//
// Ordering: an fp64 value maps to a 64-bit key that keeps order (sign bit flipped for non-negatives, all bits flipped for
// negatives); every NaN maps to one key above +inf's, as np.sort places it.  -0.0 and +0.0 get adjacent keys: which of the
// two comes back is decided by the rank alone, never by timing.
//
// All kernels are read-only on the table:
//   quantile_mask_kernel      include_slot[j] and the members that take part, one workgroup
//   weighted_prepare_kernel   w_slot[j] = include[m] ? q[m] : 0 with m = member_of_slot[j] (or j); T, the members with
//                             w_slot > 0 and the weights above 2^40, in one launch of one workgroup
//   quantile_sort_kernel      rows of <= QSORT_MAX members: 4096 / P rows per workgroup (P = row length padded to a power of
//                             two) are loaded into LDS as keys and sorted there by bitonic_segments; one sweep of the table
//   weighted_sort_kernel      rows of <= WQSORT_MAX members: (key, weight) pairs of 2048 / P rows at a time go through the same
//                             network, the weights of every sorted segment are scanned, and each threshold is found by bisection
//                             of the running sums
//   quantile_select_kernel, weighted_select_kernel
//                             longer rows: radix_select under its two policies.  One 1024-lane workgroup owns a row from first
//                             digit to last and runs a most-significant-digit radix select over it, 8 bits per sweep.  The
//                             wanted values are refined in the same sweep: those that still share a key prefix share one 256-bin
//                             LDS histogram ("group"); a wanted value is a remaining rank (weight) walked down the bins.  Once
//                             every group's bucket holds <= LIST members, one last sweep collects the buckets in LDS and the
//                             values are settled there by counting (summing) -- 4 sweeps for a row of 100 000 distinct doubles
//                             within a few binades, 8 (the whole key) for rows with heavy ties.  Histogram adds are LDS atomics
//                             on integers: the bins, and with them every output, do not depend on arrival order.  Lanes of a
//                             wavefront that hit the same bin -- all of them in the first sweeps, where the digit is sign and
//                             exponent -- are merged into one add first, twice, then one by one.
// A policy (QSelect, WQSelect) is what differs between the two selects and nothing else: what a bin accumulates and how a lane's
// contribution is read, whether member counts are kept beside the bins, how a wave merge is formed and from how many lanes on,
// the list length, and the wanted values of a row with their output planes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simplyp.h"

namespace simplyp {

constexpr int QUANT_MAX_K = 16;            // probabilities per call
constexpr int QUANT_MAX_T = 2 * QUANT_MAX_K;   // wanted ranks per row: lower and upper of each
constexpr int WQ_MAX_K = 16;               // weighted: probabilities per call = groups of the select: one value each
constexpr int QSORT_MAX = 4096;            // longest row the LDS sort takes (32 KB of keys)
constexpr int WQSORT_MAX = 2048;           // weighted: 16 KB of keys and 16 KB of weights
constexpr int QSORT_THREADS = 256;         // both sorts
constexpr int WQSORT_CHUNK = WQSORT_MAX / QSORT_THREADS;     // consecutive elements a lane scans
constexpr int QSEL_THREADS = 1024;
constexpr int QSEL_UNROLL = 4;             // independent loads in flight per lane
constexpr int QLIST = 64;                  // bucket size at which a group is finished by counting in LDS (one lane each)
constexpr int WQLIST = 32;                 // weighted: ... by summing in LDS
constexpr unsigned long long QKEY_NAN = 0xFFF8000000000000ull;   // above +inf's key 0xFFF0...
constexpr unsigned long long QKEY_PAD = 0xFFFFFFFFFFFFFFFFull;   // excluded members and padding of the LDS sort: after everything
constexpr unsigned long long WQ_MAX_WEIGHT = 1ull << 40;

struct SelectArgs {                        // what both selections are told
    int E;                                 // members = row length
    long long n_rows;
    const double* table;                   // [n_rows][E]
    double* order_stats;                   // [planes][out_stride]: row r of the table is row out_row0 + r of the result
    long long out_row0, out_stride;        // (0, n_rows) for a table selected in one launch; a chunk of a larger result otherwise
    int* n_passes;                         // max over rows of the sweeps made (atomicMax)
};

struct QuantileArgs : SelectArgs {         // order_stats: [2][K][out_stride]
    const uint8_t* include_slot;           // [E] in the table's column order, or nullptr = all
    int T;                                 // 2K
    long long rank[QUANT_MAX_T];           // rank[2k] = k_lo, rank[2k+1] = k_hi of probability k; all < n_used
};

struct WQuantileArgs : SelectArgs {        // order_stats: [K][out_stride]
    const unsigned long long* w_slot;      // [E] in the table's column order
    int K;
    unsigned long long thr[WQ_MAX_K];      // 1 <= thr[k] <= T
};

struct WqPrepared {                        // the head of the context's weighted workspace
    unsigned long long T;
    int n_used, n_bad, n_passes, pad;
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

__device__ __forceinline__ unsigned long long wq_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
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

__global__ __launch_bounds__(256) void quantile_fill_nan_kernel(double* p, long long n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = __longlong_as_double(0x7FF8000000000000ll);
}

// ---- the bitonic network: n LDS keys sorted ascending inside every P-long segment --------------------------------------------
// n and P are powers of two, P <= n; WTS: `wts` is carried along with the keys (a template flag, not a null test: an LDS address
// is not known to the compiler).  The whole workgroup of THREADS lanes calls it, with the arrays written and a barrier passed; it
// returns behind the barrier of the last stage.  Every segment runs the standard network up to k = P.
template <int THREADS, bool WTS>
__device__ __forceinline__ void bitonic_segments(unsigned long long* keys, unsigned long long* wts, int n, int P)
{
    for (int k = 2; k <= P; k <<= 1) {
        // the bit of i that says "descending": none in the last merge of several segments, which is ascending in each (with one
        // segment i < P has no such bit anyway).  Formed here and not as a second condition inside the compare-exchange: that
        // form cost the quantile sorts 3 % or the scores' tile sort a scalar instruction per pair (profiles/selection_refactor.md)
        const int dir = (k == P && n > P) ? 0 : k;
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < n / 2; t += THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));      // lower index of the pair
                const int l = i | j;
                const bool asc = (i & dir) == 0;
                const unsigned long long a = keys[i], b = keys[l];
                if ((a > b) == asc) {
                    keys[i] = b; keys[l] = a;
                    if (WTS) { const unsigned long long wa = wts[i]; wts[i] = wts[l]; wts[l] = wa; }
                }
            }
            __syncthreads();
        }
    }
}

// ---- short rows: 4096 / P rows at a time sorted in LDS, the wanted ranks read off ----------------------------------------------
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
    bitonic_segments<QSORT_THREADS, false>(keys, nullptr, QSORT_MAX, P);
    const int K = g.T / 2;
    for (int i = threadIdx.x; i < rows_per_block * g.T; i += QSORT_THREADS) {
        const int r = i / g.T, t = i - r * g.T;
        if (row0 + r < g.n_rows)
            g.order_stats[((size_t)(t & 1) * K + (t >> 1)) * g.out_stride + g.out_row0 + row0 + r] = quantile_value(keys[r * P + (int)g.rank[t]]);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicMax(g.n_passes, 1);
}

// ---- short rows, weighted: (key, weight) pairs of 2048 / P rows at a time, scanned and bisected --------------------------------
__global__ __launch_bounds__(QSORT_THREADS) void weighted_sort_kernel(const WQuantileArgs g, int P)
{
    __shared__ unsigned long long keys[WQSORT_MAX];
    __shared__ unsigned long long wts[WQSORT_MAX];             // the weights, then their running sums per segment
    __shared__ unsigned long long tot[2][QSORT_THREADS];       // the lanes' chunk sums, scanned
    const int rows_per_block = WQSORT_MAX / P;
    const long long row0 = (long long)blockIdx.x * rows_per_block;
    const int E = g.E, tid = threadIdx.x;
    for (int i = tid; i < WQSORT_MAX; i += QSORT_THREADS) {
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
    bitonic_segments<QSORT_THREADS, true>(keys, wts, WQSORT_MAX, P);
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
    for (int i = tid; i < rows_per_block * g.K; i += QSORT_THREADS) {
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

// ---- long rows: radix select, one workgroup per row ------------------------------------------------------------------------
// The two policies.  Acc: what a bin accumulates, and a lane's contribution to it (0: the member takes no part).
struct QSelect {                           // ranks: a bin counts its members, so the bins are the member counts too
    using Args = QuantileArgs;
    using Acc = unsigned;
    static constexpr bool WEIGHTED = false;
    static constexpr int MAX_T = QUANT_MAX_T, LIST = QLIST;
    static constexpr int MERGE_ROUNDS = 2, MERGE_MIN = 1;      // a merged count is a popcount: it always pays
    static __device__ __forceinline__ int wanted(const Args& g) { return g.T; }
    static __device__ __forceinline__ unsigned long long rem0(const Args& g, int t) { return (unsigned long long)g.rank[t]; }
    static __device__ __forceinline__ size_t plane(const Args& g, int t) { return (size_t)(t & 1) * (g.T / 2) + (t >> 1); }
    static __device__ __forceinline__ Acc contribution(const Args& g, int j) { return (!g.include_slot || g.include_slot[j]) ? 1u : 0u; }
    static __device__ __forceinline__ Acc merged(Acc, bool, unsigned long long same_mask) { return (unsigned)__popcll(same_mask); }
};

struct WQSelect {                          // weights: a bin sums its members' weights; their number is kept beside it
    using Args = WQuantileArgs;
    using Acc = unsigned long long;
    static constexpr bool WEIGHTED = true;
    static constexpr int MAX_T = WQ_MAX_K, LIST = WQLIST;
#ifdef SIMPLYP_WQ_NO_MERGE                 // an experiment's build (tools/time_weighted_bands.py): every lane adds on its own
    static constexpr int MERGE_ROUNDS = 0;
#else
    static constexpr int MERGE_ROUNDS = 2;
#endif
    // a sum costs six shuffle steps where a count is a popcount: a round merges only when this many lanes or more share the bin
    // (the first sweeps, where the digit is sign and exponent)
    static constexpr int MERGE_MIN = 8;
    static __device__ __forceinline__ int wanted(const Args& g) { return g.K; }
    static __device__ __forceinline__ unsigned long long rem0(const Args& g, int t) { return g.thr[t] - 1ull; }
    static __device__ __forceinline__ size_t plane(const Args&, int t) { return (size_t)t; }
    static __device__ __forceinline__ Acc contribution(const Args& g, int j) { return g.w_slot[j]; }
    static __device__ __forceinline__ Acc merged(Acc mine, bool same, unsigned long long) { return wq_wave_sum(same ? mine : 0ull); }
};

template <class P, bool W = P::WEIGHTED> struct SelBins {          // unweighted: no second histogram, no weight list
    typename P::Acc hist[P::MAX_T * 256];          // per group: the bins
    unsigned long long list[P::MAX_T * P::LIST];   // per group: the bucket's keys (last sweep)
};
template <class P> struct SelBins<P, true> {
    typename P::Acc hist[P::MAX_T * 256];          // per group: the bins' weights
    unsigned chist[P::MAX_T * 256];                // per group: the bins' members
    unsigned long long list[P::MAX_T * P::LIST];   // per group: the bucket's keys and weights (last sweep)
    unsigned long long list_w[P::MAX_T * P::LIST];
};

template <class P> struct SelShared : SelBins<P> {
    unsigned list_n[P::MAX_T];
    unsigned long long prefix[P::MAX_T];           // per group: the key bits settled so far (right-aligned)
    unsigned count[P::MAX_T];                      // per group: members of the row under that prefix
    unsigned long long t_prefix[P::MAX_T];         // per wanted value, while regrouping
    unsigned t_count[P::MAX_T];
    unsigned long long rem[P::MAX_T];              // per wanted value: the rank (weight) still to pass inside its group's bucket
    int group[P::MAX_T];                           // per wanted value
    int G;
    int collect;                                   // 1: the next sweep collects the buckets instead of adding to the bins
};

// One sweep over the row.  COLLECT = false: histogram of the next 8 key bits per group.  true: the groups' buckets to LDS.
template <class P, bool COLLECT>
__device__ __forceinline__ void select_sweep(const typename P::Args& g, const double* row, SelShared<P>& s, int pass)
{
    using Acc = typename P::Acc;
    const int E = g.E, G = s.G;
    const int shift = 56 - 8 * pass;               // the digit's position; bits above shift + 8 are the prefix
    const int lane = threadIdx.x & 63;
    for (int base = 0; base < E; base += QSEL_THREADS * QSEL_UNROLL) {     // uniform trip count: ballots and shuffles below
        double x[QSEL_UNROLL];
        Acc w[QSEL_UNROLL];
#pragma unroll
        for (int u = 0; u < QSEL_UNROLL; ++u) {
            const int j = base + u * QSEL_THREADS + (int)threadIdx.x;
            w[u] = j < E ? P::contribution(g, j) : Acc(0);
            // a weight is 8 bytes: the table load does not wait for it, both are in flight together; a mask byte decides first
            x[u] = (P::WEIGHTED ? j < E : w[u] != Acc(0)) ? row[j] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < QSEL_UNROLL; ++u) {
            const unsigned long long key = quantile_key(x[u]);
            int grp = -1;
            if (w[u] != Acc(0)) {
                if (pass == 0) grp = 0;
                else {
                    const unsigned long long pre = key >> (shift + 8);
                    for (int q = 0; q < G; ++q) if (s.prefix[q] == pre) grp = q;
                }
            }
            if constexpr (COLLECT) {
                if (grp >= 0) {
                    const unsigned at = atomicAdd(&s.list_n[grp], 1u);     // < count[grp] <= LIST for a table nobody writes
                    if (at < (unsigned)P::LIST) {
                        s.list[grp * P::LIST + at] = key;
                        if constexpr (P::WEIGHTED) s.list_w[grp * P::LIST + at] = w[u];
                    }
                }
            } else {
                const unsigned bin = grp >= 0 ? (unsigned)(grp * 256 + (int)((key >> shift) & 0xFF)) : 0xFFFFFFFFu;
                bool pending = grp >= 0;
                // lanes of the wavefront on the same bin: one add of what they merge to (twice; what is left adds one by one)
#pragma unroll
                for (int it = 0; it < P::MERGE_ROUNDS; ++it) {
                    const unsigned long long m = __ballot(pending);
                    if (m != 0ull) {
                        const int leader = __ffsll((long long)m) - 1;
                        const unsigned b0 = (unsigned)__shfl((int)bin, leader);
                        const bool same = pending && bin == b0;
                        const unsigned long long sm = __ballot(same);
                        // few lanes on the leader's bin (uniform: sm is a ballot): the digits are spread, a reduction would cost
                        // more than the adds it saves, here and in the next round -- what is pending adds one by one
                        if (P::MERGE_MIN > 1 && __popcll(sm) < P::MERGE_MIN) break;
                        const Acc sum = P::merged(w[u], same, sm);
                        if (lane == leader) {
                            atomicAdd(&s.hist[b0], sum);
                            if constexpr (P::WEIGHTED) atomicAdd(&s.chist[b0], (unsigned)__popcll(sm));
                        }
                        if (same) pending = false;
                    }
                }
                if (pending) {
                    atomicAdd(&s.hist[bin], w[u]);
                    if constexpr (P::WEIGHTED) atomicAdd(&s.chist[bin], 1u);
                }
            }
        }
    }
}

template <class P>
__device__ __forceinline__ void radix_select(const typename P::Args& g, SelShared<P>& s)
{
    using Acc = typename P::Acc;
    const int T = P::wanted(g);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int max_sweeps = 0;
    for (long long r = blockIdx.x; r < g.n_rows; r += gridDim.x) {
        const double* row = g.table + (size_t)r * g.E;
        __syncthreads();                           // the previous row's state is no longer read
        if (tid < T) { s.rem[tid] = P::rem0(g, tid); s.group[tid] = 0; }
        if (tid == 0) { s.G = 1; s.prefix[0] = 0ull; s.collect = 0; }
        __syncthreads();
        int sweeps = 0;
        bool done = false;
        for (int pass = 0; pass < 8 && !done; ++pass) {
            const int G = s.G;
            if (s.collect) {                       // uniform: written before the last barrier
                if (tid < G) s.list_n[tid] = 0u;
                __syncthreads();
                select_sweep<P, true>(g, row, s, pass);
                ++sweeps;
                __syncthreads();
                // a wavefront per wanted value: lane i places the bucket's i-th key by adding up the keys below and beside it
                for (int t = wave; t < T; t += QSEL_THREADS / 64) {
                    const int q = s.group[t];
                    const unsigned n = s.count[q];
                    const unsigned long long want = s.rem[t];
                    if ((unsigned)lane < n) {
                        const unsigned long long mine = s.list[q * P::LIST + lane];
                        Acc less = 0, equal = 0;
                        for (unsigned i = 0; i < n; ++i) {
                            const unsigned long long o = s.list[q * P::LIST + i];
                            Acc ow = 1;
                            if constexpr (P::WEIGHTED) ow = s.list_w[q * P::LIST + i];
                            less += o < mine ? ow : Acc(0);
                            equal += o == mine ? ow : Acc(0);
                        }
                        if (less <= want && want < less + equal)       // lanes holding equal keys store the same value
                            g.order_stats[P::plane(g, t) * g.out_stride + g.out_row0 + r] = quantile_value(mine);
                    }
                }
                done = true;
                break;
            }
            for (int i = tid; i < G * 256; i += QSEL_THREADS) {
                s.hist[i] = 0;
                if constexpr (P::WEIGHTED) s.chist[i] = 0u;
            }
            __syncthreads();
            select_sweep<P, false>(g, row, s, pass);
            ++sweeps;
            __syncthreads();
            // every wanted value walks its group's histogram to its digit
            if (tid < T) {
                const int q = s.group[tid];
                const Acc* h = s.hist + q * 256;
                unsigned long long rem = s.rem[tid];
                int d = 0;
                for (; d < 255; ++d) { const Acc c = h[d]; if (rem < c) break; rem -= c; }
                s.rem[tid] = rem;
                s.t_prefix[tid] = (s.prefix[q] << 8) | (unsigned long long)d;
                if constexpr (P::WEIGHTED) s.t_count[tid] = s.chist[q * 256 + d];
                else s.t_count[tid] = h[d];
            }
            __syncthreads();
            if (tid == 0) {                        // wanted values with equal prefixes share a group from here on
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
                s.collect = (biggest <= (unsigned)P::LIST) ? 1 : 0;
            }
            __syncthreads();
        }
        if (!done && tid < T)                      // all 64 bits settled: the prefix is the key
            g.order_stats[P::plane(g, tid) * g.out_stride + g.out_row0 + r] = quantile_value(s.prefix[s.group[tid]]);
        max_sweeps = sweeps > max_sweeps ? sweeps : max_sweeps;
    }
    if (tid == 0 && max_sweeps > 0) atomicMax(g.n_passes, max_sweeps);
}

__global__ __launch_bounds__(QSEL_THREADS) void quantile_select_kernel(const QuantileArgs g)
{
    __shared__ SelShared<QSelect> s;
    radix_select<QSelect>(g, s);
}

__global__ __launch_bounds__(QSEL_THREADS) void weighted_select_kernel(const WQuantileArgs g)
{
    __shared__ SelShared<WQSelect> s;
    radix_select<WQSelect>(g, s);
}

}  // namespace simplyp
