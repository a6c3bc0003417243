// simplyp_time_quantile.hip.h -- exact order statistics along the DAY axis of a run's device table [n_cols][D][R][E] (gfx950).
//
// What the reference's users make of every run with one DataFrame.quantile() call on what run_simply_p returns: the
// flow-duration curve (Q95, Q50, Q10), annual maxima (q = 1), the annual 90th percentile of a concentration, the same for a
// season -- per member, so the result keeps the member axis and composes with the other reductions of the library.  For every
// (series, period, reach, member) and each of K probabilities the kernel returns the two order statistics x_(k_lo), x_(k_hi)
// that bracket numpy's 'linear' quantile (k_lo = floor(q (n - 1)), k_hi = min(k_lo + 1, n - 1), n = the period's days); the
// host interpolates.  Ordering is quantile_key's (simplyp_quantile.hip.h): NaN after +inf, -0.0 and +0.0 tied.
//
// A series is a column of the table, or one of the six series of the reference's df_R computed on the fly from Qr and the
// flux columns with the expressions of spearman_sim_value (simplyp_gof.hip.h), operation for operation.
//
// Layout: one 64-lane workgroup per (64 member slots, period, series x reach); lane = member slot, so every load of a wave
// is one 512-byte segment of a day's row, and a lane owns its member from the first digit to the last: no lane ever reads
// what another wrote, so the kernel has no barrier and no atomic that two lanes share.  Per lane a most-significant-digit
// radix select, 8 bits per sweep, over the period's days:
//   * the lane's 256-bin histogram is a column of hist[256][64] in LDS (64 KiB; lane l always hits bank l mod 32);
//   * the 2K wanted ranks (k_lo and k_hi of each probability; the host hands them over ascending and without repeats) are
//     refined together: ranks of a lane that still share a key prefix share one sweep ("group"); where the lanes' groups
//     differ, the wave sweeps once per group index (a lane with fewer groups idles in the extra sweeps);
//   * as soon as the buckets of every lane's groups hold <= TQ_LIST keys together, one last sweep collects them into the same
//     LDS (now a list[128][64] of keys), every lane sorts its buckets there by insertion, and the ranks index the sorted
//     buckets.  A period of <= 128 days takes this path at once: one sweep.  Smooth positive series within a few binades
//     settle after 2-3 digits (3-4 sweeps for 30 years of days); heavy ties run all 8 digits, then the prefix is the key.
// k_lo and k_hi are adjacent, so they part only when k_lo is the last of its bucket -- they cost a sweep of their own only
// then, instead of one extra sweep for the upper values always.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simplyp.h"
#include "simplyp_quantile.hip.h"      // quantile_key, quantile_value

namespace simplyp {

constexpr int TQ_MAX_K = 16;               // probabilities per call
constexpr int TQ_MAX_SERIES = 32;
constexpr int TQ_LIST = 128;               // keys per lane the LDS list holds: 128 x 64 x 8 B = the histogram's 64 KiB
constexpr int TQ_BATCH = 8;                // day rows whose loads are issued together

struct TqArgs {
    int E, R, D, K, T;                     // T = ranks per period (<= 2K)
    int n_series, n_periods;               // n_periods >= 1
    const double* out;                     // [n_cols][D][R][E]
    long long col_stride;                  // D*R*E
    int col[4];                            // column slots of Qr, Msus_kg/day, TDP_kg/day, PP_kg/day (derived series only)
    int series[TQ_MAX_SERIES];             // >= 0: column slot; < 0: derived, -1 - SIMPLYP_GOF_*
    const int32_t* member_of_slot;         // [E] or nullptr
    const double* f_tdp;                   // [E] member order (derived only)
    const double* a_catch;                 // [S][E] member order (derived only)
    const int32_t* reach_of;               // [R]
    const int32_t* day;                    // the participating days, period after period
    const int32_t* day_ptr;                // [n_periods + 1] offsets into day
    const int32_t* ranks;                  // [n_periods][T] ascending; rows with fewer distinct ranks repeat their last
    const uint8_t* rank_of;                // [n_periods][2][K]: position in the period's rank row of k_lo, k_hi
    double* order_stats;                   // [2][K][n_series][n_periods][R][E]
    int* n_sweeps;                         // max over workgroups (atomicMax)
    unsigned long long* rows_read;         // 512-byte row segments loaded by all sweeps (atomicAdd)
};

template <int TMAX>
struct alignas(16) TqShared {
    unsigned hist[256 * 64];               // [bin][lane]; in the collecting sweep a list[TQ_LIST][lane] of 64-bit keys
    unsigned long long pre[TMAX][64];      // per rank: the key bits settled so far (right-aligned)
    unsigned rem[TMAX][64];                // per rank: its rank inside the bucket of that prefix
    unsigned cnt[TMAX][64];                // per rank: the bucket's size
    unsigned pos[TMAX][64];                // per group (at its first rank): where the bucket's next key goes in the list
};

// The series of one (workgroup, lane).  KIND 0: a column.  1: Q_cumecs = Qr*A*1000/86400.  2: (flux/Qr)/A, times f (f = 1
// except for SRP = TDP*f_TDP; x*1.0 is x).  3: TP = TDP + PP.
struct TqSeries {
    const double* p0;                      // the column, or Qr
    const double* p1;                      // flux (KIND 2), TDP flux (KIND 3)
    const double* p2;                      // PP flux (KIND 3)
    double A, f;
};

template <int KIND>
__device__ __forceinline__ double tq_value(const TqSeries& s, double a, double b, double c)
{
    if constexpr (KIND == 0) return a;
    else if constexpr (KIND == 1) return a * s.A * 1000 / 86400;
    else if constexpr (KIND == 2) return ((b / a) / s.A) * s.f;
    else return (b / a) / s.A + (c / a) / s.A;
}

// The series `code` (>= 0: column slot; < 0: derived, -1 - SIMPLYP_GOF_*) at element `base` of a day's rows: its pointers at
// day 0, A = a_catch[a_index] and f (f_tdp[member] for SRP).  col: the slots of Qr and the three fluxes.  Returns KIND.
__device__ __forceinline__ int tq_series(TqSeries& sr, int code, const double* out, long long col_stride, const int* col,
                                         size_t base, const double* a_catch, const double* f_tdp, size_t a_index, int member)
{
    sr.p1 = sr.p2 = nullptr;
    sr.A = sr.f = 1.0;
    if (code >= 0) {
        sr.p0 = out + (size_t)code * col_stride + base;
        return 0;
    }
    const int var = -1 - code;
    sr.A = a_catch[a_index];
    sr.p0 = out + (size_t)col[0] * col_stride + base;
    if (var == SIMPLYP_GOF_Q) return 1;
    if (var == SIMPLYP_GOF_TP) {
        sr.p1 = out + (size_t)col[2] * col_stride + base;
        sr.p2 = out + (size_t)col[3] * col_stride + base;
        return 3;
    }
    const int c = var == SIMPLYP_GOF_SS ? 1 : var == SIMPLYP_GOF_PP ? 3 : 2;          // SS, PP, and TDP / SRP from the TDP flux
    sr.p1 = out + (size_t)col[c] * col_stride + base;
    if (var == SIMPLYP_GOF_SRP) sr.f = f_tdp[member];
    return 2;
}

template <int KIND>
__device__ __forceinline__ unsigned long long tq_key(const TqSeries& s, double a, double b, double c)
{
    return quantile_key(tq_value<KIND>(s, a, b, c));
}

// f(key) for every participating day of the period, TQ_BATCH rows in flight.
template <int KIND, typename F>
__device__ __forceinline__ void tq_sweep(const TqSeries& s, const int32_t* day, int n, size_t day_stride, F&& f)
{
    int i = 0;
    for (; i + TQ_BATCH <= n; i += TQ_BATCH) {
        double a[TQ_BATCH], b[TQ_BATCH], c[TQ_BATCH];
#pragma unroll
        for (int j = 0; j < TQ_BATCH; ++j) {
            const size_t off = (size_t)day[i + j] * day_stride;
            a[j] = s.p0[off];
            b[j] = KIND >= 2 ? s.p1[off] : 0.0;
            c[j] = KIND == 3 ? s.p2[off] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < TQ_BATCH; ++j) f(tq_key<KIND>(s, a[j], b[j], c[j]));
    }
    for (; i < n; ++i) {
        const size_t off = (size_t)day[i] * day_stride;
        f(tq_key<KIND>(s, s.p0[off], KIND >= 2 ? s.p1[off] : 0.0, KIND == 3 ? s.p2[off] : 0.0));
    }
}

// One period of one lane's series.  Leaves the lane's answers where tq_answer finds them; returns the sweeps made.
// level_out: 8 when every digit was settled (answers are the prefixes), else the answers are in the sorted list.
template <int TMAX, int KIND>
__device__ __forceinline__ int tq_select(TqShared<TMAX>& s, const TqSeries& sr, const int32_t* day, int n, size_t day_stride,
                                         const int32_t* ranks, int T, int lane, int& level_out)
{
    unsigned long long* list = reinterpret_cast<unsigned long long*>(s.hist);
    for (int t = 0; t < T; ++t) {
        s.pre[t][lane] = 0ull;
        s.rem[t][lane] = (unsigned)ranks[t];
        s.cnt[t][lane] = (unsigned)n;
    }
    int sweeps = 0, level = 0;
    for (;; ++level) {
        // the lane's groups: a rank whose prefix differs from its predecessor's starts one (prefixes ascend with the ranks)
        unsigned total = 0, lead = 0;
        for (int t = 0; t < T; ++t) {
            if (t == 0 || s.pre[t][lane] != s.pre[t - 1][lane]) { total += s.cnt[t][lane]; lead |= 1u << t; }
        }
        if (level == 8) break;                                         // all 64 bits settled
        if (__all(total <= (unsigned)TQ_LIST)) {
            // ---- collect the groups' buckets, sort each, done
            unsigned at = 0;
            for (int t = 0; t < T; ++t)
                if ((lead >> t) & 1u) { s.pos[t][lane] = at; at += s.cnt[t][lane]; }
            const int pshift = 64 - 8 * level;
            tq_sweep<KIND>(sr, day, n, day_stride, [&](unsigned long long key) {
                const unsigned long long x = level == 0 ? 0ull : key >> pshift;
                for (int t = 0; t < T; ++t) {
                    if (((lead >> t) & 1u) && s.pre[t][lane] == x) {
                        const unsigned p = s.pos[t][lane];
                        if (p < (unsigned)TQ_LIST) { list[p * 64 + lane] = key; s.pos[t][lane] = p + 1; }
                    }
                }
            });
            ++sweeps;
            for (int t = 0; t < T; ++t) {
                if (!((lead >> t) & 1u)) continue;
                const int end = (int)s.pos[t][lane], start = end - (int)s.cnt[t][lane];
                for (int i = start + 1; i < end; ++i) {
                    const unsigned long long key = list[i * 64 + lane];
                    int j = i;
                    while (j > start && list[(j - 1) * 64 + lane] > key) { list[j * 64 + lane] = list[(j - 1) * 64 + lane]; --j; }
                    list[j * 64 + lane] = key;
                }
            }
            // every rank: the list index of its answer
            unsigned start = 0;
            for (int t = 0; t < T; ++t) {
                if ((lead >> t) & 1u) start = s.pos[t][lane] - s.cnt[t][lane];
                s.rem[t][lane] = start + s.rem[t][lane];
            }
            break;
        }
        // ---- one more digit: a sweep per group index
        const int shift = 56 - 8 * level;
        int cur = 0;
        while (__any(cur < T)) {
            for (int b = 0; b < 256; ++b) s.hist[b * 64 + lane] = 0u;
            const bool on = cur < T;
            const unsigned long long P = on ? s.pre[cur][lane] : 0ull;
            tq_sweep<KIND>(sr, day, n, day_stride, [&](unsigned long long key) {
                if (on && (level == 0 || (key >> (shift + 8)) == P))
                    atomicAdd(&s.hist[(unsigned)((key >> shift) & 0xFFull) * 64 + lane], 1u);
            });
            ++sweeps;
            if (on) {
                // the group's ranks ascend: one walk of the histogram serves them all
                int d = 0, t = cur;
                unsigned below = 0, c = s.hist[lane];
                for (; t < T && s.pre[t][lane] == P; ++t) {
                    const unsigned r = s.rem[t][lane];
                    while (r >= below + c && d < 255) { below += c; ++d; c = s.hist[d * 64 + lane]; }
                    s.pre[t][lane] = (P << 8) | (unsigned long long)d;
                    s.rem[t][lane] = r - below;
                    s.cnt[t][lane] = c;
                }
                cur = t;
            }
        }
    }
    level_out = level;
    return sweeps;
}

template <int TMAX, int KIND>
__device__ __forceinline__ void tq_periods(const TqArgs& g, TqShared<TMAX>& s, const TqSeries& sr, int si, int r, int slot, bool live)
{
    const int lane = threadIdx.x;
    const size_t day_stride = (size_t)g.R * g.E;
    const int loads = KIND == 0 || KIND == 1 ? 1 : KIND == 2 ? 2 : 3;
    const unsigned long long* list = reinterpret_cast<const unsigned long long*>(s.hist);
    int max_sweeps = 0;
    unsigned long long rows = 0ull;
    for (int p = blockIdx.y; p < g.n_periods; p += gridDim.y) {
        const int d0 = g.day_ptr[p], n = g.day_ptr[p + 1] - d0;
        double* o = g.order_stats + (((size_t)si * g.n_periods + p) * g.R + r) * g.E + slot;
        const size_t k_stride = (size_t)g.n_series * g.n_periods * g.R * g.E;
        if (n <= 0) {
            if (live)
                for (int k = 0; k < 2 * g.K; ++k) o[(size_t)k * k_stride] = __longlong_as_double(0x7FF8000000000000ll);
            continue;
        }
        int level = 0;
        const int sweeps = tq_select<TMAX, KIND>(s, sr, g.day + d0, n, day_stride, g.ranks + (size_t)p * g.T, g.T, lane, level);
        max_sweeps = sweeps > max_sweeps ? sweeps : max_sweeps;
        rows += (unsigned long long)sweeps * (unsigned long long)n * loads;
        if (live) {
            const uint8_t* ro = g.rank_of + (size_t)p * 2 * g.K;
            for (int k = 0; k < 2 * g.K; ++k) {                        // k = plane * K + probability
                const int t = ro[k];
                const unsigned long long key = level == 8 ? s.pre[t][lane] : list[s.rem[t][lane] * 64 + lane];
                o[(size_t)k * k_stride] = quantile_value(key);
            }
        }
    }
    if (lane == 0 && max_sweeps > 0) {
        atomicMax(g.n_sweeps, max_sweeps);
        atomicAdd(g.rows_read, rows);
    }
}

// grid: (member blocks of 64, periods (strided), n_series * R)
template <int TMAX>
__global__ __launch_bounds__(64) void simplyp_time_quantile_kernel(const TqArgs g)
{
    __shared__ TqShared<TMAX> s;
    const int lane = threadIdx.x;
    const int si = blockIdx.z / g.R, r = blockIdx.z - si * g.R;
    const int raw = blockIdx.x * 64 + lane;
    const bool live = raw < g.E;
    const int slot = live ? raw : g.E - 1;                             // idle lanes of the last block shadow the last member
    TqSeries sr;
    const int member = g.member_of_slot && g.series[si] < 0 ? g.member_of_slot[slot] : slot;
    const int kind = tq_series(sr, g.series[si], g.out, g.col_stride, g.col, (size_t)r * g.E + slot,
                               g.a_catch, g.f_tdp, (size_t)g.reach_of[r] * g.E + member, member);
    if (kind == 0) tq_periods<TMAX, 0>(g, s, sr, si, r, slot, live);
    else if (kind == 1) tq_periods<TMAX, 1>(g, s, sr, si, r, slot, live);
    else if (kind == 2) tq_periods<TMAX, 2>(g, s, sr, si, r, slot, live);
    else tq_periods<TMAX, 3>(g, s, sr, si, r, slot, live);
}

}  // namespace simplyp
