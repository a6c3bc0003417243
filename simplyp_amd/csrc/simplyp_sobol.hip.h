// simplyp_sobol.hip.h -- Sobol' sensitivity indices of an ensemble, bootstrapped on the device (gfx950): Saltelli's design of
// N (d + 2) members, the first- and total-order indices of Saltelli et al. 2010 with the Sobol'-Levitan centring (what
// scipy.stats.sobol_indices computes), and their bootstrap as a dense fp64 contraction of resampling counts with per-sample terms.
// simplyp_amd/sobol.py states all of it in NumPy.
//
//   simplyp_sobol_design_kernel     lane = member j N + n: x = lo + (hi - lo) u, written to x [n_dim][E] and scattered through target[]
//   simplyp_sobol_mean_kernel       block = row: valid[N] (no member of the sample carries SIMPLYP_STATUS_NONFINITE), mu of the row
//   simplyp_sobol_counts_kernel     block = resample: a histogram of the N bootstrap indices in LDS, 16-bit bins packed in pairs
//   simplyp_sobol_contract_kernel   sums[b][r][:] = sum_n C[b][n] terms[r][n][:], v_mfma_f64_16x16x4_f64
//   simplyp_sobol_epilogue_kernel   lane = (row, resample): the ratios from the sums
//
// The draws are counter-based (Philox4x32-10, simplyp_predictive.hip.h), key (seed & 0xffffffff, seed >> 32):
//   design   counter (n, k, m, 0x53454E53), m = 0: A, 1: B: u = uniform(x0, x1)
//   bootstrap counter (b, j >> 2, 0, 0x424F4F54): idx(b, j) = (x_{j & 3} N) >> 32, j < N, b >= 1; resample 0 is c = 1
//
// The contraction: a block owns a row and 64 resamples (4 waves x 16) and walks the samples in chunks of 64.  Per chunk the 256
// lanes load a, b, ab_i coalesced from table[r][j N + n], subtract mu, and form the 2 d + 2 terms once into LDS (an invalid
// sample's terms are selected to 0, never multiplied by 0); every wave then issues 16 k-steps of the 16x16x4 MFMA per 16-column
// tile: A = its counts tile converted to fp64, one value per lane, A[l & 15][k = l >> 4]; B = the terms, B[k = l >> 4][l & 15];
// C/D col = lane & 15, row = (lane >> 4) + 4 reg.  Lane half h takes samples 16 h .. 16 h + 15 of the chunk as its k values, so a
// lane's 16 counts are 32 contiguous bytes of a row of C.  C's rows are padded with zeros to a multiple of 64 samples, which is
// also the K tail.  One accumulator per tile lives through all chunks: no split over n, no floating-point atomic, one fixed
// order of additions -- the same call twice gives the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simplyp.h"
#include "simplyp_mcmc.hip.h"              // MCMC_MAX_DIM, MCMC_TARGET_*
#include "simplyp_predictive.hip.h"        // philox4x32_10, philox_uniform

namespace simplyp {

constexpr int SOBOL_MAX_DIM = MCMC_MAX_DIM;
constexpr int SOBOL_MIN_N = 2, SOBOL_MAX_N = 32768;
constexpr int SOBOL_MAX_BOOT = 1 << 20;
constexpr uint32_t SOBOL_DESIGN_STREAM = 0x53454E53u;  // "SENS"
constexpr uint32_t SOBOL_BOOT_STREAM = 0x424F4F54u;    // "BOOT"
constexpr int SOBOL_THREADS = 256;
constexpr int SOBOL_KC = 64;                           // samples per chunk; the rows of C are padded to a multiple of it
constexpr int SOBOL_RB = 64;                           // resamples per block: 4 waves x 16 rows

struct SobolDesignArgs {
    int N, n_dim;
    uint32_t key0, key1;
    double lo[SOBOL_MAX_DIM], hi[SOBOL_MAX_DIM];
    int target[SOBOL_MAX_DIM];
    const double* unit;                    // [2][n_dim][N] or nullptr
    double* x;                             // [n_dim][E]
    double* member_params;                 // [NP_M][E]
    double* f_tdp;                         // [E]
};

struct SobolArgs {
    int N, Npad, n_dim, n_rows, B;         // B = 1 + n_boot
    uint32_t key0, key1;
    const double* table;                   // [n_rows][E]
    const int32_t* status;                 // [E] or nullptr
    uint8_t* valid;                        // [Npad]
    double* mu;                            // [n_rows]
    int32_t* n_valid;                      // [1]
    uint16_t* counts;                      // [B][Npad]
    int32_t* n_used;                       // [B]
    double* sums;                          // [B][n_rows][2 n_dim + 2]
    double* indices;                       // [2][n_dim][n_rows][B]
};

__global__ __launch_bounds__(SOBOL_THREADS) void simplyp_sobol_design_kernel(const SobolDesignArgs g)
{
    const int e = blockIdx.x * SOBOL_THREADS + threadIdx.x;
    const int N = g.N, d = g.n_dim, E = N * (d + 2);
    if (e >= E) return;
    const int j = e / N, n = e - j * N;
    for (int k = 0; k < d; ++k) {
        const int m = (j == 1 || j == 2 + k) ? 1 : 0;              // B itself, or AB_k's own dimension
        double u;
        if (g.unit) {
            u = g.unit[((size_t)m * d + k) * N + n];
        } else {
            const Philox4 r = philox4x32_10((uint32_t)n, (uint32_t)k, (uint32_t)m, SOBOL_DESIGN_STREAM, g.key0, g.key1);
            u = philox_uniform(r.x0, r.x1);
        }
        const double x = g.lo[k] + (g.hi[k] - g.lo[k]) * u;
        g.x[(size_t)k * E + e] = x;
        const int tg = g.target[k];
        if (tg == MCMC_TARGET_NONE) continue;
        if (tg == MCMC_TARGET_F_TDP) g.f_tdp[e] = x;
        else g.member_params[(size_t)tg * E + e] = x;
    }
}

// s + e = a + b exactly (Knuth); the library is built without contraction or reassociation.
__device__ __forceinline__ void sobol_two_sum(double a, double b, double& s, double& e)
{
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}

// (hi, lo) += (h2, l2) in double-double, renormalised.
__device__ __forceinline__ void sobol_dd_add(double& hi, double& lo, double h2, double l2)
{
    double s, e;
    sobol_two_sum(hi, h2, s, e);
    e = e + (lo + l2);
    hi = s + e;
    lo = e - (hi - s);
}

// valid[n] and the row's mu = sum_valid (a + b) / (2 n_valid).  Each a + b is one fp64 addition; their sum is accumulated in
// double-double (a lane's samples n = t, t + 256, .. in order, then a halving tree over the lanes), which carries ~106 bits: the
// rounded result is the exactly rounded sum whatever the order -- what math.fsum gives the NumPy statement -- unless the exact sum
// lies within ~N 2^-106 of a rounding boundary.  So a, b, ab_i and every term are the mirror's bits, and the sums differ from it
// by their order of addition alone.
__global__ __launch_bounds__(SOBOL_THREADS) void simplyp_sobol_mean_kernel(const SobolArgs g)
{
    __shared__ double red_hi[SOBOL_THREADS];
    __shared__ double red_lo[SOBOL_THREADS];
    __shared__ int cnt[SOBOL_THREADS];
    const int r = blockIdx.x, t = threadIdx.x, N = g.N, J = g.n_dim + 2;
    const double* row = g.table + (size_t)r * N * J;
    double hi = 0.0, lo = 0.0;
    int c = 0;
    for (int n = t; n < g.Npad; n += SOBOL_THREADS) {
        bool v = n < N;
        if (v && g.status)
            for (int j = 0; j < J; ++j) v = v && ((g.status[(size_t)j * N + n] & SIMPLYP_STATUS_NONFINITE) == 0);
        if (v) { sobol_dd_add(hi, lo, row[n] + row[N + n], 0.0); c += 1; }
        if (r == 0) g.valid[n] = v ? 1 : 0;
    }
    red_hi[t] = hi; red_lo[t] = lo; cnt[t] = c;
    __syncthreads();
    for (int s = SOBOL_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
            sobol_dd_add(hi, lo, red_hi[t + s], red_lo[t + s]);
            red_hi[t] = hi; red_lo[t] = lo; cnt[t] += cnt[t + s];
        }
        __syncthreads();
    }
    if (t == 0) {
        g.mu[r] = hi / (2.0 * (double)cnt[0]);
        if (r == 0) *g.n_valid = cnt[0];
    }
}

// C[b][n]: resample 0 all ones; resample b >= 1 the histogram of idx(b, j), j < N.  The bins are 16 bits wide, two to an LDS
// word, and take integer LDS atomics: a bin holds at most N <= 32768, so no carry reaches its neighbour.  n_used[b] = sum c v.
// Dynamic LDS: max(Npad / 2, 256) words.
__global__ __launch_bounds__(SOBOL_THREADS) void simplyp_sobol_counts_kernel(const SobolArgs g)
{
    extern __shared__ uint32_t sobol_bins[];
    const int b = blockIdx.x, t = threadIdx.x, N = g.N, W = g.Npad >> 1;
    for (int w = t; w < W; w += SOBOL_THREADS) sobol_bins[w] = 0u;
    __syncthreads();
    if (b > 0) {
        const int Q = (N + 3) >> 2;
        for (int q = t; q < Q; q += SOBOL_THREADS) {
            const Philox4 x = philox4x32_10((uint32_t)b, (uint32_t)q, 0u, SOBOL_BOOT_STREAM, g.key0, g.key1);
            const int j = 4 * q;
            const uint32_t i0 = (uint32_t)(((unsigned long long)x.x0 * (unsigned long long)N) >> 32);
            const uint32_t i1 = (uint32_t)(((unsigned long long)x.x1 * (unsigned long long)N) >> 32);
            const uint32_t i2 = (uint32_t)(((unsigned long long)x.x2 * (unsigned long long)N) >> 32);
            const uint32_t i3 = (uint32_t)(((unsigned long long)x.x3 * (unsigned long long)N) >> 32);
            atomicAdd(&sobol_bins[i0 >> 1], 1u << (16 * (i0 & 1u)));
            if (j + 1 < N) atomicAdd(&sobol_bins[i1 >> 1], 1u << (16 * (i1 & 1u)));
            if (j + 2 < N) atomicAdd(&sobol_bins[i2 >> 1], 1u << (16 * (i2 & 1u)));
            if (j + 3 < N) atomicAdd(&sobol_bins[i3 >> 1], 1u << (16 * (i3 & 1u)));
        }
    }
    __syncthreads();
    int used = 0;
    uint16_t* out = g.counts + (size_t)b * g.Npad;
    for (int n = t; n < g.Npad; n += SOBOL_THREADS) {
        uint32_t c = 0u;
        if (n < N) c = b == 0 ? 1u : ((sobol_bins[n >> 1] >> (16 * (n & 1))) & 0xFFFFu);
        out[n] = (uint16_t)c;
        if (g.valid[n]) used += (int)c;                                // valid[n] = 0 for n >= N
    }
    __syncthreads();                                                   // the bins have been read: they carry the block's sum now
    int* red = (int*)sobol_bins;
    red[t] = used;
    __syncthreads();
    for (int s = SOBOL_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    if (t == 0) g.n_used[b] = red[0];
}

typedef double sobol_acc_t __attribute__((ext_vector_type(4)));

// CT: 16-column tiles of the 2 d + 2 term columns (1..3).  Grid (n_rows, ceil(B / 64)).
template <int CT>
__global__ __launch_bounds__(SOBOL_THREADS) void simplyp_sobol_contract_kernel(const SobolArgs g)
{
    constexpr int LD = CT * 16 + 1;                                    // odd: the four lane halves' 128-byte reads fall on two bank phases
    __shared__ double terms[SOBOL_KC * LD];
    const int r = blockIdx.x, t = threadIdx.x, N = g.N, d = g.n_dim, T = 2 * d + 2;
    const int lane = t & 63, wave = t >> 6;
    const int s_own = t & (SOBOL_KC - 1);                              // the sample of the chunk this lane forms terms for
    const double* row = g.table + (size_t)r * N * (d + 2);
    const double mu = g.mu[r];
    const int b_base = blockIdx.y * SOBOL_RB + wave * 16;
    const bool wave_on = b_base < g.B;                                 // wave-uniform
    const int b_lane = min(b_base + (lane & 15), g.B - 1);             // rows past the end read the last row; nothing of them is written
    const int h = lane >> 4;
    const uint16_t* crow = g.counts + (size_t)b_lane * g.Npad + 16 * h;

    for (int i = t; i < SOBOL_KC * LD; i += SOBOL_THREADS) terms[i] = 0.0;     // the padding columns stay 0
    sobol_acc_t acc[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) acc[c] = sobol_acc_t{0.0, 0.0, 0.0, 0.0};

    for (int n0 = 0; n0 < g.Npad; n0 += SOBOL_KC) {
        __syncthreads();                                               // the last chunk's terms have been read
        const int n = n0 + s_own;
        const bool ok = g.valid[n] != 0;                               // valid[] is Npad long, 0 past N
        double a = 0.0, b = 0.0;
        if (n < N) { a = row[n] - mu; b = row[N + n] - mu; }
        double* trow = terms + s_own * LD;
        if (wave == 0) {
            trow[0] = ok ? a + b : 0.0;
            trow[1] = ok ? a * a + b * b : 0.0;
        }
        for (int i = wave; i < d; i += 4) {
            double ab = 0.0;
            if (n < N) ab = row[(size_t)(2 + i) * N + n] - mu;
            const double gi = b * (ab - a), ti = (a - ab) * (a - ab);
            trow[2 + i] = ok ? gi : 0.0;
            trow[2 + d + i] = ok ? ti : 0.0;
        }
        uint4 c_lo = uint4{0u, 0u, 0u, 0u}, c_hi = c_lo;
        if (wave_on) {
            c_lo = *(const uint4*)(crow + n0);
            c_hi = *(const uint4*)(crow + n0 + 8);
        }
        __syncthreads();
        if (wave_on) {
            const uint32_t w[8] = {c_lo.x, c_lo.y, c_lo.z, c_lo.w, c_hi.x, c_hi.y, c_hi.z, c_hi.w};
            const double* brow = terms + (16 * h) * LD + (lane & 15);
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) {
                const double cnt = (double)((w[kk >> 1] >> (16 * (kk & 1))) & 0xFFFFu);
#pragma unroll
                for (int c = 0; c < CT; ++c)
                    acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(cnt, brow[kk * LD + 16 * c], acc[c], 0, 0, 0);
            }
        }
    }
    if (!wave_on) return;
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        const int col = 16 * c + (lane & 15);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int bb = b_base + h + 4 * i;
            if (bb < g.B && col < T) g.sums[((size_t)bb * g.n_rows + r) * T + col] = acc[c][i];
        }
    }
}

// m1 = P / (2 n_c), m2 = S / (2 n_c), var = m2 - m1 m1, S1_i = (G_i / n_c) / var, ST_i = (0.5 (T_i / n_c)) / var: IEEE, so a
// constant row (var = 0) gives NaN.  The resample axis is the fastest of indices [2][n_dim][n_rows][B].
__global__ __launch_bounds__(SOBOL_THREADS) void simplyp_sobol_epilogue_kernel(const SobolArgs g)
{
    const long long idx = (long long)blockIdx.x * SOBOL_THREADS + threadIdx.x;
    const long long total = (long long)g.n_rows * g.B;
    if (idx >= total) return;
    const int b = (int)(idx % g.B);
    const long long r = idx / g.B;
    const int d = g.n_dim, T = 2 * d + 2;
    const double* s = g.sums + ((size_t)b * g.n_rows + r) * T;
    const double n_c = (double)g.n_used[b];
    const double m1 = s[0] / (2.0 * n_c), m2 = s[1] / (2.0 * n_c);
    const double var = m2 - m1 * m1;
    const size_t plane = (size_t)d * g.n_rows * g.B;
    for (int i = 0; i < d; ++i) {
        double* dst = g.indices + ((size_t)i * g.n_rows + r) * g.B + b;
        dst[0] = (s[2 + i] / n_c) / var;
        dst[plane] = (0.5 * (s[2 + d + i] / n_c)) / var;
    }
}

}  // namespace simplyp
