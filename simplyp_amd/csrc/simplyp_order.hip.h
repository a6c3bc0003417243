// simplyp_order.hip.h -- the members' lane-slot order computed on the device (gfx950): order_members' rule (simplyp_order.h)
// as kernels that read the pilot's cost table d_cost[8][E] and write d_perm[E] on the run's stream, so that the host neither
// copies the costs nor waits for them.
//
//   order_stats_kernel    per member: total cost -> the sort key ((0xFFFFFFFF - total) << 32 | member), padded with all-ones to a
//                         power of two; per workgroup: sum and sum of squares of log2(cost + 1) for each window
//   order_cov_kernel      mean and 1 / deviation of each window from those sums (every workgroup forms them in the same order);
//                         per workgroup the 36 sums of products of the standardised windows
//   order_pca_kernel      one wavefront: the 8 x 8 covariance, cyclic Jacobi in ONE lane on LDS arrays (a few hundred flops a
//                         sweep; no second copy and no wait on the host), the eigenvectors of the 2nd and 3rd largest eigenvalues
//   order_sort_*          a bitonic network over the padded keys: 8192-key chunks in LDS, the longer strides in global memory.
//                         The keys are distinct integers (the member id is their low half), so every implementation of the
//                         sort gives the same array: block membership by total cost is the host's exactly
//   order_blocks_kernel   one workgroup per block of the total-cost order: its members sorted in LDS by (PC2, member), then by
//                         (sub-block, PC3, member) -- directions alternating as on the host --, written to d_perm
//
// Every reduction is a fixed tree (wave shuffles, then the waves of a workgroup in order, then the workgroups in order); there
// is no floating-point atomic and no atomic at all, so the same costs give the same order.  PC2 and PC3 are rounded as the
// device rounds them (a tree sum where the host adds in member order, the device's log2f): members may be ordered differently
// from the host's inside a block, which changes SIMT efficiency in the fourth digit and no result.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "simplyp_quantile.hip.h"

namespace simplyp {

constexpr int ORD_WIN = 8;                     // pilot windows
constexpr int ORD_THREADS = 1024;
constexpr int ORD_CHUNK = 8192;                // keys a workgroup sorts in LDS: 64 KB
constexpr int ORD_MAX_BLOCKS = 24, ORD_MAX_SUB = 6, ORD_MIN_BLOCK = 256;      // order_members' constants
constexpr int ORD_MAX_E = ORD_MAX_BLOCKS * ORD_CHUNK;     // a block of the total-cost order must fit one LDS sort
constexpr int ORD_NCOV = ORD_WIN * (ORD_WIN + 1) / 2;
constexpr int ORD_ID_BITS = 29;                // member id in the second key of a block: 3 bits of sub-block, 32 of PC3 above it
static_assert(ORD_MAX_E <= (1 << ORD_ID_BITS) && ORD_MAX_SUB <= 8, "the second key of a block holds sub-block, PC3 and member");

struct OrderArgs {
    int E, P;                                  // members; keys of the sort: a power of two >= max(E, ORD_CHUNK)
    int n_groups;                              // workgroups of the stats and covariance kernels: ceil(E / ORD_THREADS)
    int nb1, nb2;                              // blocks by total cost, sub-blocks by PC2
    const uint32_t* cost;                      // [ORD_WIN][E]
    unsigned long long* key;                   // [P]
    double* part_stats;                        // [n_groups][2 * ORD_WIN]: sum, sum of squares per window
    double* part_cov;                          // [n_groups][ORD_NCOV]
    double* moments;                           // [2 * ORD_WIN]: mean, 1 / deviation per window
    float* vec;                                // [2 * ORD_WIN]: eigenvectors of PC2 and PC3
    int32_t* perm;                             // [E]
};

__device__ __forceinline__ double ord_wave_sum(double v)
{
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

// Sum of v[0 .. N) over the workgroup into out[0 .. N) (thread 0 .. N - 1 write): the lanes of a wave by shuffles, the waves in
// order.  `lds` holds (ORD_THREADS / 64) * N doubles.
template <int N>
__device__ __forceinline__ void ord_group_sum(const double (&v)[N], double* lds, double* out)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double s = ord_wave_sum(v[k]);
        if (lane == 0) lds[wave * N + k] = s;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        double s = 0.0;
        for (int w = 0; w < ORD_THREADS / 64; ++w) s += lds[w * N + threadIdx.x];
        out[threadIdx.x] = s;
    }
}

__device__ __forceinline__ float ord_log_cost(uint32_t c) { return log2f((float)c + 1.0f); }

__global__ __launch_bounds__(ORD_THREADS) void order_stats_kernel(const OrderArgs g)
{
    __shared__ double lds[(ORD_THREADS / 64) * 2 * ORD_WIN];
    const int e = blockIdx.x * ORD_THREADS + threadIdx.x;
    double v[2 * ORD_WIN];
    uint32_t total = 0u;
#pragma unroll
    for (int w = 0; w < ORD_WIN; ++w) {
        const uint32_t c = e < g.E ? g.cost[(size_t)w * g.E + e] : 0u;
        const float l = e < g.E ? ord_log_cost(c) : 0.0f;
        total += c;
        v[w] = (double)l;
        v[ORD_WIN + w] = (double)l * (double)l;
    }
    if (e < g.P) g.key[e] = e < g.E ? ((unsigned long long)(0xFFFFFFFFu - total) << 32) | (unsigned)e : ~0ull;
    if (blockIdx.x < g.n_groups) ord_group_sum(v, lds, g.part_stats + (size_t)blockIdx.x * 2 * ORD_WIN);      // (uniform)
}

// What a member contributes to the principal components: its standardised log costs, as order_members forms them.
__device__ __forceinline__ void ord_standardised(const OrderArgs& g, const double* moments, int e, float (&z)[ORD_WIN])
{
#pragma unroll
    for (int w = 0; w < ORD_WIN; ++w) {
        const float m = (float)moments[w], inv = (float)moments[ORD_WIN + w];
        z[w] = (ord_log_cost(g.cost[(size_t)w * g.E + e]) - m) * inv;
    }
}

__global__ __launch_bounds__(ORD_THREADS) void order_cov_kernel(const OrderArgs g)
{
    __shared__ double lds[(ORD_THREADS / 64) * ORD_NCOV];
    __shared__ double sums[2 * ORD_WIN], mom[2 * ORD_WIN];
    if (threadIdx.x < 2 * ORD_WIN) {
        double s = 0.0;
        for (int b = 0; b < g.n_groups; ++b) s += g.part_stats[(size_t)b * 2 * ORD_WIN + threadIdx.x];
        sums[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x < ORD_WIN) {
        const double mean = sums[threadIdx.x] / g.E;
        const double var = sums[ORD_WIN + threadIdx.x] / g.E - mean * mean;
        const double inv = 1.0 / (sqrt(var > 0.0 ? var : 0.0) + 1e-12);
        mom[threadIdx.x] = mean;
        mom[ORD_WIN + threadIdx.x] = inv;
        if (blockIdx.x == 0) { g.moments[threadIdx.x] = mean; g.moments[ORD_WIN + threadIdx.x] = inv; }
    }
    __syncthreads();
    const int e = blockIdx.x * ORD_THREADS + threadIdx.x;
    float z[ORD_WIN];
    if (e < g.E) {
        ord_standardised(g, mom, e, z);
    } else {
#pragma unroll
        for (int w = 0; w < ORD_WIN; ++w) z[w] = 0.0f;
    }
    double v[ORD_NCOV];
    int k = 0;
#pragma unroll
    for (int i = 0; i < ORD_WIN; ++i)
#pragma unroll
        for (int j = i; j < ORD_WIN; ++j) v[k++] = (double)(z[i] * z[j]);
    ord_group_sum(v, lds, g.part_cov + (size_t)blockIdx.x * ORD_NCOV);
}

// One wavefront.  A and V live in LDS: a lane's private array with a run-time index would be scratch memory.
__global__ __launch_bounds__(64) void order_pca_kernel(const OrderArgs g)
{
    constexpr int n = ORD_WIN;
    __shared__ double A[n * n], V[n * n];
    const int lane = threadIdx.x;
    if (lane < ORD_NCOV) {
        double s = 0.0;
        for (int b = 0; b < g.n_groups; ++b) s += g.part_cov[(size_t)b * ORD_NCOV + lane];
        s /= g.E;
        int k = lane, i = 0;
        while (k >= n - i) { k -= n - i; ++i; }
        const int j = i + k;
        A[i * n + j] = s;
        A[j * n + i] = s;
    }
    V[lane] = (lane / n == lane % n) ? 1.0 : 0.0;
    __syncthreads();
    if (lane != 0) return;
    for (int sweep = 0; sweep < 50; ++sweep) {
        double off = 0.0;
        for (int i = 0; i < n; ++i) for (int j = i + 1; j < n; ++j) off += A[i * n + j] * A[i * n + j];
        if (off < 1e-22) break;
        for (int pi = 0; pi < n; ++pi)
            for (int qi = pi + 1; qi < n; ++qi) {
                const double apq = A[pi * n + qi];
                if (fabs(apq) < 1e-300) continue;
                const double theta = (A[qi * n + qi] - A[pi * n + pi]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
                for (int k = 0; k < n; ++k) {
                    const double akp = A[k * n + pi], akq = A[k * n + qi];
                    A[k * n + pi] = c * akp - sn * akq; A[k * n + qi] = sn * akp + c * akq;
                }
                for (int k = 0; k < n; ++k) {
                    const double apk = A[pi * n + k], aqk = A[qi * n + k];
                    A[pi * n + k] = c * apk - sn * aqk; A[qi * n + k] = sn * apk + c * aqk;
                }
                for (int k = 0; k < n; ++k) {
                    const double vkp = V[k * n + pi], vkq = V[k * n + qi];
                    V[k * n + pi] = c * vkp - sn * vkq; V[k * n + qi] = sn * vkp + c * vkq;
                }
            }
    }
    // the eigenvalues in descending order, equal ones by index: the second and the third
    int i2 = 0, i3 = 0;
    for (int x = 0; x < n; ++x) {
        int rank = 0;
        for (int y = 0; y < n; ++y) rank += (A[y * n + y] > A[x * n + x] || (A[y * n + y] == A[x * n + x] && y < x)) ? 1 : 0;
        if (rank == 1) i2 = x;
        if (rank == 2) i3 = x;
    }
    for (int w = 0; w < n; ++w) {
        g.vec[w] = (float)V[w * n + i2];
        g.vec[n + w] = (float)V[w * n + i3];
    }
}

// ---- the sort of the total-cost keys ------------------------------------------------------------------------------------------
// Strides j0, j0 / 2, .. 1 of stage k of the bitonic network on the ORD_CHUNK keys of a chunk that starts at `base` of the array.
__device__ __forceinline__ void ord_local_steps(unsigned long long* keys, int base, int k, int j0)
{
    for (int j = j0; j > 0; j >>= 1) {
        for (int t = threadIdx.x; t < ORD_CHUNK / 2; t += ORD_THREADS) {
            const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
            const bool asc = ((base + i) & k) == 0;
            const unsigned long long a = keys[i], b = keys[l];
            if ((a > b) == asc) { keys[i] = b; keys[l] = a; }
        }
        __syncthreads();
    }
}

// k_first = 2: every stage up to ORD_CHUNK (the chunk comes out sorted, up or down as stage 2 * ORD_CHUNK wants it);
// k_first > ORD_CHUNK: the strides below ORD_CHUNK of that stage alone.
__global__ __launch_bounds__(ORD_THREADS) void order_sort_chunk_kernel(unsigned long long* key, int k_first)
{
    __shared__ unsigned long long keys[ORD_CHUNK];
    const int base = blockIdx.x * ORD_CHUNK;
    for (int i = threadIdx.x; i < ORD_CHUNK; i += ORD_THREADS) keys[i] = key[(size_t)base + i];
    __syncthreads();
    if (k_first > ORD_CHUNK) ord_local_steps(keys, base, k_first, ORD_CHUNK / 2);
    else for (int k = 2; k <= ORD_CHUNK; k <<= 1) ord_local_steps(keys, base, k, k >> 1);
    for (int i = threadIdx.x; i < ORD_CHUNK; i += ORD_THREADS) key[(size_t)base + i] = keys[i];
}

// Stride j >= ORD_CHUNK of stage k, in global memory: P / 2 pairs.
__global__ __launch_bounds__(256) void order_sort_stride_kernel(unsigned long long* key, int P, int k, int j)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= P / 2) return;
    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
    const bool asc = (i & k) == 0;
    const unsigned long long a = key[i], b = key[l];
    if ((a > b) == asc) { key[i] = b; key[l] = a; }
}

// ---- the blocks ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned ord_float_key(float f, bool ascending)
{
    if (!ascending) f = -f;
    unsigned u = __float_as_uint(f);
    u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;
    return u;
}

__device__ __forceinline__ void ord_project(const OrderArgs& g, int e, float& pc2, float& pc3)
{
    float z[ORD_WIN];
    ord_standardised(g, g.moments, e, z);
    pc2 = 0.0f; pc3 = 0.0f;
#pragma unroll
    for (int w = 0; w < ORD_WIN; ++w) { pc2 += g.vec[w] * z[w]; pc3 += g.vec[ORD_WIN + w] * z[w]; }
}

// Workgroup b: positions [E b / nb1, E (b + 1) / nb1) of the sorted keys.
__global__ __launch_bounds__(ORD_THREADS) void order_blocks_kernel(const OrderArgs g)
{
    __shared__ unsigned long long keys[ORD_CHUNK];
    const int b = blockIdx.x;
    const int lo = (int)((long long)g.E * b / g.nb1), hi = (int)((long long)g.E * (b + 1) / g.nb1), cnt = hi - lo;
    if (cnt <= 0 || cnt > ORD_CHUNK) return;                   // (uniform; the host does not launch such a shape)
    int P = 2;
    while (P < cnt) P <<= 1;
    for (int i = threadIdx.x; i < P; i += ORD_THREADS) {
        unsigned long long k = ~0ull;
        if (i < cnt) {
            const unsigned e = min((unsigned)g.key[lo + i], (unsigned)(g.E - 1));
            float pc2, pc3;
            ord_project(g, (int)e, pc2, pc3);
            k = ((unsigned long long)ord_float_key(pc2, b % 2 == 0) << 32) | e;
        }
        keys[i] = k;
    }
    __syncthreads();
    bitonic_segments<ORD_THREADS, false>(keys, nullptr, P, P);
    for (int i = threadIdx.x; i < cnt; i += ORD_THREADS) {
        const unsigned e = (unsigned)keys[i];
        int c = g.nb2 - 1;
        while (c > 0 && (long long)cnt * c / g.nb2 > i) --c;     // sub-block c holds [cnt c / nb2, cnt (c + 1) / nb2)
        float pc2, pc3;
        ord_project(g, (int)e, pc2, pc3);
        keys[i] = ((unsigned long long)c << 61) | ((unsigned long long)ord_float_key(pc3, (b * g.nb2 + c) % 2 == 0) << ORD_ID_BITS) | e;
    }
    __syncthreads();
    bitonic_segments<ORD_THREADS, false>(keys, nullptr, P, P);
    for (int i = threadIdx.x; i < cnt; i += ORD_THREADS) g.perm[lo + i] = (int32_t)(keys[i] & ((1ull << ORD_ID_BITS) - 1ull));
}

// ---- what the kernels above left in the workspace, for simplyp_order_members (not on a run's path) ------------------------------
// One wavefront.  diag: mean[8], inv[8] as order_cov_kernel stored them; the 36 covariances, each the sum order_pca_kernel forms
// (the workgroups' partials in index order, then / E: the same additions, so the same bits); v2[8], v3[8] widened to double.
__global__ __launch_bounds__(64) void order_diag_kernel(int E, int n_groups, const double* part_cov, const double* moments,
                                                        const float* vec, double* diag)
{
    const int lane = threadIdx.x;
    if (lane < 2 * ORD_WIN) {
        diag[lane] = moments[lane];
        diag[2 * ORD_WIN + ORD_NCOV + lane] = (double)vec[lane];
    }
    if (lane < ORD_NCOV) {
        double s = 0.0;
        for (int b = 0; b < n_groups; ++b) s += part_cov[(size_t)b * ORD_NCOV + lane];
        s /= E;
        diag[2 * ORD_WIN + lane] = s;
    }
}

}  // namespace simplyp
