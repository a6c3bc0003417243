// simplyp_order.h -- the members' lane-slot order for the load balancer, in plain C++ (no HIP, no context): the host rule that
// simplyp_order.hip.h restates as kernels.  simplyp_hip.hip (SIMPLYP_ORDER_HOST=1, ensembles above ORD_MAX_E, simplyp_order_members
// with where = 1) and a host program (tests/order_host_main.cpp) share it; tests/order_model.py states what a correct order is.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <functional>
#include <numeric>
#include <thread>
#include <vector>

namespace simplyp_order {

// Doubles order_members reports of its intermediate results for n_win = 8: mean[8], inv[8] (1 / deviation), the 36 covariances
// of the standardised windows (i <= j, row by row), v2[8], v3[8] (the eigenvectors of PC2 and PC3 as the projection uses them).
constexpr int DIAG_DOUBLES = 8 + 8 + 36 + 8 + 8;

// Lane-slot order for the load balancer, from the pilot's cost table cost[n_win][E] (right-hand-side evaluations of each
// member in each of n_win short windows of the forcing).  Lanes of a wavefront step in lockstep through a day, so what
// matters is that the 64 members of a wave need similar step counts *day by day*, not only in total:
//   1. rank by total cost, descending, and cut into blocks (long waves start first; LPT order for the dispatcher);
//   2. inside a block, order by the dominant cost *patterns*: the 2nd and 3rd principal components of the standardised
//      log-cost table (the 1st is the total) -- sub-blocks by PC2, PC3 inside, directions alternating so that neighbours
//      across a block border stay alike.
// Measured on the bench ensemble: SIMT efficiency 0.78 (total cost only) -> 0.82, main kernel -4 %.
// run fn(i) for i in [0, n) on up to 8 host threads (the ordering below is a few independent passes over 100 000+ members
// that sit between the pilot and the main launch, i.e. in the timed path)
template <class F>
void parallel_for(int n, F fn)
{
    const int n_thr = std::max(1, std::min({n, 8, (int)std::thread::hardware_concurrency()}));
    std::atomic<int> next(0);
    auto work = [&]() { for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) fn(i); };
    std::vector<std::thread> pool;
    try {
        for (int t = 1; t < n_thr; ++t) pool.emplace_back(work);
    } catch (...) {
        // no more threads to be had: the calling thread does whatever the started ones do not
    }
    work();
    for (std::thread& t : pool) t.join();
}

// diag (optional): mean[n], inv[n], the n (n + 1) / 2 covariances (i <= j, row by row), v2[n], v3[n] -- DIAG_DOUBLES for n = 8.
inline void order_members(const std::vector<uint32_t>& cost, int n_win, int E, std::vector<int32_t>& perm, double* diag = nullptr)
{
    const int n = n_win;
    std::vector<uint32_t> total((size_t)E, 0u);
    std::vector<float> z((size_t)n * E);
    for (int w = 0; w < n; ++w) {
        const uint32_t* c = cost.data() + (size_t)w * E;
        for (int e = 0; e < E; ++e) total[e] += c[e];
    }
    parallel_for(n, [&](int w) {          // standardised log cost of every member in window w
        const uint32_t* c = cost.data() + (size_t)w * E;
        float* zw = z.data() + (size_t)w * E;
        double mean = 0.0, sq = 0.0;
        for (int e = 0; e < E; ++e) {
            const float l = std::log2((float)c[e] + 1.0f);
            zw[e] = l;
            mean += l;
            sq += (double)l * l;
        }
        mean /= E;
        const double inv64 = 1.0 / (std::sqrt(std::max(0.0, sq / E - mean * mean)) + 1e-12);
        const float m = (float)mean, inv = (float)inv64;
        if (diag) { diag[w] = mean; diag[n + w] = inv64; }
        for (int e = 0; e < E; ++e) zw[e] = (zw[e] - m) * inv;
    });
    // covariance of the windows and its eigenvectors (cyclic Jacobi on an n x n symmetric matrix)
    std::vector<double> A((size_t)n * n, 0.0), V((size_t)n * n, 0.0);
    parallel_for(n * n, [&](int ij) {
        const int i = ij / n, j = ij % n;
        if (j < i) return;
        const float *zi = z.data() + (size_t)i * E, *zj = z.data() + (size_t)j * E;
        double acc = 0.0;
        for (int e = 0; e < E; ++e) acc += (double)(zi[e] * zj[e]);
        A[(size_t)i * n + j] = A[(size_t)j * n + i] = acc / E;
    });
    if (diag)
        for (int i = 0, k = 0; i < n; ++i) for (int j = i; j < n; ++j) diag[2 * n + k++] = A[(size_t)i * n + j];
    for (int i = 0; i < n; ++i) V[(size_t)i * n + i] = 1.0;
    for (int sweep = 0; sweep < 50; ++sweep) {
        double off = 0.0;
        for (int i = 0; i < n; ++i) for (int j = i + 1; j < n; ++j) off += A[(size_t)i * n + j] * A[(size_t)i * n + j];
        if (off < 1e-22) break;
        for (int pi = 0; pi < n; ++pi)
            for (int qi = pi + 1; qi < n; ++qi) {
                const double apq = A[(size_t)pi * n + qi];
                if (std::fabs(apq) < 1e-300) continue;
                const double theta = (A[(size_t)qi * n + qi] - A[(size_t)pi * n + pi]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
                for (int k = 0; k < n; ++k) {
                    const double akp = A[(size_t)k * n + pi], akq = A[(size_t)k * n + qi];
                    A[(size_t)k * n + pi] = c * akp - sn * akq; A[(size_t)k * n + qi] = sn * akp + c * akq;
                }
                for (int k = 0; k < n; ++k) {
                    const double apk = A[(size_t)pi * n + k], aqk = A[(size_t)qi * n + k];
                    A[(size_t)pi * n + k] = c * apk - sn * aqk; A[(size_t)qi * n + k] = sn * apk + c * aqk;
                }
                for (int k = 0; k < n; ++k) {
                    const double vkp = V[(size_t)k * n + pi], vkq = V[(size_t)k * n + qi];
                    V[(size_t)k * n + pi] = c * vkp - sn * vkq; V[(size_t)k * n + qi] = sn * vkp + c * vkq;
                }
            }
    }
    std::vector<int> ev(n);
    std::iota(ev.begin(), ev.end(), 0);
    std::stable_sort(ev.begin(), ev.end(), [&](int x, int y) { return A[(size_t)x * n + x] > A[(size_t)y * n + y]; });
    if (diag)
        for (int w = 0; w < n; ++w) {
            diag[2 * n + n * (n + 1) / 2 + w] = n > 1 ? (float)V[(size_t)w * n + ev[1]] : 0.0f;
            diag[3 * n + n * (n + 1) / 2 + w] = n > 2 ? (float)V[(size_t)w * n + ev[2]] : 0.0f;
        }
    std::vector<float> pc2((size_t)E, 0.0f), pc3((size_t)E, 0.0f);
    const int slabs = 8;
    parallel_for(slabs, [&](int sl) {
        const int e0 = (int)((long long)E * sl / slabs), e1 = (int)((long long)E * (sl + 1) / slabs);
        for (int w = 0; w < n; ++w) {
            const float v2 = n > 1 ? (float)V[(size_t)w * n + ev[1]] : 0.0f, v3 = n > 2 ? (float)V[(size_t)w * n + ev[2]] : 0.0f;
            const float* zw = z.data() + (size_t)w * E;
            for (int e = e0; e < e1; ++e) { pc2[e] += v2 * zw[e]; pc3[e] += v3 * zw[e]; }
        }
    });
    // Packed (key << 32 | member) words: ties fall back to the member id, so the order is fully determined.
    auto fkey = [](float f, bool ascending) -> uint64_t {      // order-preserving map float -> uint32
        if (!ascending) f = -f;
        uint32_t u; memcpy(&u, &f, sizeof(u));
        u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;
        return (uint64_t)u << 32;
    };
    std::vector<uint64_t> key((size_t)E);
    for (int e = 0; e < E; ++e) key[e] = ((uint64_t)(0xFFFFFFFFu - total[e]) << 32) | (uint32_t)e;     // total cost, descending
    // blocks of >= 256 members by total cost (at most 24), sub-blocks of >= 256 by PC2 (at most 6), PC3 inside.  Only the
    // leaves need a full sort: the block borders come from nth_element.
    const int nb1 = std::max(1, std::min(24, E / 256));
    const int nb2 = std::max(1, std::min(6, E / (nb1 * 256)));
    std::function<void(size_t, size_t, int, int)> split = [&](size_t lo, size_t hi, int b0, int b1) {      // blocks [b0, b1) live in [lo, hi)
        if (b1 - b0 <= 1) return;
        const int bm = (b0 + b1) / 2;
        const size_t mid = (size_t)E * bm / nb1;
        std::nth_element(key.begin() + lo, key.begin() + mid, key.begin() + hi);
        split(lo, mid, b0, bm);
        split(mid, hi, bm, b1);
    };
    split(0, (size_t)E, 0, nb1);
    parallel_for(nb1, [&](int b) {
        const size_t lo = (size_t)E * b / nb1, hi = (size_t)E * (b + 1) / nb1;
        for (size_t i = lo; i < hi; ++i) { const uint32_t e = (uint32_t)key[i]; key[i] = fkey(pc2[e], b % 2 == 0) | e; }
        std::sort(key.begin() + lo, key.begin() + hi);
        for (int c = 0; c < nb2; ++c) {
            const size_t l2 = lo + (hi - lo) * c / nb2, h2 = lo + (hi - lo) * (c + 1) / nb2;
            for (size_t i = l2; i < h2; ++i) { const uint32_t e = (uint32_t)key[i]; key[i] = fkey(pc3[e], (b * nb2 + c) % 2 == 0) | e; }
            std::sort(key.begin() + l2, key.begin() + h2);
        }
    });
    perm.resize((size_t)E);
    for (int e = 0; e < E; ++e) perm[e] = (int32_t)(uint32_t)key[e];
}

}  // namespace simplyp_order
