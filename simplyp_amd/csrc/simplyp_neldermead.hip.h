// simplyp_neldermead.hip.h -- multi-start Nelder-Mead on the device (gfx950): what the reference's calibration notebooks do with
// scipy.optimize.fmin(neg_log_posterior, init_guess) (Development/2016/MAP.ipynb, find_map), for S simplexes at once.
//
// Every simplex owns four members of each ensemble run, member index slot S + s, and a phase:
//   STEP   the slots hold xr, xe, xc, xcc: an iteration's four candidates are functions of the simplex alone, so they are all
//          evaluated in one run and scipy's decision tree is walked afterwards -- the lazy algorithm's path
//   EVAL   the slots hold up to four vertices that have no value yet, from `cursor` on: the initial N + 1, or the N shrunk ones
//   DONE   converged, at the iteration limit, or started where f is not finite
// One run is two kernels around the model:
//   simplyp_nm_propose_kernel   the slots' points, the box test lo <= x < hi, the run points scattered into the run's arrays
//   (simplyp_run, simplyp_gof, simplyp_mcmc_log_prob: ln p of the 4 S run points; or the caller's own target)
//   simplyp_nm_update_kernel    f = -ln p; the decision or the stored values, the shrink, the sort, the count, the termination test
// The run point of a slot that is idle or outside the box is the simplex's first vertex: the model never sees a point outside.
//
// The vertices are kept sorted in place: a step inserts its one new vertex (stable: behind every vertex that is not worse), an
// evaluation ends with a stable rank count through a workspace in global memory.  Everything is + - * / and comparisons in fp64
// (the library is built with -ffp-contract=off) in the order simplyp_amd/neldermead.py states, so the two agree bit for bit.
//
// Layout: lane = simplex; sim [N + 1][n_dim][S], fsim [N + 1][S], istate [SIMPLYP_NM_N_ISTATE][S], prop [n_dim][4 S] and the run's
// arrays are SoA in S, so every load and store of a wave is one contiguous segment.  No LDS, no barrier, no per-lane arrays: the
// loops over dimensions and vertices load what they need.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/simplyp.h"
#include "simplyp_mcmc.hip.h"              // MCMC_MAX_DIM, MCMC_TARGET_*, mcmc_count

namespace simplyp {

constexpr int NM_THREADS = 256;
constexpr int NM_SLOTS = 4;

struct NmProposeArgs {
    int S, n_dim;
    double lo[MCMC_MAX_DIM], hi[MCMC_MAX_DIM];
    int target[MCMC_MAX_DIM];
    const double* sim;                     // [N + 1][n_dim][S]
    const int32_t* istate;                 // [SIMPLYP_NM_N_ISTATE][S]
    double* prop;                          // [n_dim][4 S]
    int32_t* inside;                       // [4 S]
    double* member_params;                 // [NP_M][4 S]
    double* f_tdp;                         // [4 S]
    unsigned* counters;                    // [8]: active, converged, shrinking, non-finite start, inside
};

struct NmUpdateArgs {
    int S, n_dim, max_iter, history_rows;
    double xatol, fatol;
    const double* prop;                    // [n_dim][4 S]
    const int32_t* inside;                 // [4 S]
    const double* lp_prop;                 // [4 S]
    double* sim;                           // [N + 1][n_dim][S]
    double* fsim;                          // [N + 1][S]
    int32_t* istate;                       // [SIMPLYP_NM_N_ISTATE][S]
    double* history;                       // [history_rows][S] or nullptr
    double* work;                          // [(N + 1) (n_dim + 1)][S]: the sort's other copy
    unsigned* counters;
};

// What both kernels report of the state they leave.
__device__ __forceinline__ void nm_count_state(unsigned* counters, int phase, int n_iter, int status)
{
    mcmc_count(counters + 0, phase != SIMPLYP_NM_DONE);
    mcmc_count(counters + 1, phase == SIMPLYP_NM_DONE && status == SIMPLYP_NM_CONVERGED);
    mcmc_count(counters + 2, phase == SIMPLYP_NM_EVAL && n_iter >= 1);
    mcmc_count(counters + 3, status == SIMPLYP_NM_NONFINITE_START);
}

__global__ __launch_bounds__(NM_THREADS) void simplyp_nm_propose_kernel(const NmProposeArgs g)
{
    const int s = blockIdx.x * NM_THREADS + threadIdx.x;
    if (s >= g.S) return;
    const size_t S = (size_t)g.S, E = (size_t)NM_SLOTS * S;
    const int n = g.n_dim, N = g.n_dim;
    const int phase = g.istate[(size_t)SIMPLYP_NM_PHASE * S + s];
    const int cursor = g.istate[(size_t)SIMPLYP_NM_CURSOR * S + s];
    const bool step = phase == SIMPLYP_NM_STEP, eval = phase == SIMPLYP_NM_EVAL;
    // slot k wants a value: every candidate of a step, vertex cursor + k of an evaluation while there is one
    const bool u0 = step || (eval && cursor + 0 <= N), u1 = step || (eval && cursor + 1 <= N);
    const bool u2 = step || (eval && cursor + 2 <= N), u3 = step || (eval && cursor + 3 <= N);
    bool in0 = u0, in1 = u1, in2 = u2, in3 = u3;
    for (int d = 0; d < n; ++d) {
        const double x0 = g.sim[(size_t)d * S + s];
        double p0 = x0, p1 = x0, p2 = x0, p3 = x0;                      // an idle slot holds the first vertex
        if (step) {
            double acc = x0;
            for (int j = 1; j < N; ++j) acc = acc + g.sim[((size_t)j * n + d) * S + s];
            const double xbar = acc / (double)N;
            const double w = g.sim[((size_t)N * n + d) * S + s];
            p0 = 2.0 * xbar - w;                                        // rho = 1
            p1 = 3.0 * xbar - 2.0 * w;                                  // chi = 2
            p2 = 1.5 * xbar - 0.5 * w;                                  // psi = 0.5, outside
            p3 = 0.5 * xbar + 0.5 * w;                                  // inside
        } else if (eval) {
            if (u0) p0 = g.sim[((size_t)(cursor + 0) * n + d) * S + s];
            if (u1) p1 = g.sim[((size_t)(cursor + 1) * n + d) * S + s];
            if (u2) p2 = g.sim[((size_t)(cursor + 2) * n + d) * S + s];
            if (u3) p3 = g.sim[((size_t)(cursor + 3) * n + d) * S + s];
        }
        const double lo = g.lo[d], hi = g.hi[d];
        in0 = in0 && (p0 >= lo) && (p0 < hi);                           // NaN fails both
        in1 = in1 && (p1 >= lo) && (p1 < hi);
        in2 = in2 && (p2 >= lo) && (p2 < hi);
        in3 = in3 && (p3 >= lo) && (p3 < hi);
        double* row = g.prop + (size_t)d * E + s;
        row[0] = p0; row[S] = p1; row[2 * S] = p2; row[3 * S] = p3;
    }
    g.inside[s] = in0 ? 1 : 0; g.inside[S + s] = in1 ? 1 : 0; g.inside[2 * S + s] = in2 ? 1 : 0; g.inside[3 * S + s] = in3 ? 1 : 0;
    for (int d = 0; d < n; ++d) {                                       // the run point: the slot's point inside the box, else the first vertex
        const int tg = g.target[d];
        if (tg == MCMC_TARGET_NONE) continue;
        const double x0 = g.sim[(size_t)d * S + s];
        const double* row = g.prop + (size_t)d * E + s;
        double* dst = (tg == MCMC_TARGET_F_TDP ? g.f_tdp : g.member_params + (size_t)tg * E) + s;
        dst[0] = in0 ? row[0] : x0;
        dst[S] = in1 ? row[S] : x0;
        dst[2 * S] = in2 ? row[2 * S] : x0;
        dst[3 * S] = in3 ? row[3 * S] : x0;
    }
    nm_count_state(g.counters, phase, g.istate[(size_t)SIMPLYP_NM_N_ITER * S + s], g.istate[(size_t)SIMPLYP_NM_STATUS * S + s]);
    const unsigned n_in = (unsigned)in0 + (unsigned)in1 + (unsigned)in2 + (unsigned)in3;
    if (n_in) atomicAdd(g.counters + 4, n_in);
}

__global__ __launch_bounds__(NM_THREADS) void simplyp_nm_update_kernel(const NmUpdateArgs g)
{
    const int s = blockIdx.x * NM_THREADS + threadIdx.x;
    if (s >= g.S) return;
    const size_t S = (size_t)g.S, E = (size_t)NM_SLOTS * S;
    const int n = g.n_dim, N = g.n_dim;
    int32_t* ist = g.istate + s;
    int phase = ist[(size_t)SIMPLYP_NM_PHASE * S];
    int n_iter = ist[(size_t)SIMPLYP_NM_N_ITER * S];
    int status = ist[(size_t)SIMPLYP_NM_STATUS * S];
    double* sim = g.sim + s;                                            // vertex j, dimension d: sim[((size_t)j * n + d) * S]
    double* fsim = g.fsim + s;                                          // vertex j: fsim[(size_t)j * S]
    if (phase != SIMPLYP_NM_DONE) {
        const double inf = __builtin_huge_val();
        double f0v, f1v, f2v, f3v;                                      // f = -ln p; +inf where the slot is not inside or ln p is NaN
        { const double lp = g.lp_prop[s];         f0v = (g.inside[s] != 0 && lp == lp) ? -lp : inf; }
        { const double lp = g.lp_prop[S + s];     f1v = (g.inside[S + s] != 0 && lp == lp) ? -lp : inf; }
        { const double lp = g.lp_prop[2 * S + s]; f2v = (g.inside[2 * S + s] != 0 && lp == lp) ? -lp : inf; }
        { const double lp = g.lp_prop[3 * S + s]; f3v = (g.inside[3 * S + s] != 0 && lp == lp) ? -lp : inf; }
        bool fin = false, complete = false;
        if (phase == SIMPLYP_NM_STEP) {
            const double fr = f0v, fe = f1v, fc = f2v, fcc = f3v;
            const double fb = fsim[0], fn1 = fsim[(size_t)(N - 1) * S], fw = fsim[(size_t)N * S];
            int sel = -1, move = SIMPLYP_NM_N_SHRINK;                   // scipy's _minimize_neldermead, its < and <= as they are
            if (fr < fb) {
                if (fe < fr) { sel = 1; move = SIMPLYP_NM_N_EXPAND; }
                else { sel = 0; move = SIMPLYP_NM_N_REFLECT; }
            } else if (fr < fn1) {
                sel = 0; move = SIMPLYP_NM_N_REFLECT;
            } else if (fr < fw) {
                if (fc <= fr) { sel = 2; move = SIMPLYP_NM_N_CONTRACT_OUT; }
            } else {
                if (fcc < fw) { sel = 3; move = SIMPLYP_NM_N_CONTRACT_IN; }
            }
            ist[(size_t)move * S] += 1;
            if (sel >= 0) {
                const double f_new = sel == 0 ? fr : (sel == 1 ? fe : (sel == 2 ? fc : fcc));
                int p = 0;                                              // behind every vertex that is not worse: the stable place
                for (int j = 0; j < N; ++j) p += (fsim[(size_t)j * S] <= f_new) ? 1 : 0;
                for (int r = N; r > p; --r) {                           // the worst vertex drops out
                    fsim[(size_t)r * S] = fsim[(size_t)(r - 1) * S];
                    for (int d = 0; d < n; ++d) sim[((size_t)r * n + d) * S] = sim[((size_t)(r - 1) * n + d) * S];
                }
                fsim[(size_t)p * S] = f_new;
                for (int d = 0; d < n; ++d) sim[((size_t)p * n + d) * S] = g.prop[(size_t)d * E + (size_t)sel * S + s];
                fin = true;
            } else {                                                    // shrink towards the best vertex, then re-evaluate
                for (int d = 0; d < n; ++d) {
                    const double x0 = sim[(size_t)d * S];
                    for (int j = 1; j <= N; ++j) {
                        const double x = sim[((size_t)j * n + d) * S];
                        sim[((size_t)j * n + d) * S] = x0 + 0.5 * (x - x0);
                    }
                }
                phase = SIMPLYP_NM_EVAL;
                ist[(size_t)SIMPLYP_NM_CURSOR * S] = 1;
            }
        } else {                                                        // EVAL: the values of vertices cursor .. cursor + 3
            const int cursor = ist[(size_t)SIMPLYP_NM_CURSOR * S];
            if (cursor + 0 <= N) fsim[(size_t)(cursor + 0) * S] = f0v;
            if (cursor + 1 <= N) fsim[(size_t)(cursor + 1) * S] = f1v;
            if (cursor + 2 <= N) fsim[(size_t)(cursor + 2) * S] = f2v;
            if (cursor + 3 <= N) fsim[(size_t)(cursor + 3) * S] = f3v;
            if (cursor + NM_SLOTS > N) {                                // all in: a stable rank count, through the workspace
                double* wx = g.work + s;
                double* wf = g.work + (size_t)(N + 1) * n * S + s;
                for (int j = 0; j <= N; ++j) {
                    const double fj = fsim[(size_t)j * S];
                    int rank = 0;
                    for (int i = 0; i <= N; ++i) {
                        const double fi = fsim[(size_t)i * S];
                        rank += (fi < fj || (fi == fj && i < j)) ? 1 : 0;
                    }
                    wf[(size_t)rank * S] = fj;
                    for (int d = 0; d < n; ++d) wx[((size_t)rank * n + d) * S] = sim[((size_t)j * n + d) * S];
                }
                for (int j = 0; j <= N; ++j) {
                    fsim[(size_t)j * S] = wf[(size_t)j * S];
                    for (int d = 0; d < n; ++d) sim[((size_t)j * n + d) * S] = wx[((size_t)j * n + d) * S];
                }
                phase = SIMPLYP_NM_STEP;
                ist[(size_t)SIMPLYP_NM_CURSOR * S] = 0;
                fin = complete = true;
            } else {
                ist[(size_t)SIMPLYP_NM_CURSOR * S] = cursor + NM_SLOTS;
            }
        }
        if (fin) {                                                      // an iteration is complete
            n_iter += 1;
            const double fb = fsim[0];
            if (g.history && n_iter - 1 < g.history_rows) g.history[(size_t)(n_iter - 1) * S + s] = fb;
            bool finite = true, conv = true;
            for (int j = 0; j <= N; ++j) {
                const double fj = fsim[(size_t)j * S];
                finite = finite && (__builtin_fabs(fj) < inf);
                if (j >= 1) {
                    conv = conv && (__builtin_fabs(fb - fj) <= g.fatol);   // max |.| <= tol: every one is, and none is NaN
                    for (int d = 0; d < n; ++d)
                        conv = conv && (__builtin_fabs(sim[((size_t)j * n + d) * S] - sim[(size_t)d * S]) <= g.xatol);
                }
            }
            if (complete && n_iter == 1 && !finite) { phase = SIMPLYP_NM_DONE; status = SIMPLYP_NM_NONFINITE_START; }
            else if (n_iter >= g.max_iter) { phase = SIMPLYP_NM_DONE; status = SIMPLYP_NM_MAXITER; }
            else if (conv) { phase = SIMPLYP_NM_DONE; status = SIMPLYP_NM_CONVERGED; }
        }
        ist[(size_t)SIMPLYP_NM_PHASE * S] = phase;
        ist[(size_t)SIMPLYP_NM_N_ITER * S] = n_iter;
        ist[(size_t)SIMPLYP_NM_STATUS * S] = status;
    }
    nm_count_state(g.counters, phase, n_iter, status);
}

}  // namespace simplyp
