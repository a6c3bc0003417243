/*
 * simplyp_nsga2.h -- an extension of the C ABI of include/simplyp.h (same library, same conventions, SIMPLYP_ABI_VERSION 18
 * still): NSGA-II's own pieces for a multi-objective search over an ensemble's fit criteria (Deb, Pratap, Agarwal & Meyarivan
 * 2002) -- the initial population, crowding distance, environmental selection, mating with variation.  The model run,
 * simplyp_gof and simplyp_pareto are the other steps of a generation.  Four more entry points that reuse simplyp_pareto_info and
 * simplyp_mcmc_info; no struct, enum or entry point of simplyp.h changes, and a caller that does not include this header sees the
 * ABI it saw before.  The entries are kept in a header of their own because simplyp.h's list of entry points is pinned, by
 * number and by name, in the project's tests of the core ABI.
 *
 * What every analysis entry of simplyp.h has in common holds here too: a NULL context is SIMPLYP_ERR_ARG; while a run is pending
 * on the context the entry refuses and launches nothing; a call refused for its arguments launches nothing and leaves `info` as it
 * was; a call that succeeds has written every field of `info`.  All four are synchronous on the context's stream.
 *
 * The rule (simplyp_amd/nsga2.py is its definition, in NumPy).  A population has N members, N even, 4 <= N <= 65536, with
 * positions theta [n_dim][N], 1 <= n_dim <= 16, inside the closed box lo <= x <= hi, and objectives obj [M][N], 1 <= M <= 8,
 * under sense[m] = +1 (larger is better) or -1 as in simplyp_pareto: y = sense x.  A member with a negative rank (what
 * simplyp_pareto gives a member its include mask leaves out) is invalid: worse than any rank, crowding 0.  The draws are
 * Philox4x32-10 under key (seed & 0xffffffff, seed >> 32) with counter (pair or member, generation t, code << 8 | dimension,
 * 0x4E534732): a pure function of their arguments, whatever the launch shape.
 */
#ifndef SIMPLYP_NSGA2_H
#define SIMPLYP_NSGA2_H

#include "simplyp.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * simplyp_nsga2_init -- the initial population: theta[d][i] = clip(lo[d] + (hi[d] - lo[d]) u), u the uniform of counter
 * (i, 0, 5 << 8 | d, 0x4E534732), and its scatter into the arrays of the run that evaluates it.
 *   lo, hi          HOST    [n_dim], lo < hi; a NaN bound is refused
 *   target          HOST    [n_dim] as for simplyp_mcmc_propose: a row of member_params, -1 = f_tdp, -2 = nowhere; no row twice
 *   theta           device  [n_dim][N], written
 *   member_params   device  [SIMPLYP_NP_M][N] or NULL when no target names a row; only the named rows are written
 *   f_tdp           device  [N] or NULL when no target is -1
 *   info            host    may be NULL; n_inside = N, n_accepted = 0, n_nan = 0
 */
int simplyp_nsga2_init(simplyp_ctx* ctx, int32_t N, int32_t n_dim, uint64_t seed, const double* lo, const double* hi,
                       const int32_t* target, double* theta, double* member_params, double* f_tdp, simplyp_mcmc_info* info);

/*
 * simplyp_nsga2_crowding -- the crowding distance of every member of a set of n, 1 <= n <= 131072, within its front.  For each
 * objective the front's members are ordered by (y, index), -0.0 and +0.0 being equal; a member that is first or last in the
 * order of any objective gets +inf, any other ((0 + term_0) + term_1) + ... with term_m = (y_next - y_prev) / (y_max - y_min)
 * of its neighbours and its front where y_max > y_min, and 0 otherwise.  A member with rank < 0 gets 0.  Neighbours and
 * extremes are selected, never summed: the bits do not depend on how the work is split.
 *   obj             device  [M][n]; no NaN where rank >= 0
 *   sense           HOST    [M], +1 or -1
 *   rank            device  [n] int32, as simplyp_pareto leaves it
 *   crowd           device  [n], written
 *   info            host    may be NULL; pair_tests = n n, n_used = the members with rank >= 0, the front counts 0
 */
int simplyp_nsga2_crowding(simplyp_ctx* ctx, int32_t n, int32_t M, const double* obj, const int32_t* sense, const int32_t* rank,
                           double* crowd, simplyp_pareto_info* info);

/*
 * simplyp_nsga2_select -- environmental selection: the n members, N <= n <= 2 N, ordered by (rank ascending with rank < 0 last,
 * crowding descending, index ascending); position[i] = the members before i; the survivors are positions 0 .. N - 1, stored at
 * their position, so what comes out is sorted best first.
 *   rank, crowd     device  [n]
 *   position        device  [n] int32, written
 *   survivor        device  [N] int32, written: the member at each position
 *   n_rows          0 .. 64 rows of doubles to gather along (positions, objectives)
 *   rows_in         device  [n_rows][n], or NULL when n_rows = 0
 *   rows_out        device  [n_rows][N]: rows_out[r][q] = rows_in[r][survivor[q]]; must not overlap rows_in
 *   rank_out        device  [N] int32 or NULL: rank[survivor[q]] -- the rank in the combined set (Deb's convention)
 *   crowd_out       device  [N] or NULL: crowd[survivor[q]]
 *   info            host    may be NULL; pair_tests = n n, n_used = N, the front counts 0
 */
int simplyp_nsga2_select(simplyp_ctx* ctx, int32_t n, int32_t N, const int32_t* rank, const double* crowd, int32_t* position,
                         int32_t* survivor, int32_t n_rows, const double* rows_in, double* rows_out, int32_t* rank_out,
                         double* crowd_out, simplyp_pareto_info* info);

/*
 * simplyp_nsga2_offspring -- the N children of generation t: child pair p < N / 2 draws two binary tournaments (lower rank, then
 * larger crowding, then lower index wins), crosses its parents with probability p_cross by bounded SBX (a dimension takes part
 * with probability 1/2 and only where the parents differ) and mutates every dimension of either child with probability p_mut by
 * bounded polynomial mutation, with distribution indices eta_c = 2^k_c - 1 and eta_m = 2^k_m - 1: every power is k squarings,
 * every root k nested square roots (simplyp_amd/csrc/simplyp_nsga2.h).  The children are columns p and N / 2 + p, clipped into the box.
 *   k_c, k_m        1 .. 5
 *   p_cross, p_mut  in [0, 1]
 *   lo, hi, target  HOST    as for simplyp_nsga2_init
 *   theta           device  [n_dim][N] the parents' positions
 *   rank, crowd     device  [N] the parents' rank and crowding
 *   child           device  [n_dim][N], written; must not overlap theta
 *   parents         device  [2][N] int32 or NULL: the two parents of every child column
 *   member_params, f_tdp    as for simplyp_nsga2_init: the children scattered into the run's arrays
 *   info            host    may be NULL; n_inside = N, n_accepted = the pairs that crossed, n_nan = 0
 */
int simplyp_nsga2_offspring(simplyp_ctx* ctx, int32_t N, int32_t n_dim, uint64_t seed, uint32_t t, int32_t k_c, int32_t k_m,
                            double p_cross, double p_mut, const double* lo, const double* hi, const int32_t* target,
                            const double* theta, const int32_t* rank, const double* crowd, double* child, int32_t* parents,
                            double* member_params, double* f_tdp, simplyp_mcmc_info* info);

#ifdef __cplusplus
}
#endif
#endif /* SIMPLYP_NSGA2_H */
