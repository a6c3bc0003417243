/*
 * simplyp_residuals.h -- an extension of the C ABI of include/simplyp.h (same library, same conventions, SIMPLYP_ABI_VERSION 18
 * still): the lag-one sums of the relative residuals and the AR(1) log-probability built on them.  Two more entry points that
 * reuse simplyp_gof_info and simplyp_mcmc_info; no struct, enum or entry point of simplyp.h changes, and a caller that does not
 * include this header sees the ABI it saw before.  The entries are kept in a header of their own because simplyp.h's list of
 * entry points is pinned, by number and by name, in the project's tests of the core ABI.
 *
 * What every analysis entry of simplyp.h has in common holds here too: a NULL context is SIMPLYP_ERR_ARG; while a run is pending
 * on the context the entry refuses and launches nothing; a call refused for its arguments launches nothing and leaves `info` as it
 * was; a call that succeeds has written every field of `info`.
 */
#ifndef SIMPLYP_RESIDUALS_H
#define SIMPLYP_RESIDUALS_H

#include "simplyp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- lag-one sums of the relative residuals: the autocorrelation check the reference's calibration notebook ends with
 * (Development/2016/MCMC.ipynb cell 21) for every member, and what an AR(1) error model needs ------------------------------ */
enum {  /* rows of `lag`.  r_t = obs_t / sim_t - 1, the quantity SIMPLYP_GOFSTAT_SUM_RELSQ squares.  A row t of the daily table
           is paired as in simplyp_gof (observation and simulated value both non-NaN) and LINKED when row t - 1 is paired too,
           for this member and this variable; the sums run over the linked rows t */
    SIMPLYP_LAGSTAT_N_LINK = 0,   /* number of linked rows                                                       */
    SIMPLYP_LAGSTAT_SQ_HEAD,      /* A = sum r_t^2                                                               */
    SIMPLYP_LAGSTAT_SQ_TAIL,      /* B = sum r_{t-1}^2                                                           */
    SIMPLYP_LAGSTAT_CROSS,        /* C = sum r_t r_{t-1}                                                         */
    SIMPLYP_N_LAG_STATS
};

/*
 * simplyp_gof_lag -- the lag-one sums of every member, from the daily table a previous simplyp_run left on the device.
 * Arguments, pairing rule and the rule for variables with 10 or fewer observations (NaN rows) are simplyp_gof's, and r_t has
 * the bits of the r_t that simplyp_gof squares.  A NaN simulated value breaks the links on both sides of it, for that member
 * only.  A paired row that is not linked starts a new segment; the error model these sums serve takes segments as independent
 * of each other: the exact treatment of a gap of g days needs phi^g, which no fixed set of sums carries.  C / B is the
 * conditional maximum-likelihood lag-one coefficient.
 *   lag             device  [SIMPLYP_N_LAG_STATS][SIMPLYP_N_GOF_VARS][n_out_reaches][E], member order
 *   info            host    may be NULL; kernel_ms = all three kernels; bytes_read = simplyp_gof's count plus the rows a slice of a
 *                           day list re-reads where its first day continues a segment (8 or 32 bytes per member and such slice);
 *                           the day and slice counts as simplyp_gof reports them
 * Synchronous.
 */
int simplyp_gof_lag(simplyp_ctx* ctx, const simplyp_dims* dims, uint32_t out_mask,
                    const int32_t* out_reaches, int32_t n_out_reaches,
                    const double* out, const int32_t* member_of_slot,
                    const double* f_tdp, const double* reach_params,
                    const double* obs, double* lag, simplyp_gof_info* info);

/*
 * simplyp_mcmc_log_prob_ar1 -- simplyp_mcmc_log_prob with an AR(1) heteroscedastic error model: the standardised residuals
 * eta_t = r_t / m_v follow eta_t | eta_{t-1} ~ N(phi_v eta_{t-1}, 1 - phi_v^2) along linked rows, a paired row that is not linked
 * starts a new segment with eta_t ~ N(0, 1), and segments are independent.  Per pair, in this order of operations, with n_link,
 * A, B, C the rows of `lag`:
 *     s = (1 - phi)(1 + phi);   q = SUM_RELSQ + ((phi phi)(A + B) - (2 phi) C) / s
 *     -0.5 n ln(2 pi) - n ln(m_v) - SUM_LOG_SIM - q / (2 m_v m_v) - 0.5 n_link ln(s)
 * At phi = 0 every pair's term has the bits of simplyp_mcmc_log_prob's.  -inf under every condition named there, and where a
 * phi is NaN or |phi| >= 1.  Arguments as for simplyp_mcmc_log_prob;
 *   lag             device  [SIMPLYP_N_LAG_STATS][SIMPLYP_N_GOF_VARS][n_out_reaches][h], as simplyp_gof_lag leaves it
 *   phi_dim         HOST    [SIMPLYP_N_GOF_VARS] the row of prop that holds the variable's phi, or -1: phi_const[v]
 *   phi_const       HOST    [SIMPLYP_N_GOF_VARS]; 0 = independent errors.  Refused when NaN or |phi| >= 1 for a variable of
 *                           pair_var whose phi_dim is -1
 */
int simplyp_mcmc_log_prob_ar1(simplyp_ctx* ctx, int32_t W, int32_t n_dim, int32_t n_out_reaches, const double* gof,
                              const double* lag, const int32_t* status, const int32_t* inside,
                              const int32_t* pair_var /* host */, const int32_t* pair_reach /* host */, int32_t n_pairs,
                              const int32_t* m_dim /* host */, const double* m_const /* host */,
                              const int32_t* phi_dim /* host */, const double* phi_const /* host */,
                              const double* prop, double* lp_prop, simplyp_mcmc_info* info);

#ifdef __cplusplus
}
#endif
#endif /* SIMPLYP_RESIDUALS_H */
