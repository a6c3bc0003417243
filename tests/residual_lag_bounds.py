"""How far the device's lag-one sums (simplyp_gof_lag) and AR(1) log-probabilities (simplyp_mcmc_log_prob_ar1) may lie from the
NumPy statement (simplyp_amd/residuals.py): the bounds the GPU tests use.  Derived from the operations on either side, the number
format (u = 2^-53) and the errors tests/test_gpu_elementary.py pins for the device's reciprocal (sp_rcp: faithful, < 1 ulp =
2 u relative) and logarithm (sp_log: < 1 ulp); evaluated on the statement's own values, never on the values under test.

The sums.  Both sides start from the same fp64 table.  The simulated value s of a pair:
  device   Q = Qr (A 1000 / 86400): 3 roundings; SS, TDP, PP = flux rcp(Qr A): 1 + 2 + 1 = 4 u; TP = TDP + PP (positive terms): + u;
           SRP = TDP f: + u -- at most 5 u from the true value
  host     Q = Qr A 1000 / 86400: 3 u; (flux / Qr) / A: 2 u; TP, SRP: + u -- at most 3 u
so the two s differ by at most E_SIM = 8 u relative.  x = obs / s: the device forms obs rcp(s) (2 u + u), the host one division
(u); with the difference in s the two x differ by at most (E_SIM + 4 u) |x|.  r = x - 1 is rounded once on either side:
  |dr| <= (E_SIM + 4 u) |1 + r| + 2 u |r|.
A term of A or B is a square, r^2: |d| <= 2 |r| dr; a term of C is r_t r_{t-1}: |d| <= |r_t| dr_{t-1} + |r_{t-1}| dr_t; the host
rounds the product once more (u |term|; the device's fused multiply-add does not).  The host adds with math.fsum (exact); the
device adds the n_link terms of a sum one after the other within a slice of the day list and then the slices in order -- never
more than n_link additions on the way of any term, each rounded within u of a partial sum that the sum of the absolute terms
bounds:
  bound = n_link u sum|term| + sum (per-term bound + u |term|).
The same holds for SUM_RELSQ over all n paired rows."""

import numpy as np

U = 2.0 ** -53
E_SIM = 8.0 * U


def residual_error(r):
    """|dr| of one pair from the statement's r."""
    r = np.abs(np.asarray(r, dtype=np.float64))
    return (E_SIM + 4.0 * U) * (1.0 + r) + 2.0 * U * r


def sum_bound(terms, term_errors):
    """The bound of one sum from the statement's terms [n] and their per-term bounds [n]."""
    terms = np.abs(np.asarray(terms, dtype=np.float64))
    return len(terms) * U * terms.sum() + (np.asarray(term_errors) + U * terms).sum()


def lag_bounds(r_head, r_tail):
    """(bound of A, bound of B, bound of C) from the statement's r on the linked rows and on their predecessors."""
    r_head, r_tail = np.asarray(r_head, dtype=np.float64), np.asarray(r_tail, dtype=np.float64)
    dh, dt = residual_error(r_head), residual_error(r_tail)
    return (sum_bound(r_head * r_head, 2.0 * np.abs(r_head) * dh), sum_bound(r_tail * r_tail, 2.0 * np.abs(r_tail) * dt),
            sum_bound(r_head * r_tail, np.abs(r_head) * dt + np.abs(r_tail) * dh))


def relsq_bound(r):
    """The bound of SUM_RELSQ from the statement's r on the paired rows."""
    r = np.asarray(r, dtype=np.float64)
    return sum_bound(r * r, 2.0 * np.abs(r) * residual_error(r))


def loglik_bound(n, sum_log_sim, sum_relsq, n_link, A, B, C, m, phi):
    """The bound of one pair's AR(1) term when both sides start from the SAME sums: every operation is the same IEEE operation in
    the same order on both sides but the two logarithms, each within 1 ulp of the truth on either side -- 2 ulp = 4 u of |ln| apart.
    That difference enters through n ln m and 0.5 n_link ln s; what follows it rounds differently by at most u of a partial
    result, six operations at most, each partial result no larger than the sum of the absolute terms."""
    s = (1 - phi) * (1 + phi)
    q = sum_relsq + ((phi * phi) * (A + B) - (2 * phi) * C) / s
    parts = [np.abs(0.5 * n * np.log(2 * np.pi)), np.abs(n * np.log(m)), np.abs(sum_log_sim), np.abs(q / (2 * m * m)),
             np.abs(0.5 * n_link * np.log(s))]
    return 4.0 * U * (parts[1] + parts[4]) + 6.0 * U * sum(parts)
