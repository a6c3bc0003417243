"""Lag-one sums of the relative residuals and the AR(1) heteroscedastic log-likelihood, stated once in NumPy: what
``simplyp_gof_lag`` and ``simplyp_mcmc_log_prob_ar1`` compute on the device and what their tests compare against.

The model.  For one observed variable at one output reach and one member, a row ``t`` of the daily table is *paired* when the
observation and the simulated value are both non-NaN (``simplyp_gof``'s rule), and ``r_t = obs_t / sim_t - 1``.  A paired row is
*linked* when row ``t - 1`` is paired too.  The standardised residuals ``eta_t = r_t / m`` form a stationary AR(1) along linked
rows, ``eta_t | eta_{t-1} ~ N(phi eta_{t-1}, 1 - phi^2)`` with ``|phi| < 1``; a paired row that is not linked starts a new segment
with ``eta_t ~ N(0, 1)``, and segments are independent of each other.  (An exact treatment of a gap of ``g`` days needs ``phi^g``,
which does not factorise into sums; independence across gaps is this model's rule.)  The per-day marginal of ``eta_t`` stays
``N(0, 1)`` for every ``phi``, so per-day predictive bands do not depend on it."""

import numpy as np

LN_2PI = np.log(2 * np.pi)


def lag_terms(obs, sim):
    """The link rule, row by row: ``(paired [D, ...], r [D, ...], link [D - 1, ...])`` of observations ``obs[D]`` (NaN = none)
    against simulated series ``sim[D, ...]`` (day axis first; trailing axes, e.g. members, are kept).  ``r`` is 0 where the row
    is not paired; ``link[t - 1]`` says that row ``t`` is linked, its pair of residuals being ``r[t]`` and ``r[t - 1]``."""
    obs = np.asarray(obs, dtype=np.float64)
    sim = np.asarray(sim, dtype=np.float64)
    o = obs.reshape(obs.shape + (1,) * (sim.ndim - 1))
    paired = ~np.isnan(o) & ~np.isnan(sim)
    with np.errstate(all='ignore'):
        r = np.where(paired, o / sim - 1.0, 0.0)
    return paired, r, paired[1:] & paired[:-1]


def lag_sums(obs, sim):
    """``(n_link, A, B, C)``: the number of linked rows, ``A = sum r_t^2``, ``B = sum r_{t-1}^2`` and ``C = sum r_t r_{t-1}``
    over the linked rows ``t`` (``lag_terms``).  A NaN simulated value breaks the links on both sides of it, for that member
    only."""
    _, r, link = lag_terms(obs, sim)
    head, tail = np.where(link, r[1:], 0.0), np.where(link, r[:-1], 0.0)
    return link.sum(axis=0).astype(np.float64), (head * head).sum(axis=0), (tail * tail).sum(axis=0), (head * tail).sum(axis=0)


def loglik_ar1(n, sum_log_sim, sum_relsq, n_link, A, B, C, m, phi):
    """The log-likelihood of the model above from ``simplyp_gof``'s sums (``n`` paired rows, ``sum_log_sim``, ``sum_relsq``) and the
    lag-one sums, in the device's order of operations.  At ``phi = 0`` this is ``visualise_results.loglik`` term for term.  The
    arguments broadcast."""
    s = (1 - phi) * (1 + phi)
    q = sum_relsq + ((phi * phi) * (A + B) - (2 * phi) * C) / s
    return -0.5 * n * LN_2PI - n * np.log(m) - sum_log_sim - q / (2 * m * m) - 0.5 * n_link * np.log(s)


def phi_hat(B, C):
    """The conditional maximum-likelihood lag-one coefficient ``C / B`` (NaN where there are no linked rows)."""
    with np.errstate(all='ignore'):
        return np.asarray(C, dtype=np.float64) / np.asarray(B, dtype=np.float64)
