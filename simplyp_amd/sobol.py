"""NumPy statement of the Sobol' sensitivity estimator the device computes (csrc/simplyp_sobol.hip.h).  CPU only.

Variance-based global sensitivity analysis of an ensemble: Saltelli's design of ``N (d + 2)`` model runs, the first-order and
total-order indices of Saltelli et al. 2010 with the Sobol'-Levitan centring -- what ``scipy.stats.sobol_indices`` computes --
and their bootstrap as resampling counts times per-sample terms.

* design: ``N`` base samples, ``d`` dimensions with a box ``lo < hi``.  Unit points ``u[m][k][n]``, ``m`` in {0: A, 1: B}, are
  ``uniform(x0, x1)`` of Philox4x32-10 (``predictive.philox4x32_10``) under key ``(seed & 0xffffffff, seed >> 32)`` at counter
  ``(n, k, m, DESIGN_STREAM)``, or the caller's ``[2][d][N]`` array in [0, 1).  ``x = lo + (hi - lo) * u``.
* ensemble: ``E = N (d + 2)`` members, block-major: member ``j N + n`` is ``A_n`` for ``j = 0``, ``B_n`` for ``j = 1`` and
  ``A_n`` with dimension ``i`` taken from ``B_n`` for ``j = 2 + i``.
* a row ``f[E]`` of any table whose fastest axis is the member axis; sample ``n`` is valid iff none of its ``d + 2`` members
  carries ``abi.STATUS_NONFINITE``.  With ``a, b, ab_i`` the row at ``A, B, AB_i`` minus ``mu = sum_valid (a + b) / (2 n_valid)``
  (every ``a + b`` one fp64 addition, their sum exactly rounded: ``math.fsum`` here, double-double on the device):
  ``p = a + b``, ``s = a a + b b``, ``g_i = b (ab_i - a)``, ``t_i = (a - ab_i) (a - ab_i)``.  Invalid samples take part in nothing
  (the device selects their terms to 0; here they are compacted away, which is the same sums).
* for a weight vector ``c[N]``: ``n_c = sum c v``, ``P = sum c p``, ``S = sum c s``, ``G_i = sum c g_i``, ``T_i = sum c t_i``;
  ``m1 = P / (2 n_c)``, ``m2 = S / (2 n_c)``, ``var = m2 - m1 m1``, ``S1_i = (G_i / n_c) / var``, ``ST_i = (0.5 (T_i / n_c)) / var``.
* resample 0 is ``c = 1``, the point estimate; resample ``b >= 1`` has ``c[n]`` = the number of ``j < N`` with ``idx(b, j) == n``,
  ``idx(b, j) = (x_{j & 3} N) >> 32`` of Philox counter ``(b, j >> 2, 0, BOOT_STREAM)``.

``var == 0`` (a constant row) gives what IEEE gives, NaN; ``scipy.stats.sobol_indices`` maps that case to 0.

The design and the counts match the device bit for bit; so do the indices as a function of the sums.  The sums themselves are
added in another order on the device and agree within the summation bound ``N 2^-53 sum |c term|``.
"""

import math

import numpy as np

from . import abi
from .predictive import philox4x32_10, _uniform

DESIGN_STREAM = 0x53454E53       # "SENS": the counter's fourth word of the design's unit points
BOOT_STREAM = 0x424F4F54         # "BOOT": ... of the bootstrap's indices
MAX_DIM = 16
MIN_BASE, MAX_BASE = 2, 32768


def _key(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32


def check_shape(N, n_dim):
    if not MIN_BASE <= int(N) <= MAX_BASE:
        raise ValueError("n_base must be in [%d, %d] (got %d)" % (MIN_BASE, MAX_BASE, N))
    if not 1 <= int(n_dim) <= MAX_DIM:
        raise ValueError("the number of dimensions must be in [1, %d] (got %d)" % (MAX_DIM, n_dim))


def unit_points(seed, N, n_dim):
    """The design's own unit points ``u[2, n_dim, N]`` in (0, 1)."""
    n = np.arange(N)[None, None, :]
    k = np.arange(n_dim)[None, :, None]
    m = np.arange(2)[:, None, None]
    x0, x1, _, _ = philox4x32_10((n, k, m, DESIGN_STREAM), _key(seed))
    return _uniform(x0, x1)


def check_unit(unit, N, n_dim):
    unit = np.ascontiguousarray(unit, dtype=np.float64)
    if unit.shape != (2, n_dim, N):
        raise ValueError("unit_samples must have shape [2, n_dim, n_base] = %s, got %s" % ((2, n_dim, N), unit.shape))
    if not ((unit >= 0.0) & (unit < 1.0)).all():
        raise ValueError("unit_samples must lie in [0, 1)")
    return unit


def design(N, lo, hi, seed=0, unit=None):
    """``x[n_dim, E]``, ``E = N (n_dim + 2)``, block-major A, B, AB_0 .. AB_{d-1}."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    d = len(lo)
    check_shape(N, d)
    u = unit_points(seed, N, d) if unit is None else check_unit(unit, N, d)
    x = np.empty((d, d + 2, N))
    x[:, 0] = u[0]
    x[:, 1] = u[1]
    for i in range(d):
        x[:, 2 + i] = u[0]
        x[i, 2 + i] = u[1, i]
    return lo[:, None] + (hi - lo)[:, None] * x.reshape(d, (d + 2) * N)


def valid_samples(status, N, n_dim):
    """``v[N]``: no member of the sample carries STATUS_NONFINITE (``status`` [E] or None: all valid)."""
    if status is None:
        return np.ones(N, dtype=bool)
    st = np.asarray(status).reshape(n_dim + 2, N)
    return ((st & abi.STATUS_NONFINITE) == 0).all(axis=0)


def boot_indices(seed, n_boot, N):
    """``idx[n_boot, N]``: row ``b - 1`` holds ``idx(b, j)`` of resample ``b >= 1``."""
    b = np.arange(1, n_boot + 1)[:, None, None]
    q = np.arange((N + 3) // 4)[None, :, None]
    x = np.stack(philox4x32_10((b, q, 0, BOOT_STREAM), _key(seed)), axis=-1)          # [n_boot, Q, 1, 4]
    x = x.reshape(n_boot, 4 * ((N + 3) // 4))[:, :N].astype(np.uint64)
    return ((x * np.uint64(N)) >> np.uint64(32)).astype(np.int64)


def boot_counts(seed, n_boot, N):
    """``c[1 + n_boot, N]`` int64: row 0 all ones, row ``b`` the resampling counts of resample ``b``."""
    c = np.ones((1 + n_boot, N), dtype=np.int64)
    idx = boot_indices(seed, n_boot, N)
    for b in range(n_boot):
        c[1 + b] = np.bincount(idx[b], minlength=N)
    return c


def row_terms(table, N, n_dim, valid):
    """The per-sample terms of every row over the valid samples: ``[n_rows, n_valid, 2 n_dim + 2]`` in the order
    p, s, g_0.., t_0.., and ``mu[n_rows]``."""
    f = np.asarray(table, dtype=np.float64).reshape(-1, n_dim + 2, N)[:, :, valid]
    n_valid = f.shape[2]
    with np.errstate(all='ignore'):
        mu = np.array([math.fsum(row) for row in f[:, 0] + f[:, 1]]) / (2.0 * n_valid)      # the exactly rounded sum: no order
        a, b = f[:, 0] - mu[:, None], f[:, 1] - mu[:, None]
        ab = f[:, 2:] - mu[:, None, None]
        t = np.empty((f.shape[0], n_valid, 2 * n_dim + 2))
        t[:, :, 0] = a + b
        t[:, :, 1] = a * a + b * b
        for i in range(n_dim):
            t[:, :, 2 + i] = b * (ab[:, i] - a)
            t[:, :, 2 + n_dim + i] = (a - ab[:, i]) * (a - ab[:, i])
    return t, mu


def weighted_sums(table, N, n_dim, status=None, counts=None):
    """``sums[B, n_rows, 2 n_dim + 2]`` and ``n_used[B]`` for the weight vectors ``counts[B, N]`` (default: one row of ones)."""
    valid = valid_samples(status, N, n_dim)
    counts = np.ones((1, N), dtype=np.int64) if counts is None else np.asarray(counts)
    cv = counts[:, valid]
    terms, _ = row_terms(table, N, n_dim, valid)
    cf = cv.astype(np.float64)
    sums = np.empty((cv.shape[0], terms.shape[0], terms.shape[2]))
    step = max(1, (1 << 22) // max(1, terms.shape[1] * terms.shape[2]))
    for r in range(terms.shape[0]):
        for b0 in range(0, cv.shape[0], step):
            sums[b0:b0 + step, r] = (cf[b0:b0 + step, :, None] * terms[r][None]).sum(axis=1)
    return sums, cv.sum(axis=1)


def indices_from_sums(sums, n_used, n_dim):
    """``[2, n_dim, n_rows, B]`` (plane 0: S1, plane 1: ST) and ``var[n_rows, B]`` from the sums, in the stated order."""
    sums = np.asarray(sums, dtype=np.float64)
    n_c = np.asarray(n_used).astype(np.float64)[:, None]
    with np.errstate(all='ignore'):
        m1 = sums[:, :, 0] / (2.0 * n_c)
        m2 = sums[:, :, 1] / (2.0 * n_c)
        var = m2 - m1 * m1
        s1 = (sums[:, :, 2:2 + n_dim] / n_c[:, :, None]) / var[:, :, None]
        st = (0.5 * (sums[:, :, 2 + n_dim:2 + 2 * n_dim] / n_c[:, :, None])) / var[:, :, None]
    return np.ascontiguousarray(np.stack([s1, st]).transpose(0, 3, 2, 1)), np.ascontiguousarray(var.T)


def sobol_indices(table, N, n_dim, status=None, n_boot=0, seed=0):
    """The estimator for every row of ``table[n_rows, E]``: dict(sums, n_used, indices[2, n_dim, n_rows, 1 + n_boot], var, counts)."""
    check_shape(N, n_dim)
    counts = boot_counts(seed, int(n_boot), N)
    sums, n_used = weighted_sums(table, N, n_dim, status, counts)
    ind, var = indices_from_sums(sums, n_used, n_dim)
    return dict(sums=sums, n_used=n_used, indices=ind, var=var, counts=counts)


def percentile_interval(indices, conf):
    """The percentile interval of the bootstrap axis (resamples 1..): ``[2, ...]`` = the ``(1 - conf) / 2`` and ``(1 + conf) / 2``
    quantiles (numpy's 'linear' method)."""
    return np.quantile(np.asarray(indices)[..., 1:], [(1.0 - conf) / 2.0, (1.0 + conf) / 2.0], axis=-1)
