"""Python-integer / ``fractions.Fraction`` statement of the scores (csrc/simplyp_score.h, csrc/simplyp_score.hip.h).  CPU only;
the specification ``Engine.scores`` and ``Engine.predictive_scores`` are tested against.

One row of a table over its member axis (values ``x_j``), one observation ``y``.  Participation and order are those of
``simplyp_amd.weighted``: member ``j`` takes part iff its include flag is set and its integer weight ``q_j > 0`` (no weights:
``q_j = 1``); ``T`` is the sum of the participating weights; NaN sorts after +inf, -0.0 and +0.0 are equal.

* ``below`` = sum q_j [x_j < y] and ``at_or_below`` = sum q_j [x_j <= y]: integers.  A NaN member is above every ``y``.  They are
  ``T F(y-)`` and ``T F(y)`` of the weighted empirical CDF whose inverse ``weighted.quantiles`` returns.
* ``abs_err`` A = (1/T) sum q_j |x_j - y|.
* ``spread`` B = (1/T^2) sum_k (x_(k+1) - x_(k)) C_k (T - C_k) over the participating values in key order, ``C_k`` the inclusive
  running weight: half the expected distance of two independent draws (``pairwise_spread``), written over the gaps.
* CRPS = A - B, the integral of (F - 1{x >= y})^2.

A row whose ``y`` is NaN is not scored (None / NaN, counts 0); ``y = +-inf`` is an error; a participating non-finite value makes
A and B NaN and leaves the counts exact; ``T == 0`` gives NaN and 0.  A and B are exact here: every float is a dyadic rational.
"""

from fractions import Fraction
import math

import numpy as np

from . import weighted


def _participants(values, weights, include):
    values = np.asarray(values, dtype=np.float64)
    E = values.shape[-1]
    q = np.ones(E, dtype=np.uint64) if weights is None else weighted._check_weights(weights, E)
    take = q > 0
    if include is not None:
        inc = np.asarray(include) != 0
        if inc.shape != (E,):
            raise ValueError("include must have one entry per member")
        take = take & inc
    return values, q, take


def _exact(x, y):
    """The finite floats ``x`` [n] and ``y`` as integers on one power-of-two scale: (X object array, Y, scale as a Fraction)."""
    m, e = np.frexp(np.append(x, y))
    lo = int(e.min()) - 53
    ints = [int(math.ldexp(float(mi), 53)) << (int(ei) - 53 - lo) for mi, ei in zip(m, e)]      # |m| 2^53 is an integer
    scale = Fraction(2) ** lo
    return np.array(ints[:-1], dtype=object), ints[-1], scale


def score_row(values, y, weights=None, include=None):
    """The rule on one row: dict(abs_err, spread (Fractions, or None where the rule says NaN), below, at_or_below, T)."""
    y = float(y)
    if math.isinf(y):
        raise ValueError("an observation must be finite, or NaN for none")
    values, q, take = _participants(values, weights, include)
    if values.ndim != 1:
        raise ValueError("score_row takes one row")
    if math.isnan(y):
        return dict(abs_err=None, spread=None, below=0, at_or_below=0, T=0)
    x = values[take]
    w = np.array([int(v) for v in q[take]], dtype=object)
    T = int(w.sum()) if len(w) else 0
    if T == 0:
        return dict(abs_err=None, spread=None, below=0, at_or_below=0, T=0)
    below = int(w[x < y].sum()) if (x < y).any() else 0
    at_or_below = int(w[x <= y].sum()) if (x <= y).any() else 0
    if not np.isfinite(x).all():
        return dict(abs_err=None, spread=None, below=below, at_or_below=at_or_below, T=T)
    order = np.argsort(x, kind='stable')
    X, Y, scale = _exact(x[order], y)
    w = w[order]
    A = Fraction(int((w * abs(X - Y)).sum()), T) * scale
    if len(X) > 1:
        C = np.cumsum(w)[:-1]
        B = Fraction(int(((X[1:] - X[:-1]) * C * (T - C)).sum()), T * T) * scale
    else:
        B = Fraction(0)
    return dict(abs_err=A, spread=B, below=below, at_or_below=at_or_below, T=T)


def pairwise_spread(values, weights=None, include=None):
    """B straight from its definition, (1 / 2 T^2) sum_i sum_j q_i q_j |x_i - x_j|, as a Fraction (None: nobody takes part or
    a participating value is not finite).  Quadratic in the members: for checking ``score_row``."""
    values, q, take = _participants(values, weights, include)
    x = [Fraction(float(v)) if math.isfinite(v) else None for v in values[take]]
    w = [int(v) for v in q[take]]
    T = sum(w)
    if T == 0 or any(v is None for v in x):
        return None
    total = sum(w[i] * w[j] * abs(x[i] - x[j]) for i in range(len(x)) for j in range(i + 1, len(x)))     # each pair once
    return Fraction(total) / (T * T)


def scores(table, y, weights=None, include=None):
    """The rule on every row of ``table`` [..., E] against ``y`` [...]: dict of arrays of shape ``table.shape[:-1]`` --
    ``abs_err``, ``spread``, ``crps`` (float64, rounded once from the exact value; NaN where not scored), ``below``,
    ``at_or_below`` (uint64), ``exact`` (object array of (A, B) Fractions or None) -- and ``T``."""
    table = np.asarray(table, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    lead = table.shape[:-1]
    if y.shape != lead:
        raise ValueError("y must have one observation per row")
    rows = table.reshape(-1, table.shape[-1])
    n = rows.shape[0]
    out = dict(abs_err=np.full(n, np.nan), spread=np.full(n, np.nan), crps=np.full(n, np.nan),
               below=np.zeros(n, dtype=np.uint64), at_or_below=np.zeros(n, dtype=np.uint64), exact=np.empty(n, dtype=object))
    _, q, take = _participants(rows[0] if n else np.zeros(table.shape[-1]), weights, include)
    for r, yr in enumerate(y.reshape(-1)):
        s = score_row(rows[r], yr, weights, include)
        out['below'][r], out['at_or_below'][r] = s['below'], s['at_or_below']
        if s['abs_err'] is not None:
            out['exact'][r] = (s['abs_err'], s['spread'])
            out['abs_err'][r], out['spread'][r] = float(s['abs_err']), float(s['spread'])
            out['crps'][r] = float(s['abs_err'] - s['spread'])
    out = {k: v.reshape(lead) for k, v in out.items()}
    out['T'] = sum(int(v) for v in q[take])
    return out


def pit(below, at_or_below, T):
    """The probability integral transform of an observation whose CDF interval is [below / T, at_or_below / T]: its mid-point
    ``(L + M) / (2 T)``, float64 (NaN where T is 0).  Arrays or scalars; ``T`` a scalar."""
    L = np.asarray(below).astype(object)
    M = np.asarray(at_or_below).astype(object)
    T = int(T)
    if T == 0:
        return np.full(L.shape, np.nan)
    flat = [float(Fraction(int(l) + int(m), 2 * T)) for l, m in zip(L.reshape(-1), M.reshape(-1))]
    return np.array(flat, dtype=np.float64).reshape(L.shape)


def pit_histogram(below, at_or_below, T, n_bins, observed=None):
    """The rank histogram over ``n_bins`` equal bins of [0, 1]: every observation's interval [L / T, M / T] is spread uniformly
    over the bins it overlaps; ``L == M`` is a point mass at L / T, and 1.0 goes into the last bin.  float64 [n_bins]; its sum
    is the number of observations.  ``observed``: a bool array like ``below``, True where there was an observation -- an
    unscored row carries ``below == at_or_below == 0``, which the counts alone cannot tell from an observation under every
    member, so the arrays of ``res['scores']`` need ``observed=~np.isnan(crps)``; None: every entry is an observation."""
    T, n_bins = int(T), int(n_bins)
    if n_bins < 1:
        raise ValueError("n_bins must be >= 1")
    below, at_or_below = np.asarray(below), np.asarray(at_or_below)
    if observed is not None:
        observed = np.asarray(observed, dtype=bool)
        if observed.shape != below.shape:
            raise ValueError("observed must have the shape of below")
        below, at_or_below = below[observed], at_or_below[observed]
    hist = [Fraction(0)] * n_bins
    if T > 0:
        for l, m in zip(below.reshape(-1), at_or_below.reshape(-1)):
            l, m = int(l), int(m)
            if not 0 <= l <= m <= T:
                raise ValueError("need 0 <= below <= at_or_below <= T")
            if l == m:
                hist[min(l * n_bins // T, n_bins - 1)] += 1
                continue
            lo, hi = Fraction(l, T), Fraction(m, T)
            for b in range(l * n_bins // T, min(-((-m * n_bins) // T), n_bins)):
                a, z = max(lo, Fraction(b, n_bins)), min(hi, Fraction(b + 1, n_bins))
                if z > a:
                    hist[b] += (z - a) / (hi - lo)
    return np.array([float(h) for h in hist], dtype=np.float64)
