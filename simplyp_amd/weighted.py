"""NumPy / Python-integer statement of the weighted bands (csrc/simplyp_weighted.h, csrc/simplyp_quantile.hip.h).
CPU only; the specification ``Engine.weighted_quantiles`` and ``Engine.predictive_bands(weights=)`` are tested against.

One row of a table over its member axis, integer weights ``q`` (``0 <= q_i <= 2^40``, ``1 <= E <= 2^22``: what
``particle.weights`` / ``simplyp_pf_weights`` write):

* a member takes part iff its include flag is set and ``q_i > 0``; ``T`` is the sum of the participating weights;
* the members are ordered as ``simplyp_quantiles`` orders them: NaN after +inf, -0.0 and +0.0 equal (``np.sort``'s order);
* ``C_i`` is the inclusive running sum of the weights in that order;
* for a probability ``p`` the threshold is ``t = max(1, ceil(p T))``, formed exactly, and the result is the value of the first
  member with ``C_i >= t`` -- the order statistic of rank ``t - 1`` of the multiset in which member ``i`` occurs ``q_i`` times.

This is numpy's ``method='inverted_cdf'`` with ``weights=`` on the members with ``q > 0`` (numpy forms its CDF in floating
point, so it is a cross-check, not the definition), and NOT the ``'linear'`` rule of the unweighted bands: one value per
probability.  ``T = 0``: NaN.  Everything is integer arithmetic: every implementation returns the same element of the row.

Log weights become integers through ``particle.weights(lw)['q']`` (``Engine.pf_weights`` on the device); non-negative linear
weights through ``linear_weights``.
"""

from fractions import Fraction

import numpy as np

WEIGHT_BITS = 40
MAX_WEIGHT = 1 << WEIGHT_BITS
MAX_E = 1 << 22
MAX_K = 16


def threshold(p, T):
    """``max(1, ceil(p T))`` for a probability ``p`` (a float, taken exactly) and an integer ``T >= 0``."""
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError("p = %r is not a probability in [0, 1]" % (p,))
    x = Fraction(p) * int(T)
    return max(1, -((-x.numerator) // x.denominator))


def _check_weights(q, E):
    q = np.asarray(q)
    if q.shape != (E,) or q.dtype.kind not in 'iu':
        raise ValueError("the weights must be %d integers, one per member" % E)
    if not 1 <= E <= MAX_E:
        raise ValueError("the number of members must be in [1, 2^22] (got %d)" % E)
    if E and (int(q.min()) < 0 or int(q.max()) > MAX_WEIGHT):
        raise ValueError("the weights must lie in [0, 2^40]")
    return q.astype(np.uint64)


def quantile_row(values, q, p, include=None):
    """The rule on one row, in Python integers: values [E], q [E] integer weights, p a probability."""
    values = np.asarray(values, dtype=np.float64)
    q = _check_weights(q, values.shape[0])
    take = [i for i in range(len(values)) if int(q[i]) > 0 and (include is None or include[i])]
    T = sum(int(q[i]) for i in take)
    t = threshold(p, T)
    order = np.argsort(values[take], kind='stable')          # NaN last, -0.0 == +0.0: np.sort's order
    C = 0
    for o in order:
        C += int(q[take[o]])
        if C >= t:
            return float(values[take[o]])
    return float('nan')


def quantiles(table, q, probs, include=None):
    """The rule on every row of ``table`` [..., E] (member axis last): returns [K, ...] float64.  q [E] integer weights in the
    order of the table's member axis; include [E] or None.  The running sums stay below 2^62, so uint64 holds them exactly."""
    table = np.asarray(table, dtype=np.float64)
    E = table.shape[-1]
    q = _check_weights(q, E)
    probs = np.atleast_1d(np.asarray(probs, dtype=np.float64))
    take = q > 0
    if include is not None:
        take &= np.asarray(include) != 0
    lead = table.shape[:-1]
    out = np.full((len(probs),) + lead, np.nan)
    T = sum(int(x) for x in q[take])
    for p in probs:
        threshold(p, 0)                                      # the probability's own check
    if T == 0:
        return out
    rows = table.reshape(-1, E)[:, take]
    w = q[take]
    order = np.argsort(rows, axis=1, kind='stable')
    C = np.cumsum(w[order], axis=1, dtype=np.uint64)
    sorted_rows = np.take_along_axis(rows, order, axis=1)
    for k, p in enumerate(probs):
        at = np.argmax(C >= np.uint64(threshold(p, T)), axis=1)
        out[k] = sorted_rows[np.arange(rows.shape[0]), at].reshape(lead)
    return out


def linear_weights(w):
    """Integer weights of non-negative finite linear weights ``w`` [E]: ``floor(ldexp(w / max(w), 40))`` -- the heaviest member
    gets 2^40, a member below ``max 2^-40`` gets 0.  ``ValueError`` for negative or non-finite entries and when all are zero."""
    w = np.asarray(w, dtype=np.float64)
    if w.ndim != 1 or w.size == 0:
        raise ValueError("the weights must be a vector with one entry per member")
    if not np.isfinite(w).all() or (w < 0).any():
        raise ValueError("linear weights must be finite and >= 0")
    top = w.max()
    if not top > 0:
        raise ValueError("all weights are zero: no member takes part")
    return np.floor(np.ldexp(w / top, WEIGHT_BITS)).astype(np.uint64)
