"""NumPy statement of the device's particle filter (csrc/simplyp_particle.hip.h, csrc/simplyp_resample.h).  CPU only; the
specification of the steps ``assimilate`` chains between two model runs.

Sequential importance resampling over the joint (state, parameter) space: ``E`` particles (``1 <= E <= 2^22``), each a member of
the ensemble with its model state, its parameters, its position ``theta[n_dim]`` in the prior box and its log weight.  One
assimilation window ``t`` (absolute: counted from the start of the filter, continuing across calls) is

* the model over the window's days from every particle's state;
* ``loglik_increment``: the window's Gaussian log-likelihood with ``sigma = m sim`` -- ``visualise_results.loglik`` without the
  more-than-10-observations rule --, added to the log weights.  For one (variable, reach) pair with ``n`` observation days in
  the window, ``term = -0.5 n ln(2 pi) - n ln(m) - sum ln sim - sum (obs / sim - 1)^2 / (2 m m)``, in that order; the
  increment is the sum of the pairs' terms in the given order from +0.0, and a pair without an observation adds nothing.  It
  is -inf for a run flagged non-finite, for an ``m <= 0`` and where the sum is NaN -- a NaN simulated value on an observation
  day among them: a particle may not skip an observation;
* ``weights``: ``w = exp(lw - lw_max)`` (exactly 1 at the maximum, 0 at -inf, +inf and NaN), ``q = floor(w 2^40)``: the filter
  resolves weights to 2^-40, a particle more than ``40 ln 2`` below the maximum is dead.  ``ESS = sum_w^2 / sum_w2``, and
  ``log_mean = lw_max + ln(sum_w / E)`` is the log of the mean weight, whose change over a window is the window's evidence;
* ``resample``: systematic resampling in integers.  ``C_i`` the inclusive prefix sum of ``q``, ``T = C_{E-1}``;
  ``x = (x0 << 32) | x1`` of Philox4x32-10 under key ``(seed & 0xffffffff, seed >> 32)`` at counter ``(t, 0, 0, RESAMPLE_STREAM)``;
  ``r = (x T) >> 64``; the ancestor of particle ``k`` is the smallest ``i`` with ``E C_i > k T + r``.  Nothing is rounded: any
  implementation gives the same ancestors;
* ``jitter``: the rejuvenation move ``y[d] = centre[d] + a (theta[d] - centre[d]) + scale[d] z`` with ``z`` the standard normal
  of the predictive stream at counter ``(k, t, d, JITTER_STREAM)``; a particle any of whose ``y[d]`` leaves ``lo <= y < hi`` keeps
  its whole position.  ``liu_west`` gives the ``a``, ``centre`` and ``scale`` of Liu & West (2001).

The integers match the device bit for bit; ``y`` differs by the roundings of ``z`` only (``predictive.standard_normal``).
"""

import numpy as np

from . import predictive
from .predictive import philox4x32_10

RESAMPLE_STREAM = 0x50465253     # "PFRS": the counter's fourth word of the resampling offset
JITTER_STREAM = 0x50464A54       # "PFJT": ... of the rejuvenation move's normals
START_STREAM = 0x50465354        # "PFST": ... of the uniform start in the prior box
WEIGHT_BITS = 40
MAX_E = 1 << 22
MAX_DIM = 16
LN_2PI = float(np.log(2 * np.pi))


def _key(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32


def check_shape(E, n_dim=1):
    """The filter's shape rules; raises ValueError."""
    if not 1 <= int(E) <= MAX_E:
        raise ValueError("the number of particles must be in [1, 2^22] (got %d)" % E)
    if not 1 <= int(n_dim) <= MAX_DIM:
        raise ValueError("n_dim must be in [1, %d] (got %d)" % (MAX_DIM, n_dim))


def loglik_increment(sim, obs, m, status_ok=None):
    """The log-likelihood increment of every particle.  sim [n_pairs, D, E]: the simulated series of each pair over the
    window's days; obs [n_pairs, D], NaN = no observation; m [n_pairs, E] (or broadcastable to it).  Returns (inc [E],
    scale [E]): the increment and the sum of the absolute values of everything that was added to form it -- what a
    comparison's tolerance is a multiple of."""
    sim = np.asarray(sim, dtype=np.float64)
    obs = np.asarray(obs, dtype=np.float64)
    n_pairs, D, E = sim.shape
    m = np.broadcast_to(np.asarray(m, dtype=np.float64), (n_pairs, E))
    inc, scale = np.zeros(E), np.zeros(E)
    with np.errstate(all='ignore'):
        for p in range(n_pairs):
            have = ~np.isnan(obs[p])
            n = float(have.sum())
            if n == 0:
                continue
            s, o = sim[p][have], obs[p][have][:, None]
            ls, rq = np.log(s), (o / s - 1.0) ** 2
            SL, SR = ls.sum(axis=0), rq.sum(axis=0)
            lm = np.log(np.where(m[p] > 0, m[p], 1.0))
            term = (((-0.5 * n) * LN_2PI) - n * lm - SL) - SR / ((2.0 * m[p]) * m[p])
            inc = inc + term
            scale = scale + (0.5 * n * LN_2PI + n * np.abs(lm) + np.abs(ls).sum(axis=0) + SR / ((2.0 * m[p]) * m[p]))
        dead = np.isnan(inc) | (m <= 0).any(axis=0)
        if status_ok is not None:
            dead = dead | ~np.asarray(status_ok, dtype=bool)
    return np.where(dead, -np.inf, inc), scale


def weights(lw):
    """dict(w [E] float64, q [E] uint64, lw_max, sum_w, sum_w2, T (Python int), n_alive, n_nan) of the log weights lw [E]."""
    lw = np.asarray(lw, dtype=np.float64)
    fin = np.isfinite(lw)
    lw_max = float(lw[fin].max()) if fin.any() else -np.inf
    w = np.zeros(lw.shape)
    if fin.any():
        with np.errstate(all='ignore'):
            w[fin] = np.where(lw[fin] == lw_max, 1.0, np.exp(lw[fin] - lw_max))
    q = np.floor(w * 2.0 ** WEIGHT_BITS).astype(np.uint64)
    return dict(w=w, q=q, lw_max=lw_max, sum_w=float(w.sum()), sum_w2=float((w * w).sum()), T=sum(int(x) for x in q),
                n_alive=int((q > 0).sum()), n_nan=int((~fin & ~(lw < 0)).sum()))


def ess(sum_w, sum_w2):
    return sum_w * sum_w / sum_w2 if sum_w2 > 0 else 0.0


def log_mean(lw_max, sum_w, E):
    with np.errstate(divide='ignore'):
        return float(lw_max + np.log(sum_w / E)) if sum_w > 0 else -np.inf


def resample_offset(seed, t, T):
    """r of assimilation step t: the high 64 bits of x T."""
    x0, x1, _, _ = philox4x32_10((int(t) & 0xFFFFFFFF, 0, 0, RESAMPLE_STREAM), _key(seed))
    return (((int(x0) << 32) | int(x1)) * int(T)) >> 64


def resample(q, seed, t, r=None):
    """dict(ancestors [E] int32, offspring [E] int32, n_unique, T, r) of the integer weights q [E].  The definition in Python
    integers: the ancestor of k is the smallest i with ``E C_i > k T + r``, that is with ``C_i > (k T + r) // E`` (C_i is an
    integer).  ``r``: the offset instead of the Philox word's (a test hook).  T = 0: the identity, no offspring, n_unique = 0."""
    qs = [int(x) for x in np.asarray(q).ravel()]
    E = len(qs)
    check_shape(E)
    if any(x < 0 or x > 1 << WEIGHT_BITS for x in qs):
        raise ValueError("q must lie in [0, 2^40]")
    C, c = [], 0
    for x in qs:
        c += x
        C.append(c)
    T = c
    if T == 0:
        return dict(ancestors=np.arange(E, dtype=np.int32), offspring=np.zeros(E, dtype=np.int32), n_unique=0, T=0, r=0)
    r = resample_offset(seed, t, T) if r is None else int(r)
    if not 0 <= r < T:
        raise ValueError("r must lie in [0, T)")
    bar = np.array([(k * T + r) // E for k in range(E)], dtype=np.uint64)          # < T <= 2^62: exact
    anc = np.searchsorted(np.array(C, dtype=np.uint64), bar, side='right').astype(np.int32)
    off = np.bincount(anc, minlength=E).astype(np.int32)
    return dict(ancestors=anc, offspring=off, n_unique=int((off > 0).sum()), T=T, r=r)


def jitter_normals(seed, t, n_dim, E):
    """z [n_dim, E] of step t."""
    return predictive.standard_normal(int(seed), np.arange(E)[None, :], int(t) & 0xFFFFFFFF, np.arange(n_dim)[:, None], JITTER_STREAM)


def jitter(theta, t, a, centre, scale, lo, hi, seed=0):
    """The rejuvenation move of step t on theta [n_dim, E] (not modified).  Returns dict(theta -- the new positions --, y -- the
    proposals --, inside [E] bool, z)."""
    theta = np.asarray(theta, dtype=np.float64)
    n_dim, E = theta.shape
    check_shape(E, n_dim)
    col = lambda v: np.asarray(v, dtype=np.float64).reshape(n_dim, 1)
    centre, scale, lo, hi = col(centre), col(scale), col(lo), col(hi)
    z = jitter_normals(seed, t, n_dim, E)
    with np.errstate(all='ignore'):
        y = (centre + float(a) * (theta - centre)) + scale * z
        inside = ((y >= lo) & (y < hi)).all(axis=0)
    return dict(theta=np.where(inside, y, theta), y=y, inside=inside, z=z)


def liu_west(theta, delta):
    """(a, centre [n_dim], scale [n_dim]) of Liu & West's kernel shrinkage for equally weighted positions theta [n_dim, E]:
    ``a = (3 delta - 1) / (2 delta)``, the mean, and ``sqrt(1 - a^2)`` times the standard deviation (ddof 0)."""
    theta = np.asarray(theta, dtype=np.float64)
    a = (3.0 * float(delta) - 1.0) / (2.0 * float(delta))
    return a, theta.mean(axis=1), np.sqrt(1.0 - a * a) * theta.std(axis=1)


def uniform_start(seed, n_dim, E, lo, hi):
    """The start for ``start=None``: ``lo + (hi - lo) u`` with ``u`` the uniform of Philox counter ``(k, d, 0, START_STREAM)``."""
    x0, x1, _, _ = philox4x32_10((np.arange(E)[None, :], np.arange(n_dim)[:, None], 0, START_STREAM), _key(seed))
    u = predictive._uniform(x0, x1)
    lo, hi = np.asarray(lo, dtype=np.float64)[:, None], np.asarray(hi, dtype=np.float64)[:, None]
    return lo + (hi - lo) * u


def run_filter(step_fn, theta, n_windows, lo, hi, seed=0, resample_threshold=1.0, delta=0.98, state=None, record=False):
    """The whole loop with ``step_fn`` in place of the model and the likelihood.  ``step_fn(t, theta [n_dim, E], x) -> (inc [E], x')``
    advances the caller's own per-particle state ``x`` (an array whose LAST axis is the particle axis, or None) over window ``t``
    and returns the log-likelihood increments.  theta [n_dim, E]: the start (not modified); ``state``: the ``'state'`` of an
    earlier result -- the filter continues from it bit for bit (``theta`` is ignored).  ``delta``: Liu & West's discount, or None
    for no rejuvenation.  Returns dict(theta, lw, x, ess [n], log_evidence [n], resampled [n], n_unique [n], n_outside [n],
    log_evidence_total, state = dict(theta, lw, x, t, seed), and with ``record`` per window inc, q, ancestors, theta_before,
    theta_after).  RuntimeError when every particle is dead."""
    if state is not None:
        theta, lw, x, t0, seed = (np.array(state['theta'], dtype=np.float64), np.array(state['lw'], dtype=np.float64),
                                  None if state['x'] is None else np.array(state['x']), int(state['t']), int(state['seed']))
    else:
        theta = np.array(theta, dtype=np.float64)
        lw, x, t0 = np.zeros(theta.shape[1]), None, 0
    n_dim, E = theta.shape
    check_shape(E, n_dim)
    out = dict(ess=[], log_evidence=[], resampled=[], n_unique=[], n_outside=[])
    rec = dict(inc=[], q=[], ancestors=[], theta_before=[], theta_after=[])
    for t in range(t0, t0 + int(n_windows)):
        before = weights(lw)
        lm0 = log_mean(before['lw_max'], before['sum_w'], E)
        inc, x = step_fn(t, theta.copy(), x)
        lw = lw + np.asarray(inc, dtype=np.float64)
        wt = weights(lw)
        if wt['T'] == 0:
            raise RuntimeError("every particle is dead in window %d" % t)
        e = ess(wt['sum_w'], wt['sum_w2'])
        out['ess'].append(e)
        out['log_evidence'].append(log_mean(wt['lw_max'], wt['sum_w'], E) - lm0)
        do = e < float(resample_threshold) * E
        theta_before = theta.copy()
        anc, n_unique, n_outside = np.arange(E, dtype=np.int32), E, 0
        if do:
            rs = resample(wt['q'], seed, t)
            anc, n_unique = rs['ancestors'], rs['n_unique']
            theta, lw = theta[:, anc], np.zeros(E)
            x = None if x is None else np.asarray(x)[..., anc]
            if delta is not None:
                a, centre, scale = liu_west(theta, delta)
                jt = jitter(theta, t, a, centre, scale, lo, hi, seed)
                theta, n_outside = jt['theta'], int((~jt['inside']).sum())
        out['resampled'].append(bool(do))
        out['n_unique'].append(n_unique)
        out['n_outside'].append(n_outside)
        if record:
            for k, v in zip(('inc', 'q', 'ancestors', 'theta_before', 'theta_after'), (np.array(inc), wt['q'], anc, theta_before, theta.copy())):
                rec[k].append(v)
    res = {k: np.array(v) for k, v in out.items()}
    res.update(theta=theta, lw=lw, x=x, log_evidence_total=float(np.sum(res['log_evidence'])) if len(res['log_evidence']) else 0.0,
               state=dict(theta=theta.copy(), lw=lw.copy(), x=None if x is None else np.array(x), t=t0 + int(n_windows), seed=int(seed)))
    if record:
        res.update(rec)
    return res
