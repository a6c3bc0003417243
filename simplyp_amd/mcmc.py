"""NumPy mirror of the device's affine-invariant ensemble sampler (csrc/simplyp_mcmc.hip.h).  CPU only; the specification
of the move.

The reference's calibration notebook (Development/2016/MCMC.ipynb, cell 10) samples its posterior with
``emcee.EnsembleSampler(n_walk, n_dim, log_posterior).run_mcmc(start, n_steps)``: the stretch move of Goodman & Weare
(2010).  Here ``W`` walkers (``W`` even, ``W >= 2 n_dim``, ``1 <= n_dim <= 16``) hold positions ``theta[n_dim, W]`` and log
posteriors ``lp[W]``; a step ``t`` (absolute: counted from the start of the chain, continuing across calls) moves half 0
against half 1, then half 1 against the new half 0.  With ``h = W / 2``, the active walkers of half ``k`` are
``i in [k h, (k + 1) h)`` and their partners come from the other half, offset ``c = (1 - k) h``:

* draw A: Philox4x32-10 (``predictive.philox4x32_10``), key ``(seed & 0xffffffff, seed >> 32)``, counter
  ``(i, t, 0, 0x4D434D43)``: ``u_z = uniform(x0, x1)``, partner ``j = c + ((uint64(x2) * h) >> 32)``;
* ``s = (a - 1) u_z + 1``, ``z = (s s) / a``: emcee's g(z) on ``[1/a, a]``;
* ``y[d] = x_j[d] + z (x_i[d] - x_j[d])``; inside iff ``lo[d] <= y[d] < hi[d]`` for every ``d`` (the reference's
  ``log_prior``; a NaN is outside);
* the target is evaluated at ``y`` where inside and at the walker's current position where not: it never sees a point
  outside the box;
* draw B: counter ``(i, t, 1, 0x4D434D43)``: ``u_a = uniform(x0, x1)``;
* ``margin = (n_dim - 1) ln z + lp_y - lp[i] - ln u_a``; accept iff inside, ``lp_y`` is not NaN and ``margin > 0``.

Everything but the two logarithms is integer arithmetic or ``+ * /`` in fp64, which the device evaluates without
contraction: partner, z, y and inside match it bit for bit, and a decision matches whenever ``|margin|`` exceeds the
rounding of ``log`` (``run_chain`` returns the smallest ``|margin|`` it met so that a test can assert that first).
"""

import numpy as np

from .predictive import philox4x32_10, _uniform

STREAM = 0x4D434D43          # "MCMC": the counter's fourth word
MAX_DIM = 16


def check_shape(W, n_dim, a=2.0):
    """The sampler's shape rules; raises ValueError."""
    if not 1 <= int(n_dim) <= MAX_DIM:
        raise ValueError("n_dim must be in [1, %d] (got %d)" % (MAX_DIM, n_dim))
    if int(W) < 2 or int(W) % 2 or int(W) < 2 * int(n_dim):
        raise ValueError("the number of walkers must be even and >= 2 n_dim (got %d walkers, n_dim = %d)" % (W, n_dim))
    if not float(a) > 1.0:
        raise ValueError("the stretch scale a must be > 1 (got %r)" % (a,))


def _key(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32


def stretch(W, half, t, a=2.0, seed=0):
    """(i, j, z) of the active walkers of ``half`` at step ``t``: their indices, their partners' and the stretch factors."""
    h = W // 2
    i = half * h + np.arange(h, dtype=np.int64)
    x0, x1, x2, _ = philox4x32_10((i, int(t) & 0xFFFFFFFF, 0, STREAM), _key(seed))
    u_z = _uniform(x0, x1)
    j = (1 - half) * h + ((x2.astype(np.uint64) * np.uint64(h)) >> np.uint64(32)).astype(np.int64)
    s = (a - 1.0) * u_z + 1.0
    return i, j, (s * s) / a


def propose(theta, half, t, lo, hi, a=2.0, seed=0):
    """The proposals of ``half`` at step ``t`` from positions ``theta[n_dim, W]``: dict(prop[n_dim, h], inside[h] bool,
    run_point[n_dim, h] -- the proposal where inside, the current position where not --, partner[h], z[h])."""
    theta = np.asarray(theta, dtype=np.float64)
    n_dim, W = theta.shape
    check_shape(W, n_dim, a)
    if half not in (0, 1):
        raise ValueError("half must be 0 or 1")
    lo = np.asarray(lo, dtype=np.float64).reshape(n_dim, 1)
    hi = np.asarray(hi, dtype=np.float64).reshape(n_dim, 1)
    if not (lo < hi).all():
        raise ValueError("the box needs lo < hi in every dimension")
    i, j, z = stretch(W, half, t, a, seed)
    xi, xj = theta[:, i], theta[:, j]
    with np.errstate(all='ignore'):
        y = xj + z * (xi - xj)
        inside = ((y >= lo) & (y < hi)).all(axis=0)
    return dict(prop=y, inside=inside, run_point=np.where(inside, y, xi), partner=j, z=z)


def accept(theta, lp, n_accept, half, t, prop, inside, lp_prop, a=2.0, seed=0):
    """The decisions of ``half`` at step ``t``, applied in place to ``theta[n_dim, W]``, ``lp[W]`` and ``n_accept[W]``.
    Returns (accepted[h] bool, margin[h])."""
    n_dim, W = theta.shape
    h = W // 2
    i, _, z = stretch(W, half, t, a, seed)
    x0, x1, _, _ = philox4x32_10((i, int(t) & 0xFFFFFFFF, 1, STREAM), _key(seed))
    u_a = _uniform(x0, x1)
    lp_prop = np.asarray(lp_prop, dtype=np.float64)
    with np.errstate(all='ignore'):
        margin = float(n_dim - 1) * np.log(z) + lp_prop - lp[i] - np.log(u_a)
        acc = np.asarray(inside, dtype=bool) & ~np.isnan(lp_prop) & (margin > 0.0)
    ia = i[acc]
    theta[:, ia] = np.asarray(prop)[:, acc]
    lp[ia] = lp_prop[acc]
    n_accept[ia] += 1
    assert len(i) == h
    return acc, margin


def run_chain(log_prob_fn, theta, lp, n_steps, lo, hi, a=2.0, seed=0, t0=0, n_accept=None, thin=1):
    """``n_steps`` steps from positions ``theta[n_dim, W]`` with log posteriors ``lp[W]`` (neither is modified), absolute
    step indices ``t0 .. t0 + n_steps - 1``.  ``log_prob_fn(points[n_dim, h]) -> lp[h]`` is called once per half-step with
    the run points; a proposal outside the box gets -inf whatever it returns.  Step ``t`` is kept when ``(t + 1) % thin == 0``.
    Returns dict(chain[n_kept, n_dim, W], log_prob[n_kept, W], theta, lp, n_accept, t = the next step, min_abs_margin = the
    smallest |margin| among the decisions the margin settled (inside, lp finite), n_inside, n_accepted: per half-step lists)."""
    theta = np.array(theta, dtype=np.float64)
    lp = np.array(lp, dtype=np.float64)
    n_dim, W = theta.shape
    n_accept = np.zeros(W, dtype=np.int64) if n_accept is None else np.array(n_accept, dtype=np.int64)
    chain, chain_lp, n_in, n_acc = [], [], [], []
    min_margin = np.inf
    for t in range(int(t0), int(t0) + int(n_steps)):
        for half in (0, 1):
            pr = propose(theta, half, t, lo, hi, a, seed)
            lp_y = np.array(log_prob_fn(pr['run_point']), dtype=np.float64)
            lp_y[~pr['inside']] = -np.inf
            acc, margin = accept(theta, lp, n_accept, half, t, pr['prop'], pr['inside'], lp_y, a, seed)
            settled = pr['inside'] & np.isfinite(margin)
            if settled.any():
                min_margin = min(min_margin, float(np.abs(margin[settled]).min()))
            n_in.append(int(pr['inside'].sum()))
            n_acc.append(int(acc.sum()))
        if (t + 1) % int(thin) == 0:
            chain.append(theta.copy())
            chain_lp.append(lp.copy())
    return dict(chain=np.array(chain).reshape(len(chain), n_dim, W), log_prob=np.array(chain_lp).reshape(len(chain_lp), W),
                theta=theta, lp=lp, n_accept=n_accept, t=int(t0) + int(n_steps), min_abs_margin=min_margin,
                n_inside=n_in, n_accepted=n_acc)
