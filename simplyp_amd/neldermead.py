"""NumPy mirror of the device's multi-start Nelder-Mead simplex search (csrc/simplyp_neldermead.hip.h).  CPU only; the
specification of the algorithm.

The reference's calibration notebooks (Development/2016/MAP.ipynb, MCMC.ipynb: ``find_map``) minimise the negative log posterior
with ``scipy.optimize.fmin``: one Nelder-Mead simplex, one model run per function call.  Here ``S`` independent simplexes in
``n_dim`` dimensions (``1 <= n_dim <= 16``, ``N = n_dim``) advance together: vertices ``sim[N + 1, n_dim, S]`` with values
``fsim[N + 1, S]``, always sorted by value, inside the box ``lo <= x < hi``.

* target: ``f = -log posterior``; a point outside the box, a NaN or a -inf log posterior gives ``f = +inf``.  The target is never
  evaluated outside the box: the run point of such a candidate is the simplex's first vertex (the sampler's rule);
* coefficients: scipy's ``rho = 1, chi = 2, psi = 0.5, sigma = 0.5``;
* one iteration: ``xbar`` = the sum of the ``N`` best vertices in order ``j = 0 .. N - 1``, divided by ``N``; with ``w`` the worst
  vertex ``xr = 2 xbar - w``, ``xe = 3 xbar - 2 w``, ``xc = 1.5 xbar - 0.5 w``, ``xcc = 0.5 xbar + 0.5 w``; the decision tree is
  ``scipy.optimize._optimize._minimize_neldermead``'s, its ``<`` / ``<=`` included; a shrink is
  ``sim[j] = sim[0] + 0.5 (sim[j] - sim[0])`` for ``j >= 1`` followed by re-evaluation; the vertices are then sorted stably by
  ``f``, ties by lower former position;
* speculation: the four candidates are functions of the simplex alone, so all four are evaluated in one run and the decision is
  taken afterwards.  The path is the lazy algorithm's;
* termination, tested when an iteration is complete, i.e. at the top of the next one as scipy does: the iteration count has
  reached the limit (status 2, tested first), or ``max |sim[1:] - sim[0]| <= xatol`` and ``max |fsim[0] - fsim[1:]| <= fatol``
  (status 0).  ``n_iter`` counts like scipy's ``nit``: 1 once the initial simplex is evaluated, + 1 per iteration, so a limit
  ``max_iter`` allows ``max_iter - 1`` iterations;
* a simplex whose initial vertices do not all have a finite ``f`` ends at once with status 3.

The schedule is the device's.  Every simplex owns four member slots per run, member index ``slot * S + s``, and a phase:
``STEP`` -- the slots hold ``xr, xe, xc, xcc``; ``EVAL`` -- the slots hold up to four vertices that have no value yet, from
``cursor`` on (the initial ``N + 1``, or the ``N`` shrunk ones: ``ceil(. / 4)`` runs); ``DONE``.  Simplexes advance independently.
An idle slot holds the first vertex and is ignored.

Everything is ``+ - * /`` and comparisons in fp64, which the device evaluates without contraction: it matches this file bit for
bit.  Ties in ``f`` are sorted here by former position; scipy's ``argsort`` is not stable for more than 16 values, so a comparison
with scipy first asserts that ``min_gap`` -- the smallest difference between neighbours in any sorted ``fsim`` -- is ``> 0``.
"""

import numpy as np

from .predictive import philox4x32_10, _uniform

MAX_DIM = 16
SLOTS = 4
STEP, EVAL, DONE = 0, 1, 2
RUNNING, CONVERGED, MAXITER, NONFINITE_START = -1, 0, 2, 3            # status; 0 and 2 are scipy's
MOVES = ['reflect', 'expand', 'contract_out', 'contract_in', 'shrink']
START_STREAM = 0x4E4D5354          # "NMST": the counter's fourth word of the uniform starts


def check_box(lo, hi, n_dim):
    lo = np.asarray(lo, dtype=np.float64).reshape(-1)
    hi = np.asarray(hi, dtype=np.float64).reshape(-1)
    if not 1 <= int(n_dim) <= MAX_DIM:
        raise ValueError("n_dim must be in [1, %d] (got %d)" % (MAX_DIM, n_dim))
    if lo.shape != (n_dim,) or hi.shape != (n_dim,) or not (lo < hi).all():
        raise ValueError("the box needs lo < hi in every one of the %d dimensions" % n_dim)
    return lo, hi


def uniform_starts(seed, n_dim, S, lo, hi):
    """``x[n_dim, S]`` uniform in the box: Philox4x32-10 with key ``(seed & 0xffffffff, seed >> 32)`` and counter
    ``(s, d, 0, START_STREAM)``, ``u = uniform(x0, x1)`` in (0, 1), ``x = lo + (hi - lo) u``, kept below ``hi``."""
    lo, hi = check_box(lo, hi, n_dim)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    x0, x1, _, _ = philox4x32_10((np.arange(S)[None, :], np.arange(n_dim)[:, None], 0, START_STREAM), (seed & 0xFFFFFFFF, seed >> 32))
    x = lo[:, None] + (hi - lo)[:, None] * _uniform(x0, x1)
    return np.minimum(x, np.nextafter(hi, lo)[:, None])


def initial_simplex(x0, lo, hi):
    """scipy's initial simplex around every column of ``x0[n_dim, S]``: ``x0``, and per dimension ``k`` the point with
    ``1.05 x0[k]`` (``0.00025`` where ``x0[k] == 0``); where that vertex leaves the box, ``0.95 x0[k]`` instead; ``ValueError``
    if that leaves it too, or if ``x0`` itself does.  Returns ``sim[N + 1, n_dim, S]``."""
    x0 = np.array(x0, dtype=np.float64)
    if x0.ndim != 2:
        raise ValueError("x0 must have shape [n_dim, S]")
    n_dim, S = x0.shape
    lo, hi = check_box(lo, hi, n_dim)
    inside = (x0 >= lo[:, None]) & (x0 < hi[:, None])
    if S < 1 or not inside.all():
        bad = int(np.argmin(inside.all(axis=0))) if S else 0
        raise ValueError("the initial guess of simplex %d lies outside the box" % bad)
    sim = np.repeat(x0[None], n_dim + 1, axis=0)
    for k in range(n_dim):
        up = np.where(x0[k] != 0.0, (1 + 0.05) * x0[k], 0.00025)
        down = 0.95 * x0[k]
        up_ok = (up >= lo[k]) & (up < hi[k])
        down_ok = (down >= lo[k]) & (down < hi[k]) & (down != x0[k])
        if not (up_ok | down_ok).all():
            raise ValueError("the initial simplex of simplex %d leaves the box in dimension %d on both sides"
                             % (int(np.argmin(up_ok | down_ok)), k))
        sim[k + 1, k] = np.where(up_ok, up, down)
    return sim


def new_state(sim):
    """The state before anything is evaluated: every simplex in ``EVAL`` from vertex 0."""
    sim = np.array(sim, dtype=np.float64)
    N1, n_dim, S = sim.shape
    if N1 != n_dim + 1 or not 1 <= n_dim <= MAX_DIM or S < 1:
        raise ValueError("sim must have shape [n_dim + 1, n_dim, S] with 1 <= n_dim <= %d" % MAX_DIM)
    return dict(sim=sim, fsim=np.full((N1, S), np.inf), phase=np.full(S, EVAL, dtype=np.int32), cursor=np.zeros(S, dtype=np.int32),
                n_iter=np.zeros(S, dtype=np.int32), status=np.full(S, RUNNING, dtype=np.int32),
                counts=np.zeros((len(MOVES), S), dtype=np.int32))


def copy_state(state):
    return {k: np.array(v) for k, v in state.items()}


def pack_istate(state):
    """The integer state as the device holds it: ``istate[abi.NM_N_ISTATE, S]`` int32 (phase, cursor, n_iter, status, the five
    move counts)."""
    return np.ascontiguousarray(np.concatenate([np.stack([state[k] for k in ('phase', 'cursor', 'n_iter', 'status')]), state['counts']]),
                                dtype=np.int32)


def unpack_istate(istate, state):
    """``pack_istate``'s inverse, into ``state``."""
    istate = np.asarray(istate, dtype=np.int32)
    for i, k in enumerate(('phase', 'cursor', 'n_iter', 'status')):
        state[k] = istate[i].copy()
    state['counts'] = istate[4:].copy()
    return state


def candidates(sim):
    """``xr, xe, xc, xcc`` of sorted simplexes ``sim[N + 1, n_dim, S]``, stacked ``[4, n_dim, S]``."""
    N = sim.shape[0] - 1
    acc = sim[0].copy()
    for j in range(1, N):
        acc = acc + sim[j]
    xbar = acc / float(N)
    w = sim[N]
    return np.stack([2.0 * xbar - w, 3.0 * xbar - 2.0 * w, 1.5 * xbar - 0.5 * w, 0.5 * xbar + 0.5 * w])


def propose(state, lo, hi):
    """What the next run evaluates: dict(prop[n_dim, 4 S] -- the slots' points --, used[4 S] bool -- the slot holds a point that
    wants a value --, inside[4 S] bool -- used and inside the box --, run_point[n_dim, 4 S] -- prop where inside, the first vertex
    where not)."""
    sim, phase, cursor = state['sim'], state['phase'], state['cursor']
    N1, n_dim, S = sim.shape
    lo, hi = check_box(lo, hi, n_dim)
    prop = np.repeat(sim[0][None], SLOTS, axis=0)                       # [4, n_dim, S]: idle slots hold the first vertex
    used = np.zeros((SLOTS, S), dtype=bool)
    step = phase == STEP
    with np.errstate(all='ignore'):
        cand = candidates(sim)
    prop[:, :, step] = cand[:, :, step]
    used[:, step] = True
    lanes = np.arange(S)
    for k in range(SLOTS):
        idx = cursor + k
        ok = (phase == EVAL) & (idx < N1)
        prop[k][:, ok] = sim[idx[ok], :, lanes[ok]].T
        used[k, ok] = True
    with np.errstate(invalid='ignore'):
        inside = used & ((prop >= lo[None, :, None]) & (prop < hi[None, :, None])).all(axis=1)
    run_point = np.where(inside[:, None, :], prop, sim[0][None])
    flat = lambda a: np.ascontiguousarray(a.transpose(1, 0, 2)).reshape(n_dim, SLOTS * S)
    return dict(prop=flat(prop), used=used.reshape(-1), inside=inside.reshape(-1), run_point=flat(run_point))


def converged(sim, fsim, xatol, fatol):
    """scipy's test, per simplex."""
    with np.errstate(invalid='ignore'):
        dx = np.max(np.abs(sim[1:] - sim[0][None]).reshape(-1, sim.shape[2]), axis=0)
        df = np.max(np.abs(fsim[0][None] - fsim[1:]), axis=0)
        return (dx <= xatol) & (df <= fatol)


def counters(state):
    """What the device's update reports: how many simplexes are still active, converged, re-evaluating a shrunk simplex, and
    stopped by a non-finite start."""
    ph, st = state['phase'], state['status']
    return dict(n_active=int((ph != DONE).sum()), n_converged=int(((ph == DONE) & (st == CONVERGED)).sum()),
                n_shrinking=int(((ph == EVAL) & (state['n_iter'] >= 1)).sum()), n_nonfinite_start=int((st == NONFINITE_START).sum()))


def update(state, prop, inside, lp_prop, max_iter, xatol=1e-4, fatol=1e-4, history=None, diag=None):
    """One run's values applied to ``state`` in place.  ``prop[n_dim, 4 S]`` and ``inside[4 S]`` as ``propose`` gave them,
    ``lp_prop[4 S]`` the log posterior of the run points (``f = -lp_prop``; +inf where not inside or NaN).  ``history[rows, S]``:
    row ``n_iter - 1`` receives the best value when an iteration completes (rows past the end are dropped).  ``diag``: a dict whose
    ``'min_gap'`` is lowered to the smallest difference between neighbours of a freshly sorted ``fsim``.  Returns ``counters``."""
    sim, fsim, phase, cursor, n_iter, status, counts = (state[k] for k in ('sim', 'fsim', 'phase', 'cursor', 'n_iter', 'status', 'counts'))
    N1, n_dim, S = sim.shape
    N = N1 - 1
    lanes = np.arange(S)
    lp = np.asarray(lp_prop, dtype=np.float64).reshape(SLOTS, S)
    ins = np.asarray(inside).astype(bool).reshape(SLOTS, S)
    f = np.where(ins & ~np.isnan(lp), -lp, np.inf)
    x = np.asarray(prop, dtype=np.float64).reshape(n_dim, SLOTS, S)
    step, ev = phase == STEP, phase == EVAL

    # ---- STEP: scipy's decision tree on (fr, fe, fc, fcc)
    fr, fe, fc, fcc = f
    f0, fn1, fw = fsim[0], fsim[N - 1], fsim[N]
    low = fr < f0
    mid = ~low & (fr < fn1)
    out = ~low & ~mid & (fr < fw)
    inn = ~low & ~mid & ~out
    expand = low & (fe < fr)
    reflect = (low & ~expand) | mid
    c_out = out & (fc <= fr)
    c_in = inn & (fcc < fw)
    shrink = step & ((out & ~c_out) | (inn & ~c_in))
    sel = np.where(expand, 1, np.where(c_out, 2, np.where(c_in, 3, 0)))
    take = step & ~shrink
    for m, flag in enumerate((reflect, expand, c_out, c_in)):
        counts[m] += (take & flag).astype(np.int32)
    counts[4] += shrink.astype(np.int32)
    if take.any():
        t = lanes[take]
        f_new = f[sel[t], t]
        x_new = x[:, sel[t], t]                                              # [n_dim, n_take]
        p = (fsim[:N, t] <= f_new[None]).sum(axis=0)                         # stable: behind every vertex that is not worse
        r = np.arange(N1)[:, None]
        src = np.where(r <= p[None], r, r - 1)                               # rank r comes from rank r (r < p) or r - 1 (r > p)
        new_f = np.where(r == p[None], f_new[None], fsim[src, t[None]])
        new_x = np.where((r == p[None])[:, None, :], x_new[None], sim[src[:, None, :], np.arange(n_dim)[None, :, None], t[None, None]])
        fsim[:, t], sim[:, :, t] = new_f, new_x
    if shrink.any():
        t = lanes[shrink]
        for j in range(1, N1):
            sim[j][:, t] = sim[0][:, t] + 0.5 * (sim[j][:, t] - sim[0][:, t])
        phase[t], cursor[t] = EVAL, 1

    # ---- EVAL: store the values; when all are in, sort
    for k in range(SLOTS):
        idx = cursor + k
        ok = ev & (idx < N1)
        fsim[idx[ok], lanes[ok]] = f[k, ok]
    cursor[ev] += SLOTS
    complete = ev & (cursor >= N1)
    if complete.any():
        t = lanes[complete]
        order = np.argsort(fsim[:, t], axis=0, kind='stable')
        fsim[:, t] = np.take_along_axis(fsim[:, t], order, axis=0)
        sim[:, :, t] = np.take_along_axis(sim[:, :, t], order[:, None, :], axis=0)
        phase[t], cursor[t] = STEP, 0

    # ---- an iteration is complete: count it, note the best value, test termination
    fin = take | complete
    n_iter[fin] += 1
    if diag is not None and fin.any():
        with np.errstate(invalid='ignore'):
            gap = np.diff(fsim[:, fin], axis=0)
        gap = np.where(np.isnan(gap), 0.0, gap)
        if gap.size:
            diag['min_gap'] = min(diag.get('min_gap', np.inf), float(gap.min()))
    if history is not None:
        w = fin & (n_iter - 1 < history.shape[0])
        history[n_iter[w] - 1, lanes[w]] = fsim[0, w]
    bad_start = complete & (n_iter == 1) & ~np.isfinite(fsim).all(axis=0)
    at_limit = fin & ~bad_start & (n_iter >= max_iter)
    conv = fin & ~bad_start & ~at_limit & converged(sim, fsim, xatol, fatol)
    for flag, code in ((bad_start, NONFINITE_START), (at_limit, MAXITER), (conv, CONVERGED)):
        phase[flag], status[flag] = DONE, code
    return counters(state)


def resume(state, max_iter, xatol=1e-4, fatol=1e-4):
    """A state whose simplexes stopped at an earlier, lower limit, made ready for ``max_iter``: the termination test of the
    iteration they stopped at is taken again, as the longer call took it.  In place."""
    again = (state['phase'] == DONE) & (state['status'] == MAXITER) & (state['n_iter'] < max_iter)
    conv = again & converged(state['sim'], state['fsim'], xatol, fatol)
    state['phase'][again & ~conv], state['status'][again & ~conv] = STEP, RUNNING
    state['status'][conv] = CONVERGED
    return state


def run(f, x0=None, lo=None, hi=None, max_iter=None, xatol=1e-4, fatol=1e-4, state=None, max_runs=None):
    """Minimise ``f`` from the columns of ``x0[n_dim, S]`` (or continue ``state``).  ``f(points[n_dim, M]) -> values[M]`` is called
    once per run with the ``4 S`` run points; what it returns for a slot that is not inside the box is ignored.  Returns
    dict(x[n_dim, S], fun[S], sim, fsim, n_iter, status, history[max_iter, S] (NaN where an iteration did not happen), counts
    -- dict move -> [S] --, min_gap, n_runs, state)."""
    if state is None:
        state = new_state(initial_simplex(x0, lo, hi))
        history = None
    else:
        history = state.get('history')
        state = copy_state({k: v for k, v in state.items() if k != 'history'})
    n_dim, S = state['sim'].shape[1:]
    lo, hi = check_box(lo, hi, n_dim)
    max_iter = 200 * n_dim if max_iter is None else int(max_iter)
    if max_iter < 1:
        raise ValueError("max_iter must be >= 1")
    resume(state, max_iter, xatol, fatol)
    hist = np.full((max_iter, S), np.nan)
    if history is not None:
        rows = min(len(history), max_iter)
        hist[:rows] = np.asarray(history)[:rows]
    diag = dict(min_gap=np.inf)
    n_runs = 0
    while (state['phase'] != DONE).any() and (max_runs is None or n_runs < max_runs):
        pr = propose(state, lo, hi)
        with np.errstate(all='ignore'):
            val = np.asarray(f(pr['run_point']), dtype=np.float64)
        update(state, pr['prop'], pr['inside'], -val, max_iter, xatol, fatol, hist, diag)
        n_runs += 1
    return dict(x=state['sim'][0].copy(), fun=state['fsim'][0].copy(), sim=state['sim'], fsim=state['fsim'], n_iter=state['n_iter'],
                status=state['status'], history=hist, counts={m: state['counts'][i] for i, m in enumerate(MOVES)},
                min_gap=diag['min_gap'], n_runs=n_runs, state=dict(state, history=hist))
