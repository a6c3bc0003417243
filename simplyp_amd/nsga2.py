"""NumPy statement of the device's NSGA-II (csrc/simplyp_nsga2.hip.h; csrc/simplyp_nsga2.h holds the variation in plain C++).
CPU only; the definition of the rule: crowding distance, environmental selection, mating and variation (Deb, Pratap, Agarwal &
Meyarivan 2002), and the draws.

Population.  ``N`` members (``N`` even, ``4 <= N <= 65536``), positions ``theta[n_dim, N]`` (``1 <= n_dim <= 16``), objectives
``obj[M, N]`` (``1 <= M <= 8``) under ``sense[m] = +-1`` as in ``simplyp_amd.pareto``: ``y = sense x``.  The box is closed,
``lo <= x <= hi``; children are clipped into it.  A member is *valid* iff all its objectives are finite and its run status
lacks ``STATUS_NONFINITE`` (``valid_mask``): that is the ``include`` mask of the Pareto ranks, which give an invalid member
rank -1 -- read below as worse than any rank, with crowding 0.

Crowding (``crowding``), for a member i of rank >= 0 in a set of n: within its front and for each objective m, the front's
members are ordered by ``(y[m], index)`` -- -0.0 and +0.0 tie, the index decides.  ``prev`` and ``next`` are i's neighbours in
that order and ``span = y_max - y_min`` of the front.  If i is first or last in the order of any m, ``d_i = +inf``; otherwise
``d_i = ((0 + term_0) + term_1) + ...`` with ``term_m = (y_next - y_prev) / span`` for ``span > 0`` and 0 otherwise.  The sum
starts at +0.0, so a term of -0.0 (two zeros of different sign as neighbours) leaves no trace and the value does not depend
on which zero an implementation carries.  Operands are selections (min / max), never sums: every correct implementation has
the same bits.

Selection (``positions``, ``select``).  The n members are ordered by (rank ascending, rank -1 last; crowding descending;
index ascending); crowding is compared through its order-preserving key (``pareto.keys``: the numeric order, -0.0 = +0.0).  A
member's *position* is the number of members before it; the survivors are positions ``0 .. N - 1``, stored at their
position, with the rank and crowding they had in the combined set.

Mating (``mating``).  Child pair p of generation t has two binary tournaments, each between ``(x N) >> 32`` of two Philox
words; the winner has the lower rank (rank -1 last), then the larger crowding, then the lower index.

Variation (``vary``): Deb's bounded SBX and bounded polynomial mutation with ``eta = 2^k - 1``, ``k`` in 1 .. 5: every
``(.)^(eta + 1)`` is k squarings (``powk``) and every ``(.)^(1 / (eta + 1))`` is k nested IEEE square roots (``rootk``) -- no
pow, exp or log, so NumPy, host C++ and the device agree bit for bit (no contraction; fp64 sqrt and / correctly rounded).

Draws.  Philox4x32-10 (``predictive.philox4x32_10``), key ``(seed & 0xffffffff, seed >> 32)``, counter
``(p or i, t, purpose, STREAM)`` with ``purpose = code << 8 | d``:

* ``TOURNAMENT`` (p, t, d = 0): candidates ``(x0 N) >> 32`` and ``(x1 N) >> 32`` of the first parent, ``x2``, ``x3`` of the second;
* ``CROSS`` (p, t, d = 0): ``u = uniform(x0, x1)``; the pair crosses iff ``u < p_cross``;
* ``SBX`` (p, t, d): three uniforms: ``u = uniform(x0, x1)`` the spread, ``u_take = (x2 + 0.5) 2^-32`` -- the dimension takes part
  iff ``u_take < 0.5`` --, ``u_swap = (x3 + 0.5) 2^-32`` -- the two children are swapped iff ``u_swap < 0.5``;
* ``MUTATE_A`` / ``MUTATE_B`` (p, t, d), per child: ``u_do = uniform(x0, x1)`` -- the dimension mutates iff ``u_do < p_mut`` --
  and ``u = uniform(x2, x3)``;
* ``INIT`` (i, 0, d): the initial population ``clip(lo + (hi - lo) u)``, ``u = uniform(x0, x1)``.

A draw is a pure function of (seed, t, pair, purpose, dimension): a search continued from a saved state equals the
uninterrupted one bit for bit.  Pair p's children are columns ``p`` and ``N / 2 + p`` of ``child[n_dim, N]``.
"""

import numpy as np

from . import abi
from .pareto import keys, ranks
from .predictive import philox4x32_10, _uniform

STREAM = 0x4E534732          # "NSG2": the counter's fourth word
TOURNAMENT, CROSS, SBX, MUTATE_A, MUTATE_B, INIT = 0, 1, 2, 3, 4, 5     # purpose codes
MAX_DIM, MAX_OBJ = 16, abi.PARETO_MAX_OBJ
MIN_POP, MAX_POP = 4, 65536
ETAS = tuple(2 ** k - 1 for k in range(1, 6))        # 1, 3, 7, 15, 31
_TWO32 = 2.0 ** -32


def k_of_eta(eta, what='eta'):
    """k with eta = 2^k - 1; ValueError naming the allowed values."""
    try:
        ok = float(eta) == int(eta) and int(eta) in ETAS
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("%s must be one of %s (2^k - 1: powers and roots are then squarings and square roots), got %r"
                         % (what, list(ETAS), eta))
    return ETAS.index(int(eta)) + 1


def check_shape(N, n_dim, M=1):
    if not MIN_POP <= int(N) <= MAX_POP or int(N) % 2:
        raise ValueError("the population must be even and in [%d, %d] (got %d)" % (MIN_POP, MAX_POP, N))
    if not 1 <= int(n_dim) <= MAX_DIM:
        raise ValueError("n_dim must be in [1, %d] (got %d)" % (MAX_DIM, n_dim))
    if not 1 <= int(M) <= MAX_OBJ:
        raise ValueError("between 1 and %d objectives (got %d)" % (MAX_OBJ, M))


def check_probability(x, what):
    if not 0.0 <= float(x) <= 1.0:                     # NaN fails
        raise ValueError("%s must be in [0, 1] (got %r)" % (what, x))
    return float(x)


def _key(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32


def _draw(seed, who, t, code, d=0):
    return philox4x32_10((who, int(t) & 0xFFFFFFFF, (code << 8) | d, STREAM), _key(seed))


def _u32(x):
    return (x.astype(np.float64) + 0.5) * _TWO32


# ---- validity, crowding, selection --------------------------------------------------------------------------------------------

def valid_mask(obj, status=None):
    """[n] bool: all objectives finite and the run status without STATUS_NONFINITE."""
    ok = np.isfinite(np.asarray(obj, dtype=np.float64)).all(axis=0)
    if status is not None:
        ok &= (np.asarray(status) & abi.STATUS_NONFINITE) == 0
    return ok


def _values(k):
    """The doubles of order-preserving keys (the inverse of ``pareto.keys`` with sense +1; a zero comes back as +0.0)."""
    k = np.asarray(k, dtype=np.uint64)
    top = np.uint64(1 << 63)
    return np.where((k & top) != 0, k ^ top, ~k).astype(np.uint64).view(np.float64)


def crowding(obj, sense, rank):
    """crowd[n] float64 of members with objectives obj[M, n] and ranks rank[n] (< 0: 0.0)."""
    obj = np.ascontiguousarray(obj, dtype=np.float64)
    rank = np.asarray(rank)
    M, n = obj.shape
    crowd = np.zeros(n, dtype=np.float64)
    for f in np.unique(rank[rank >= 0]):
        ids = np.flatnonzero(rank == f)
        y = _values(keys(obj[:, ids], sense))              # [M, size] sense applied, one zero
        size = ids.size
        edge = np.zeros(size, dtype=bool)
        d = np.zeros(size, dtype=np.float64)
        for m in range(M):
            order = np.lexsort((ids, y[m]))                # by (y, index): ids ascend already, stable in any case
            ys = y[m][order]
            span = ys[-1] - ys[0]
            term = np.zeros(size, dtype=np.float64)
            edge[order[0]] = edge[order[-1]] = True
            if size > 2 and span > 0.0:
                with np.errstate(all='ignore'):
                    term[order[1:-1]] = (ys[2:] - ys[:-2]) / span
            d = d + term
        crowd[ids] = np.where(edge, np.inf, d)
    return crowd


def _order(rank, crowd):
    rank = np.asarray(rank, dtype=np.int64)
    r = np.where(rank < 0, np.int64(1) << 32, rank)
    ck = keys(np.asarray(crowd, dtype=np.float64)[None, :], [1])[0]
    return np.lexsort((np.arange(rank.size), ~ck, r))      # best first


def positions(rank, crowd):
    """position[n] int32: how many members come before each in (rank, -crowding, index)."""
    order = _order(rank, crowd)
    pos = np.empty(order.size, dtype=np.int32)
    pos[order] = np.arange(order.size, dtype=np.int32)
    return pos


def select(N, rank, crowd):
    """(position[n], survivor[N]): survivor[q] is the member at position q."""
    pos = positions(rank, crowd)
    survivor = np.empty(int(N), dtype=np.int32)
    keep = pos < int(N)
    survivor[pos[keep]] = np.flatnonzero(keep)
    return pos, survivor


# ---- mating and variation -----------------------------------------------------------------------------------------------------

def _better(a, b, rank, ck):
    """Of candidates a, b (arrays of indices): the tournament's winner."""
    r = np.where(np.asarray(rank, dtype=np.int64) < 0, np.int64(1) << 32, np.asarray(rank, dtype=np.int64))
    a_wins = (r[a] < r[b]) | ((r[a] == r[b]) & ((ck[a] > ck[b]) | ((ck[a] == ck[b]) & (a <= b))))
    return np.where(a_wins, a, b)


def mating(N, t, rank, crowd, seed=0):
    """parents[2, N/2] int64 of the child pairs of generation t."""
    h = int(N) // 2
    x = _draw(seed, np.arange(h, dtype=np.int64), t, TOURNAMENT)
    c = [((w.astype(np.uint64) * np.uint64(N)) >> np.uint64(32)).astype(np.int64) for w in x]
    ck = keys(np.asarray(crowd, dtype=np.float64)[None, :], [1])[0]
    return np.stack([_better(c[0], c[1], rank, ck), _better(c[2], c[3], rank, ck)])


def powk(x, k):
    """x^(2^k): k squarings."""
    for _ in range(k):
        x = x * x
    return x


def rootk(x, k):
    """x^(1 / 2^k): k nested square roots."""
    for _ in range(k):
        x = np.sqrt(x)
    return x


def _clip(c, lo, hi):
    return np.where(c < lo, lo, np.where(c > hi, hi, c))


def _bq(beta, u, k):
    alpha = 2.0 - 1.0 / powk(beta, k)
    ua = u * alpha
    return np.where(u <= 1.0 / alpha, rootk(ua, k), rootk(1.0 / (2.0 - ua), k))


def sbx(x1, x2, lo, hi, k, cross, u, u_take, u_swap):
    """Bounded SBX of one dimension (every argument broadcasts): the two children."""
    x1, x2, lo, hi, u = (np.asarray(a, dtype=np.float64) for a in (x1, x2, lo, hi, u))
    with np.errstate(all='ignore'):
        y1, y2 = np.minimum(x1, x2), np.maximum(x1, x2)
        dy = y2 - y1
        c1 = 0.5 * ((y1 + y2) - _bq(1.0 + 2.0 * (y1 - lo) / dy, u, k) * dy)
        c2 = 0.5 * ((y1 + y2) + _bq(1.0 + 2.0 * (hi - y2) / dy, u, k) * dy)
    c1, c2 = _clip(c1, lo, hi), _clip(c2, lo, hi)
    swap = np.asarray(u_swap) < 0.5
    a, b = np.where(swap, c2, c1), np.where(swap, c1, c2)
    takes = np.asarray(cross, dtype=bool) & (np.asarray(u_take) < 0.5) & (x1 != x2)
    return np.where(takes, a, x1), np.where(takes, b, x2)


def mutate(c, lo, hi, k, p_mut, u_do, u):
    """Bounded polynomial mutation of one dimension (every argument broadcasts)."""
    c, lo, hi, u = (np.asarray(a, dtype=np.float64) for a in (c, lo, hi, u))
    with np.errstate(all='ignore'):
        w = hi - lo
        low = u <= 0.5
        xy = 1.0 - np.where(low, c - lo, hi - c) / w
        p = powk(xy, k)
        t = 2.0 * u
        val = np.where(low, t + (1.0 - t) * p, 2.0 * (1.0 - u) + (2.0 * (u - 0.5)) * p)
        r = rootk(val, k)
        dq = np.where(low, r - 1.0, 1.0 - r)
        moved = _clip(c + dq * w, lo, hi)
    return np.where(np.asarray(u_do) < p_mut, moved, c)


def vary(x1, x2, lo, hi, k_c, k_m, p_mut, cross, u, u_take, u_swap, u_do_a, u_a, u_do_b, u_b):
    """One dimension of one pair from its uniforms: SBX, then the mutation of either child.  csrc/simplyp_nsga2.h's
    ``vary_dim`` is the same function."""
    a, b = sbx(x1, x2, lo, hi, k_c, cross, u, u_take, u_swap)
    return mutate(a, lo, hi, k_m, p_mut, u_do_a, u_a), mutate(b, lo, hi, k_m, p_mut, u_do_b, u_b)


def offspring(theta, rank, crowd, t, lo, hi, eta_c=15, eta_m=15, p_cross=0.9, p_mut=None, seed=0):
    """The children of generation t: dict(child[n_dim, N], parents[2, N] -- the two parents of every child column)."""
    theta = np.asarray(theta, dtype=np.float64)
    n_dim, N = theta.shape
    check_shape(N, n_dim)
    k_c, k_m = k_of_eta(eta_c, 'eta_c'), k_of_eta(eta_m, 'eta_m')
    p_cross = check_probability(p_cross, 'p_cross')
    p_mut = check_probability(1.0 / n_dim if p_mut is None else p_mut, 'p_mut')
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    if lo.shape != (n_dim,) or hi.shape != (n_dim,) or not (lo < hi).all():
        raise ValueError("the box needs lo < hi in every dimension")
    h = N // 2
    p = np.arange(h, dtype=np.int64)
    par = mating(N, t, rank, crowd, seed)
    x0, x1, _, _ = _draw(seed, p, t, CROSS)
    cross = _uniform(x0, x1) < p_cross
    child = np.empty((n_dim, N), dtype=np.float64)
    for d in range(n_dim):
        s = _draw(seed, p, t, SBX, d)
        ma, mb = _draw(seed, p, t, MUTATE_A, d), _draw(seed, p, t, MUTATE_B, d)
        a, b = vary(theta[d, par[0]], theta[d, par[1]], lo[d], hi[d], k_c, k_m, p_mut, cross,
                    _uniform(s[0], s[1]), _u32(s[2]), _u32(s[3]),
                    _uniform(ma[0], ma[1]), _uniform(ma[2], ma[3]), _uniform(mb[0], mb[1]), _uniform(mb[2], mb[3]))
        child[d, :h], child[d, h:] = a, b
    return dict(child=child, parents=np.concatenate([par, par], axis=1).astype(np.int32), crossed=cross)


def initial_population(N, lo, hi, seed=0):
    """theta[n_dim, N] = clip(lo + (hi - lo) u) from the INIT draws."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    n_dim = lo.size
    check_shape(N, n_dim)
    i = np.arange(int(N), dtype=np.int64)
    theta = np.empty((n_dim, int(N)), dtype=np.float64)
    for d in range(n_dim):
        x0, x1, _, _ = _draw(seed, i, 0, INIT, d)
        theta[d] = _clip(lo[d] + (hi[d] - lo[d]) * _uniform(x0, x1), lo[d], hi[d])
    return theta


# ---- the loop -----------------------------------------------------------------------------------------------------------------

def rank_and_crowd(obj, sense, valid=None):
    """(rank[n] int32 with -1 for the invalid, crowd[n], the dict of ``pareto.ranks``)."""
    obj = np.asarray(obj, dtype=np.float64)
    valid = valid_mask(obj) if valid is None else np.asarray(valid, dtype=bool)
    got = ranks(obj, sense, include=valid)
    return got['rank'], crowding(obj, sense, got['rank']), got


def survive(N, theta, obj, sense, valid=None):
    """Environmental selection of a set theta[n_dim, n], obj[M, n], N <= n: dict(theta[n_dim, N], obj[M, N], rank[N],
    crowd[N], survivor[N], position[n], n_fronts, n_front0, n_invalid), best first."""
    rank, crowd, got = rank_and_crowd(obj, sense, valid)
    pos, sv = select(N, rank, crowd)
    return dict(theta=np.asarray(theta)[:, sv], obj=np.asarray(obj)[:, sv], rank=rank[sv], crowd=crowd[sv], survivor=sv,
                position=pos, all_rank=rank, all_crowd=crowd, n_fronts=got['n_fronts'], n_front0=got['n_front0'],
                n_invalid=int(rank.size - got['n_used']))


def new_state(theta, obj, sense, valid=None):
    """Generation 0: the evaluated initial population sorted best first, t = 0."""
    N = np.asarray(theta).shape[1]
    s = survive(N, theta, obj, sense, valid)
    return dict(theta=s['theta'], obj=s['obj'], rank=s['rank'], crowd=s['crowd'], t=0), s


def step(state, evaluate, sense, lo, hi, eta_c=15, eta_m=15, p_cross=0.9, p_mut=None, seed=0):
    """One generation from ``state`` (not modified): ``evaluate(child[n_dim, N]) -> obj[M, N]`` or ``(obj, valid[N])``.
    Returns (the new state, dict(child, child_obj, parents, and what ``survive`` returns for the 2N set))."""
    t = int(state['t']) + 1
    N = state['theta'].shape[1]
    off = offspring(state['theta'], state['rank'], state['crowd'], t, lo, hi, eta_c, eta_m, p_cross, p_mut, seed)
    got = evaluate(off['child'])
    child_obj, child_valid = got if isinstance(got, tuple) else (got, None)
    child_obj = np.asarray(child_obj, dtype=np.float64)
    obj = np.concatenate([state['obj'], child_obj], axis=1)
    valid = valid_mask(obj)
    if child_valid is not None:
        valid[N:] &= np.asarray(child_valid, dtype=bool)
    valid[:N] &= state['rank'] >= 0
    s = survive(N, np.concatenate([state['theta'], off['child']], axis=1), obj, sense, valid)
    new = dict(theta=s['theta'], obj=s['obj'], rank=s['rank'], crowd=s['crowd'], t=t)
    return new, dict(s, child=off['child'], child_obj=child_obj, parents=off['parents'])


def run(evaluate, N, n_gen, sense, lo, hi, eta_c=15, eta_m=15, p_cross=0.9, p_mut=None, seed=0, start=None, state=None):
    """The whole search: ``n_gen`` generations after the initial population's (or from ``state``).  Returns (state, the list of
    every generation's record)."""
    records = []
    if state is None:
        theta0 = initial_population(N, lo, hi, seed) if start is None else np.array(start, dtype=np.float64)
        got = evaluate(theta0)
        obj0, valid0 = got if isinstance(got, tuple) else (got, None)
        obj0 = np.asarray(obj0, dtype=np.float64)
        valid = valid_mask(obj0) & (True if valid0 is None else np.asarray(valid0, dtype=bool))
        state, rec = new_state(theta0, obj0, sense, valid)
        records.append(dict(rec, child=theta0, child_obj=obj0))
    for _ in range(int(n_gen)):
        state, rec = step(state, evaluate, sense, lo, hi, eta_c, eta_m, p_cross, p_mut, seed)
        records.append(rec)
    return state, records
