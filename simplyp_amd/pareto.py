"""Pareto dominance among the members of an ensemble: the rule ``simplyp_pareto`` computes on the device, stated in NumPy and
Python integers (``ranks``), the objectives a goodness-of-fit table offers (``resolve_objectives``, ``objective_rows``), and the
public call on such a table (``pareto_ranks``).  ``simplyp_amd/csrc/simplyp_pareto.h`` states the same rule in plain C++.

The rule.  ``obj[M, E]`` holds M objectives of E members, ``sense[m]`` is +1 (larger is better) or -1 (smaller is better).
A member takes part iff its include flag is set and none of its objectives is NaN; +-inf are ordinary values, -0.0 and +0.0
are equal.  With y = sense x, a dominates b iff y_a >= y_b in every objective and y_a > y_b in some; members with identical
objectives do not dominate each other.  ``dominated_by[i]`` counts the participants that dominate i, ``dominates[i]`` those i
dominates, ``rank[i]`` is 0 when nobody dominates i and otherwise 1 + the largest rank among its dominators -- the longest chain
of dominators above i, which is the index of the front i leaves with when the non-dominated members are peeled off one front
at a time (NSGA-II's non-dominated rank).  ``ranks`` computes the rank both ways and asserts that they agree.  Members that do
not take part get ``EXCLUDED`` (-1) everywhere; with ``max_fronts = F > 0`` a participant of rank >= F gets ``UNRANKED`` (-2)
as its rank and keeps its exact counts.  Only comparisons and integer counts: every correct implementation gives these integers.
"""

import struct

import numpy as np

from . import abi

EXCLUDED = abi.PARETO_EXCLUDED
UNRANKED = abi.PARETO_UNRANKED
MAX_OBJ = abi.PARETO_MAX_OBJ
_SIGN = 1 << 63
_ALL = (1 << 64) - 1


def key(x, sense):
    """The order-preserving 64-bit key of y = sense x as a Python integer: ``simplyp_quantiles``' key with the sense folded in
    and the two zeros made one.  x must not be NaN."""
    x = float(x)
    if x != x:
        raise ValueError("a NaN has no key: the member takes no part")
    b = struct.unpack('<Q', struct.pack('<d', x))[0]
    if sense < 0:
        b ^= _SIGN
    if b == _SIGN:
        b = 0
    return (~b & _ALL) if b >> 63 else (b | _SIGN)


def keys(obj, sense):
    """``key`` of every element of obj [M, n] (no NaN) under sense [M], as uint64."""
    b = np.ascontiguousarray(obj, dtype=np.float64).view(np.uint64).copy()
    flip = np.where(np.asarray(sense).reshape(-1, 1) < 0, np.uint64(_SIGN), np.uint64(0))
    b ^= flip
    b[b == np.uint64(_SIGN)] = 0
    return np.where((b >> np.uint64(63)) != 0, ~b, b | np.uint64(_SIGN))


def _check(obj, sense, include, max_fronts):
    obj = np.asarray(obj, dtype=np.float64)
    if obj.ndim != 2 or not 1 <= obj.shape[0] <= MAX_OBJ or obj.shape[1] < 1:
        raise ValueError("obj must be [M, E] with 1 <= M <= %d and E >= 1" % MAX_OBJ)
    sense = [int(s) for s in np.atleast_1d(np.asarray(sense))]
    if len(sense) != obj.shape[0] or any(s not in (1, -1) for s in sense):
        raise ValueError("sense must hold one +1 or -1 per objective")
    max_fronts = int(max_fronts)
    if max_fronts < 0:
        raise ValueError("max_fronts must be >= 0")
    take = ~np.isnan(obj).any(axis=0)
    if include is not None:
        inc = np.asarray(include)
        if inc.shape != (obj.shape[1],):
            raise ValueError("include must have one entry per member")
        take &= inc != 0
    return obj, sense, take, max_fronts


def _dominators(rows, cols):
    """D[r, c]: does column member c dominate row member r?  And the mirror.  rows [M, a], cols [M, b]: dense ranks."""
    ge = np.ones((rows.shape[1], cols.shape[1]), dtype=bool)
    le = np.ones_like(ge)
    for m in range(rows.shape[0]):
        ge &= cols[m][None, :] >= rows[m][:, None]
        le &= cols[m][None, :] <= rows[m][:, None]
    return ge & ~le, le & ~ge


def ranks(obj, sense, include=None, max_fronts=0, block=256):
    """The rule on the host, in row blocks of ``block`` members (no E x E array).  obj [M, E] in member order.
    Returns dict(dominated_by, dominates, rank: int32 [E]; n_used, n_fronts, n_front0, n_unranked, pair_tests: Python ints)."""
    obj, sense, take, F = _check(obj, sense, include, max_fronts)
    E = obj.shape[1]
    ids = np.flatnonzero(take)
    n = int(ids.size)
    out = {k: np.full(E, EXCLUDED, dtype=np.int32) for k in ('dominated_by', 'dominates', 'rank')}
    if n == 0:
        return dict(out, n_used=0, n_fronts=0, n_front0=0, n_unranked=0, pair_tests=0)
    K = keys(obj[:, ids], sense)
    # dominance is invariant under a strictly increasing map of an objective: dense ranks of the keys, in the narrowest type
    dt = np.uint16 if n <= 1 << 16 else np.uint32
    R = np.stack([np.unique(K[m], return_inverse=True)[1].reshape(-1).astype(dt) for m in range(K.shape[0])])
    # a dominator has a strictly larger sum of dense ranks: in descending order of the sum every dominator comes first
    order = np.argsort(-R.sum(axis=0, dtype=np.int64), kind='stable')
    R = np.ascontiguousarray(R[:, order])
    by = np.zeros(n, dtype=np.int64)
    of = np.zeros(n, dtype=np.int64)
    chain = np.full(n, -1, dtype=np.int32)                     # the longest chain of dominators, by the recurrence
    for lo in range(0, n, block):
        hi = min(n, lo + block)
        D, O = _dominators(R[:, lo:hi], R)
        by[lo:hi] = D.sum(axis=1)
        of[lo:hi] = O.sum(axis=1)
        inner = D[:, lo:hi]
        assert not D[:, hi:].any() and not np.triu(inner).any()
        ext = np.where(D[:, :lo], chain[None, :lo], -1).max(axis=1) if lo else np.full(hi - lo, -1)
        for t in range(hi - lo):
            best = int(ext[t])
            mine = chain[lo:lo + t][inner[t, :t]]
            if mine.size:
                best = max(best, int(mine.max()))
            chain[lo + t] = best + 1
    # the same rank by peeling: the members nobody left dominates leave, and are taken off the counts of the others
    left = by.copy()
    rank = np.full(n, UNRANKED, dtype=np.int32)
    alive = np.arange(n)
    n_fronts = n_front0 = 0
    pair_tests = n * n
    while alive.size and (F == 0 or n_fronts < F):
        gone = left[alive] == 0
        front, rest = alive[gone], alive[~gone]
        assert front.size > 0
        rank[front] = n_fronts
        if n_fronts == 0:
            n_front0 = int(front.size)
        n_fronts += 1
        if rest.size and (F == 0 or n_fronts < F):
            pair_tests += int(front.size) * int(rest.size)
            step = max(1, (1 << 22) // int(front.size))
            for a in range(0, rest.size, step):
                part = rest[a:a + step]
                left[part] -= _dominators(R[:, part], R[:, front])[0].sum(axis=1)
        alive = rest
    assert (left[rank >= 0] == 0).all() and (left >= 0).all()
    assert np.array_equal(rank, np.where((chain < F) | (F == 0), chain, UNRANKED)), "peeling and the longest chain disagree"
    where = ids[order]
    out['dominated_by'][where] = by
    out['dominates'][where] = of
    out['rank'][where] = rank
    return dict(out, n_used=n, n_fronts=n_fronts, n_front0=n_front0, n_unranked=int(alive.size), pair_tests=int(pair_tests))


# ---- the objectives of a goodness-of-fit table -------------------------------------------------------------------------------
# what a statistic is optimised towards: +1 larger is better, -1 smaller is better, 'abs' the absolute value is minimised,
# None: no direction of its own (a count, the sums a likelihood is made of) -- the caller must name one
DEFAULT_SENSE = {'N obs': None, 'NSE': 1, 'log NSE': 1, 'r2': 1, 'Bias (%)': 'abs', 'nRMSD (%)': -1, 'sum_log_sim': None,
                 'sum_relsq': None, 'spearman': 1}


def resolve_objectives(objectives, n_reaches=1, has_spearman=False, stats=None, variables=None):
    """The objectives as rows of a goodness-of-fit table.  Each is ``(stat, variable)``, ``(stat, variable, reach_index)`` or
    ``(stat, variable, reach_index, sense)``: stat a name of ``abi.GOF_STATS`` or ``'spearman'`` (when the table holds it),
    variable a name of ``abi.GOF_VARS``, reach_index the position among the table's reaches (default 0), sense +1 or -1.
    Without a sense: NSE, log NSE, r2 and Spearman's r are maximised, nRMSD (%) is minimised, Bias (%) is minimised in absolute
    value; 'N obs' and the two likelihood sums have no direction and are refused.  With a sense the statistic is taken as it is.
    Returns a list of dict(stat, variable, reach, stat_index (None: Spearman), var_index, sense, absolute, label)."""
    stats = list(abi.GOF_STATS if stats is None else stats)
    variables = list(abi.GOF_VARS if variables is None else variables)
    try:
        objectives = [tuple(o) for o in objectives]
    except TypeError:
        raise ValueError("objectives must be a list of (stat, variable[, reach_index[, sense]])")
    if not 1 <= len(objectives) <= MAX_OBJ:
        raise ValueError("between 1 and %d objectives, got %d" % (MAX_OBJ, len(objectives)))
    res = []
    for o in objectives:
        if not 2 <= len(o) <= 4:
            raise ValueError("an objective is (stat, variable[, reach_index[, sense]]), got %r" % (o,))
        stat, var = o[0], o[1]
        reach = int(o[2]) if len(o) > 2 and o[2] is not None else 0
        if stat == 'spearman':
            if not has_spearman:
                raise ValueError("objective %r: the table holds no Spearman's r (run with spearman=True)" % (o,))
        elif stat not in stats:
            raise ValueError("objective %r: the statistic must be one of %s or 'spearman'" % (o, stats))
        if var not in variables:
            raise ValueError("objective %r: the variable must be one of %s" % (o, variables))
        if not 0 <= reach < n_reaches:
            raise ValueError("objective %r: reach_index must be in [0, %d)" % (o, n_reaches))
        absolute = False
        if len(o) == 4:
            if o[3] not in (1, -1):
                raise ValueError("objective %r: the sense must be +1 or -1" % (o,))
            sense = int(o[3])
        else:
            default = DEFAULT_SENSE[stat]
            if default is None:
                raise ValueError("objective %r: %r has no direction of its own -- give the sense as a fourth element" % (o, stat))
            absolute = default == 'abs'
            sense = -1 if absolute else default
        label = ('|%s|' if absolute else '%s') % stat + '(%s)' % var + ('' if n_reaches == 1 else '[%d]' % reach)
        res.append(dict(stat=stat, variable=var, reach=reach, stat_index=None if stat == 'spearman' else stats.index(stat),
                        var_index=variables.index(var), sense=sense, absolute=absolute, label=label))
    return res


def objective_rows(data, spearman, resolved):
    """[M, E] float64: the resolved objectives' rows of the table ``data`` [n_stats, n_vars, n_reaches, E] (and ``spearman``
    [n_vars, n_reaches, E]), the absolute value taken where an objective asks for it -- torch on the table's device."""
    import torch
    rows = []
    for r in resolved:
        row = spearman[r['var_index'], r['reach']] if r['stat_index'] is None else data[r['stat_index'], r['var_index'], r['reach']]
        rows.append(row.abs() if r['absolute'] else row)
    return torch.stack(rows).contiguous()


def result(got, resolved):
    """``Engine.pareto``'s dict as the public result: numpy arrays and the front's member ids."""
    info = {k: got[k] for k in ('kernel_ms', 'pair_tests', 'n_used', 'n_fronts', 'n_front0', 'n_unranked')}
    rank = got['rank'].cpu().numpy()
    return dict(rank=rank, dominated_by=got['dominated_by'].cpu().numpy(), dominates=got['dominates'].cpu().numpy(),
                front=np.flatnonzero(rank == 0), objectives=[r['label'] for r in resolved], sense=[r['sense'] for r in resolved],
                n_members=int(info['n_used']), n_fronts=int(info['n_fronts']), info=info)


def pareto_ranks(gof, objectives, members=None, max_fronts=0, device=0):
    """Pareto ranks of the members of an ensemble on several goodness-of-fit criteria at once, sorted on the device.

    gof: the dict ``run_simply_p_ensemble(..., obs_dict=...)`` returns under ``'gof'`` (its ``data`` a host array or a device
    tensor); objectives: see ``resolve_objectives``; members: optional mask [E] of the members that take part; max_fronts: 0
    resolves every rank, F > 0 the ranks below F.  A member with a NaN objective takes no part.
    Returns dict(rank, dominated_by, dominates: int32 [E], -1 for a member that takes no part, rank -2 beyond ``max_fronts``;
    front: the member ids of rank 0; objectives, sense, n_members, n_fronts, info)."""
    from . import engine
    import torch
    eng = engine.get_engine(device)
    data = gof['data']
    if not torch.is_tensor(data):
        data = np.asarray(data, dtype=np.float64)
    if data.ndim != 4:
        raise ValueError("gof['data'] must be [n_stats, n_vars, n_reaches, E]")
    rho = gof.get('spearman')
    resolved = resolve_objectives(objectives, n_reaches=int(data.shape[2]), has_spearman=rho is not None,
                                  stats=gof.get('stats'), variables=gof.get('variables'))
    data = eng.to_device(data, torch.float64)
    rho = None if rho is None else eng.to_device(rho, torch.float64)
    E = int(data.shape[3])
    if members is not None and np.asarray(members.cpu() if torch.is_tensor(members) else members).shape != (E,):
        raise ValueError("members must be a mask with one entry per member")
    got = eng.pareto(objective_rows(data, rho, resolved), [r['sense'] for r in resolved], include=members, max_fronts=max_fronts)
    return result(got, resolved)
