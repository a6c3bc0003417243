"""What the NSGA-II tests share: an independent statement of crowding and positions (per front, np.lexsort and Python loops --
nothing of simplyp_amd.nsga2), the planted tables, ZDT1, and the comparison of doubles by their bits."""

import numpy as np

from simplyp_amd import nsga2


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(got, want, what=''):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(bits(got).reshape(-1) != bits(want).reshape(-1))
    assert bad.size == 0, (what, bad[:5], got.reshape(-1)[bad[:5]], want.reshape(-1)[bad[:5]])


def crowding_by_sorting(obj, sense, rank):
    """Deb's crowding distance front by front: sort by (y, index), infinite at either end of any objective, else the sum over
    the objectives, in their order and from 0, of (next - prev) / (max - min) where the front's span is positive."""
    obj = np.asarray(obj, dtype=np.float64)
    M, n = obj.shape
    y = obj * np.asarray(sense, dtype=np.float64)[:, None] + 0.0        # -0.0 + 0.0 = +0.0: the two zeros tie
    crowd = np.zeros(n)
    for f in sorted(set(int(r) for r in rank if r >= 0)):
        ids = np.flatnonzero(np.asarray(rank) == f)
        d = {int(i): 0.0 for i in ids}
        for m in range(M):
            order = ids[np.lexsort((ids, y[m, ids]))]
            span = y[m, order[-1]] - y[m, order[0]]
            d[int(order[0])] = d[int(order[-1])] = np.inf
            for q in range(1, len(order) - 1):
                if span > 0.0:
                    d[int(order[q])] = d[int(order[q])] + (y[m, order[q + 1]] - y[m, order[q - 1]]) / span
        for i, v in d.items():
            crowd[i] = v
    return crowd


def positions_by_sorting(rank, crowd):
    rank = np.asarray(rank, dtype=np.int64)
    order = np.lexsort((np.arange(rank.size), -(np.asarray(crowd) + 0.0), np.where(rank < 0, rank.max() + 1, rank)))
    pos = np.empty(rank.size, dtype=np.int64)
    pos[order] = np.arange(rank.size)
    return pos


def ranked(obj, sense, valid=None):
    """(rank with -1 for the invalid, the valid mask) by simplyp_amd.pareto's statement."""
    rank, _, _ = nsga2.rank_and_crowd(obj, sense, valid)
    return rank.astype(np.int32), (nsga2.valid_mask(obj) if valid is None else np.asarray(valid, dtype=bool))


def planted(rng, n, M):
    """[(name, obj [M, n], sense [M], rank [n] int32)]: every kind of table the rule distinguishes, n even."""
    out = []
    plus = [1] * M
    mixed = [(-1) ** m for m in range(M)]
    normals = rng.standard_normal((M, n))
    out.append(('normals', normals, plus))
    out.append(('sense -1', normals.copy(), [-1] * M))
    out.append(('mixed sense', rng.standard_normal((M, n)), mixed))
    out.append(('ties', rng.integers(0, 4, (M, n)).astype(np.float64), mixed))
    half = rng.standard_normal((M, n // 2))
    out.append(('duplicates', np.concatenate([half, half], axis=1), plus))
    out.append(('zeros', rng.choice([0.0, -0.0, 1.0, -1.0, 5e-324, -5e-324], (M, n)), mixed))
    const = rng.standard_normal((M, n))
    const[M - 1] = 3.0
    out.append(('a constant objective', const, plus))
    bad = rng.standard_normal((M, n))
    where = rng.choice(n, max(1, n // 4), replace=False)
    bad[rng.integers(0, M, where.size), where] = rng.choice([np.nan, np.inf, -np.inf], where.size)
    out.append(('invalid members', bad, mixed))
    most = rng.standard_normal((M, n))
    most[0, rng.choice(n, n // 2 + 1, replace=False)] = np.nan
    out.append(('more invalid than half', most, plus))
    cases = [(name, obj, np.array(sense, dtype=np.int32), ranked(obj, sense)[0]) for name, obj, sense in out]
    # ranks that no dominance gave: fronts of one and of two members beside a large one, and members left out
    by_hand = np.zeros(n, dtype=np.int32)
    by_hand[:min(n, 3)] = [1, 2, 2][:min(n, 3)]
    if n > 6:
        by_hand[n - 2:] = -1
    cases.append(('fronts of one and two', rng.integers(0, 6, (M, n)).astype(np.float64), np.array(plus, dtype=np.int32), by_hand))
    return cases


def zdt1(x):
    """(objectives [2, N] -- both minimised --, g [N]) of positions x [n_dim, N] in [0, 1]."""
    x = np.asarray(x, dtype=np.float64)
    g = 1.0 + 9.0 * x[1:].sum(axis=0) / (x.shape[0] - 1)
    return np.stack([x[0], g * (1.0 - np.sqrt(x[0] / g))]), g
