"""Rows and tables built to hit the limits of the two radix selects, shared by tests/test_selection_model_host.py (the model
against np.sort, on the CPU) and the device tests (the kernels against the model and np.sort).

The first key digit is the sign and the upper seven exponent bits, so three ranges of values fall into three first-digit
buckets: FILL = [0.5, 1) (digit 0xBF), TOP = [2, 4) (0xC0) and FAR = [2^20, 2^21) (0xC1).  The second digit is the lower four
exponent bits and the upper four mantissa bits: 'spread' values fill a range evenly and meet 16 second digits, 'narrow' ones
stay in its lowest sixteenth ([2, 2.125)), share the second digit and part in the third."""

import numpy as np

from selection_model import LANES, QLIST, WQLIST

E_SELECT, E_WSELECT = 4097, 2049       # the shortest rows that reach the two member-axis selects


def ramp(lo, n, narrow=False):
    """n distinct values evenly inside [lo, 2 lo), or inside its lowest sixteenth."""
    return lo * (1.0 + (np.arange(n) + 0.5) / (n * (16 if narrow else 1)))


def limit_row(E, top_cols, far_cols=(), narrow=False, rng=None):
    """A row [E]: TOP values in the columns top_cols, FAR values in far_cols, FILL values everywhere else, each in a
    shuffled order."""
    row = np.empty(E)
    top_cols, far_cols = np.asarray(top_cols, dtype=np.int64), np.asarray(far_cols, dtype=np.int64)
    rest = np.setdiff1d(np.arange(E), np.concatenate([top_cols, far_cols]))
    assert len(rest) + len(top_cols) + len(far_cols) == E
    row[rng.permutation(top_cols)] = ramp(2.0, len(top_cols), narrow)
    row[rng.permutation(far_cols)] = ramp(2.0 ** 20, len(far_cols))
    row[rng.permutation(rest)] = ramp(0.5, len(rest))
    return row


# ---- member axis, unweighted: (name, n_top, n_far, narrow, probabilities, sweeps) -----------------------------------------------
# E = 4097, so rank k is probability k / 4096 exactly; the TOP values hold the ranks [E - n_far - n_top, E - n_far), the FAR
# values those above.  Sweeps, by hand (LIST = 64):
#   top64          digit 1: the wanted bucket holds 64 <= LIST -> collect.                                         2
#   top65 spread   digit 1: 65 > LIST; digit 2: 16 bins of 4 or 5 -> collect.                                      3
#   top65 narrow   digit 1: 65; digit 2: all 65 share the bin; digit 3: one value per bin -> collect.              4
#   two groups     TOP holds 64, FAR 65.  Ranks in TOP alone: 2, as top64.  A rank in FAR as well: after digit 1 the groups
#                  hold 64 and 65, the collect waits for the larger; digit 2 parts FAR's 65 -> collect.              3
def _p(E, *ranks):
    return [k / (E - 1) for k in ranks]


def member_cases(E=E_SELECT, L=QLIST):
    return [
        ('top LIST', L, 0, False, _p(E, E - L, E - L // 2) + [1.0], 2),
        ('top LIST + 1, spread', L + 1, 0, False, _p(E, E - L - 1, E - L // 2) + [1.0], 3),
        ('top LIST + 1, narrow', L + 1, 0, True, _p(E, E - L - 1, E - L // 2) + [1.0], 4),
        ('two groups, ranks in the small one', L, L + 1, False, _p(E, E - 2 * L - 1, E - L - 3), 2),
        ('two groups, ranks in both', L, L + 1, False, _p(E, E - 2 * L - 1, E - L - 2) + [1.0], 3),
    ]


def member_table(case, n_rows, rng, E=E_SELECT):
    """[n_rows, E]: every row the case's values in columns of its own."""
    _, n_top, n_far, narrow, _, _ = case
    rows = []
    for _ in range(n_rows):
        cols = rng.permutation(E)
        rows.append(limit_row(E, cols[:n_top], cols[n_top:n_top + n_far], narrow, rng))
    return np.stack(rows)


# ---- member axis, weighted: (name, n_top, n_top_zero, n_far, narrow, sweeps) ----------------------------------------------------
# A member with weight 0 takes no part and does not count towards LIST = 32: a bucket of 33 members one of which has weight 0
# is a bucket of 32.  Sweeps as above with 32 for 64.
def weighted_cases(L=WQLIST):
    return [
        ('top LIST', L, 0, 0, False, 2),
        ('top LIST + 1, spread', L + 1, 0, 0, False, 3),
        ('top LIST + 1, narrow', L + 1, 0, 0, True, 4),
        ('top LIST and one member of weight 0', L, 1, 0, False, 2),
        ('two groups, thresholds in the small one', L, 0, L + 1, False, 2),
        ('two groups, thresholds in both', L, 0, L + 1, False, 3),
    ]


def weighted_table(case, q, n_rows, rng):
    """([n_rows, E], probabilities): the case's TOP and FAR values in columns that carry a weight (n_top_zero TOP values in
    columns that carry none), the same columns in every row; probabilities whose thresholds fall among the TOP values' running
    weights -- and, in the case that names both, among the FAR values' too."""
    name, n_top, n_zero, n_far, narrow, _ = case
    E = len(q)
    with_w, without = rng.permutation(np.flatnonzero(q > 0)), rng.permutation(np.flatnonzero(q == 0))
    top, far = with_w[:n_top], with_w[n_top:n_top + n_far]
    rows = np.stack([limit_row(E, np.concatenate([top, without[:n_zero]]), far, narrow, rng) for _ in range(n_rows)])
    T = sum(int(v) for v in q)
    w_top, w_far = sum(int(v) for v in q[top]), sum(int(v) for v in q[far])
    # the TOP values' running weights are (T - w_far - w_top, T - w_far]: aim well inside, away from the float rounding of p T
    probs = [(T - w_far - f * w_top) / T for f in (0.9, 0.5, 0.1)]
    if 'both' in name or n_far == 0:
        probs.append(1.0)
    return rows, probs, (T, w_top, w_far)


# ---- the six base rows of the tables that run past the select's grid cap ---------------------------------------------------------
BASE_KINDS = ('normals', 'ties', 'equal', 'special', 'top LIST', 'top LIST + 1')


def base_rows(E, L, rng, weights=None):
    """[6, E]: distinct normals, heavy ties, all equal, specials without denormals (they would not scale exactly), and the
    two limit rows (their TOP values in columns with a weight where weights are given)."""
    special = rng.normal(size=E)
    hit = rng.random(E) < 0.3
    special[hit] = rng.choice(np.array([np.inf, -np.inf, -0.0, 0.0, np.nan, -np.nan, 1e300, -1e300]), size=int(hit.sum()))
    cols = rng.permutation(E if weights is None else np.flatnonzero(weights > 0))
    return np.stack([rng.normal(size=E), rng.choice(np.array([-3.5, -0.0, 0.0, 1.25, 7.25e11]), size=E), np.full(E, 3.25), special,
                     limit_row(E, cols[:L], (), False, rng), limit_row(E, cols[:L + 1], (), False, rng)])


def capped_rows(n_first, B, rng):
    """(kind_of_row, scale_of_row) of n_first + B^2 rows: a workgroup of an n_first-wide grid selects row i < B^2 and then row
    n_first + i, kinds i % B and (i // B) % B -- every ordered pair of kinds --, each row scaled by a power of two."""
    n = n_first + B * B
    kind = rng.integers(0, B, n)
    i = np.arange(B * B)
    kind[i] = i % B
    kind[n_first + i] = (i // B) % B
    return kind, 2.0 ** rng.integers(-8, 9, n)


# ---- day axis ------------------------------------------------------------------------------------------------------------------
KINDS = ('smooth', 'equal', 'two', 'lastbits', 'special')


def time_table(kind, shape, rng):
    """[n_cols, D, R, E] of one kind."""
    if kind == 'smooth':                                                   # positive, within a few binades, day-to-day smooth
        t = np.exp(np.cumsum(rng.normal(scale=0.05, size=shape), axis=1) + rng.normal(size=(shape[0], 1) + shape[2:]))
        return t
    if kind == 'equal':
        return np.full(shape, rng.normal())
    if kind == 'two':
        return rng.choice(np.array([1.5, -2.25]), size=shape)
    if kind == 'lastbits':                                                 # differ in the last bits only
        base = np.float64(0.7310585786300049)
        return (np.full(shape, base).view(np.int64) + rng.integers(0, 7, size=shape)).view(np.float64)
    assert kind == 'special'                                               # mixed sign, +-0, +-inf, denormals, a few NaN
    t = rng.normal(size=shape) * 10.0 ** rng.integers(-3, 4, size=(shape[0], 1) + shape[2:])
    specials = np.array([np.inf, -np.inf, 5e-324, -5e-324, 1e-310, -1e-310, -0.0, 0.0, 0.0, -0.0, np.nan, -np.nan,
                         np.finfo(np.float64).max, -np.finfo(np.float64).max])
    hit = rng.random(size=shape) < 0.3
    t[hit] = rng.choice(specials, size=int(hit.sum()))
    return t


def lead_bucket_table(shape, n_far, rng, odd_lane=None):
    """[n_cols, D, R, E] in which every member's D days are 64 TOP values, n_far FAR values and FILL values for the rest, in a
    shuffled order of its own; odd_lane = (member, n_far) gives one member another number of FAR values.  With ranks among the
    TOP and the FAR values a lane has two groups after the first digit, whose buckets hold 64 + n_far keys together."""
    n_cols, D, R, E = shape
    t = np.empty(shape)
    for c in range(n_cols):
        for r in range(R):
            for e in range(E):
                far = odd_lane[1] if odd_lane is not None and e == odd_lane[0] else n_far
                days = rng.permutation(D)
                t[c, :, r, e] = limit_row(D, days[:64], days[64:64 + far], False, rng)
    return t


def mixed_table(shape, rng):
    """Member e of kind KINDS[e % 5]: every wave holds lanes that settle after two digits beside lanes that need all eight."""
    per_kind = [time_table(kind, shape, rng) for kind in KINDS]
    t = np.empty(shape)
    for e in range(shape[3]):
        t[..., e] = per_kind[e % 5][..., e]
    return t


def lone_lanes_table(shape, rng):
    """Every member smooth, but one 'equal' lane in the first wave and one 'lastbits' lane in the last, partial one."""
    t = time_table('smooth', shape, rng)
    E = shape[3]
    a, b = 17, E - 1
    assert a < LANES and b >= (E // LANES) * LANES and E % LANES
    t[..., a] = time_table('equal', shape[:3] + (1,), rng)[..., 0]
    t[..., b] = time_table('lastbits', shape[:3] + (1,), rng)[..., 0]
    return t


def periods_130_1_200(D):
    """period_of_day: four periods of 130, 1, 200 days and the rest (D = 300: 130, 1, 169 and none)."""
    cuts = np.minimum(np.cumsum([0, 130, 1, 200]), D)
    return np.repeat(np.arange(4), np.diff(np.append(cuts, D)))


def capped_periods(n_first, n_second=70):
    """The periods of a call whose period axis runs past a grid of n_first: (kind_of_period, days_of_period) for
    n_first + n_second periods.  A workgroup takes period y and then n_first + y.  First trip: 0-31 200 days 'smooth', 32-63
    200 days 'two' (all 8 digits), 64 empty, the others one day.  Second trip j = 0 ...: every fourth 129-300 days of the kinds
    in turn (long after long), 33 empty (full, then empty), 64 long (empty, then full), 65-69 long of each kind (short, then
    long), the others one day (long, then short)."""
    kind, n = [], []
    for p in range(n_first):
        kind.append('smooth' if p < 32 else 'two' if p < 64 else 'smooth')
        n.append(200 if p < 64 else 0 if p == 64 else 1)
    for j in range(n_second):
        long_n = 129 + (j * 37) % 172
        if j == 33:
            kind.append('smooth'); n.append(0)
        elif j == 64:
            kind.append('smooth'); n.append(250)
        elif 65 <= j < 70:
            kind.append(KINDS[j - 65]); n.append(long_n)
        elif j % 4 == 0:
            kind.append(KINDS[(j // 4) % 5]); n.append(long_n)
        else:
            kind.append('smooth'); n.append(1)
    return kind, np.asarray(n, dtype=np.int64)


def sorted_periods(x, q, period_of_day, n_periods):
    """np.sort's view of x [n_series, D, R, E] for many periods: lower, upper [K, n_series, P, R, E] and n_days [P].  What
    tests/test_gpu_time_quantiles.py::expected computes, with the one-day periods taken all at once."""
    pod = np.asarray(period_of_day)
    order = np.flatnonzero(pod >= 0)
    bounds = np.searchsorted(pod[order], np.arange(n_periods + 1))
    n_days = np.diff(bounds)
    lo = np.full((len(q), x.shape[0], n_periods) + x.shape[2:], np.nan)
    hi = lo.copy()
    one = np.flatnonzero(n_days == 1)
    lo[:, :, one] = hi[:, :, one] = x[:, order[bounds[one]]][None]
    for p in np.flatnonzero(n_days > 1):
        n = int(n_days[p])
        s = np.sort(x[:, order[bounds[p]:bounds[p + 1]]], axis=1)          # NaN last
        k_lo = np.floor(np.asarray(q, dtype=np.float64) * np.float64(n - 1)).astype(np.int64)
        lo[:, :, p] = np.moveaxis(s[:, k_lo], 1, 0)
        hi[:, :, p] = np.moveaxis(s[:, np.minimum(k_lo + 1, n - 1)], 1, 0)
    return lo, hi, n_days


def capped_period_table(n_cols, E, n_first, rng):
    """(table [n_cols, D, 1, E], period_of_day [D], n_periods) for ``capped_periods``: the days of a period are of its kind."""
    kind, n = capped_periods(n_first)
    pod = np.repeat(np.arange(len(n)), n)
    D = len(pod)
    kind_of_day = np.repeat(np.asarray([KINDS.index(k) for k in kind]), n)
    t = np.empty((n_cols, D, 1, E))
    for i, k in enumerate(KINDS):
        days = kind_of_day == i
        if days.any():
            t[:, days] = time_table(k, (n_cols, int(days.sum()), 1, E), rng)
    return t, pod, len(n)
