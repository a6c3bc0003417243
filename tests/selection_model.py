"""A plain NumPy model of the library's two radix selects: what they return AND how many sweeps over the data they make to get
there.  It restates the rule the kernels' headers give (csrc/simplyp_quantile.hip.h, csrc/simplyp_time_quantile.hip.h) and
nothing of their code; tests/test_selection_model_host.py checks it against np.sort on the CPU, the device tests compare the
kernels' values, ``n_passes``, ``n_sweeps`` and ``bytes_read`` with it.

The rule both share.  A float64 maps to a 64-bit key that keeps np.sort's order (sign bit flipped for non-negatives, all bits
flipped for negatives, every NaN one key above +inf's).  The select settles the key of a wanted rank 8 bits at a time, most
significant digit first: one sweep over the data builds the 256-bin histogram of the next digit among the values that share
the digits settled so far (the "prefix"), the rank walks the bins to its digit and becomes a rank inside that bin (its
"bucket").  Wanted ranks with equal prefixes share a histogram (a "group").  Once the buckets are small enough, one last sweep
collects them and the answer is found there by sorting; after 8 digits the prefix is the key and no collecting sweep is made.

What differs:
* member axis (``member_select``): one workgroup owns a row; all groups are refined in the same sweep; the collecting sweep
  comes once EVERY wanted bucket holds at most ``list_len`` participating members (64 unweighted, 32 weighted, where a member
  with weight 0 does not count); rows of at most ``sort_max`` members (4096 / 2048) are sorted in one sweep instead.
* day axis (``time_select``): a lane owns a member, 64 lanes decide together: the collecting sweep comes once every lane's
  buckets (one per group) hold at most 128 keys together; until then a digit costs one sweep per group index, up to the
  largest number of groups any of the 64 lanes has.
"""

import numpy as np

QLIST, WQLIST = 64, 32                 # list_len of the two member-axis selects
QSORT_MAX, WQSORT_MAX = 4096, 2048     # longest rows their sorts take
TQ_LIST = 128                          # keys per lane the day-axis select collects
LANES = 64
KEY_NAN = np.uint64(0xFFF8000000000000)
_SIGN = np.uint64(0x8000000000000000)
_U8 = np.uint64(8)


def quantile_key(x):
    """The order-keeping uint64 keys of float64 values."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    b = x.view(np.uint64)
    k = np.where((b >> np.uint64(63)) != 0, ~b, b | _SIGN)
    return np.where(np.isnan(x), KEY_NAN, k)


def quantile_value(k):
    """The float64 values of keys (a prefix of 8 digits among them)."""
    k = np.ascontiguousarray(k, dtype=np.uint64)
    b = np.where((k >> np.uint64(63)) != 0, k & ~_SIGN, ~k)
    return b.view(np.float64)


def linear_ranks(q, n):
    """k_lo = floor(q (n - 1)), k_hi = min(k_lo + 1, n - 1) of numpy's 'linear' quantile: two int64 arrays [K]."""
    h = np.asarray(q, dtype=np.float64) * np.float64(n - 1)
    k_lo = np.clip(np.floor(h).astype(np.int64), 0, n - 1)
    return k_lo, np.minimum(k_lo + 1, n - 1)


def _under(keys, prefix, digits):
    """Which keys carry `prefix` in their first `digits` digits."""
    if digits == 0:
        return np.ones(keys.shape, dtype=bool)
    return (keys >> np.uint64(64 - 8 * digits)) == np.uint64(prefix)


# ---- member axis -------------------------------------------------------------------------------------------------------------

def member_select(row, ranks_or_thresholds, weights=None, include=None, sort_max=None, list_len=None):
    """One row [E] through the member-axis select.  Unweighted: ``ranks_or_thresholds`` are zero-based ranks among the
    participating members.  Weighted (``weights`` [E] integers): thresholds t >= 1, the answer is the first member in key order
    whose inclusive running weight reaches t.  A member takes part iff ``include`` says so and (weighted) its weight is > 0.
    Returns (values [T] float64, sweeps)."""
    row = np.ascontiguousarray(row, dtype=np.float64)
    weighted = weights is not None
    sort_max = (WQSORT_MAX if weighted else QSORT_MAX) if sort_max is None else sort_max
    list_len = (WQLIST if weighted else QLIST) if list_len is None else list_len
    part = np.ones(row.shape, dtype=bool) if include is None else np.asarray(include) != 0
    w = np.ones(row.shape, dtype=np.uint64)
    if weighted:
        w = np.asarray(weights).astype(np.uint64)
        part = part & (w > 0)
    keys, w = quantile_key(row)[part], w[part]
    # what is still to pass inside the bucket: the rank itself, or the weight below the threshold
    rem = [int(v) - 1 if weighted else int(v) for v in np.atleast_1d(ranks_or_thresholds)]
    T = len(rem)
    assert all(0 <= r < int(w.sum()) for r in rem)

    def settle(bucket_keys, bucket_w, r):
        order = np.argsort(bucket_keys, kind='stable')
        running = np.cumsum(bucket_w[order], dtype=np.uint64)
        return bucket_keys[order][int(np.argmax(running > np.uint64(r)))]

    if row.shape[0] <= sort_max:                                           # the LDS sort: one sweep
        return quantile_value(np.array([settle(keys, w, r) for r in rem], dtype=np.uint64)), 1
    prefix = [0] * T                                                       # per wanted value; equal prefixes = one group
    sweeps, collect = 0, False
    for digits in range(8):
        sweeps += 1
        if collect:
            found = []
            for t in range(T):
                m = _under(keys, prefix[t], digits)
                found.append(settle(keys[m], w[m], rem[t]))
            return quantile_value(np.array(found, dtype=np.uint64)), sweeps
        shift = np.uint64(56 - 8 * digits)
        biggest = 0
        for t in range(T):
            m = _under(keys, prefix[t], digits)
            digit = ((keys[m] >> shift) & np.uint64(0xFF)).astype(np.int64)
            hist = np.zeros(256, dtype=np.uint64)
            np.add.at(hist, digit, w[m])
            d = 0
            while d < 255 and rem[t] >= int(hist[d]):
                rem[t] -= int(hist[d])
                d += 1
            prefix[t] = (prefix[t] << 8) | d
            biggest = max(biggest, int((digit == d).sum()))                # members, not weight
        collect = biggest <= list_len
    return quantile_value(np.array(prefix, dtype=np.uint64)), sweeps       # all 64 bits settled: the prefix is the key


# ---- day axis ----------------------------------------------------------------------------------------------------------------

def time_select(block, days, ranks, loads=1):
    """One workgroup of the day-axis select on one period.  block [D, n] holds a series' values of the workgroup's n <= 64
    member slots for every day of the table; days: the period's day indices (at least one); ranks: the wanted ranks,
    ascending without repeats.  A partial workgroup's idle lanes shadow its last member.  loads: table rows the series reads
    per day (1: a column or Q_cumecs; 2: a concentration; 3: TP).
    Returns (values [T, n], sweeps, rows): rows = sweeps x days x loads, the 512-byte row segments the workgroup loaded."""
    block = np.asarray(block, dtype=np.float64)
    n_live = block.shape[1]
    assert 1 <= n_live <= LANES and len(days) >= 1
    cols = np.minimum(np.arange(LANES), n_live - 1)                        # idle lanes shadow the last member
    keys = quantile_key(block[np.asarray(days)][:, cols])                  # [n_days, 64]
    n = keys.shape[0]
    ranks = np.asarray(ranks, dtype=np.int64)
    T = len(ranks)
    assert T >= 1 and (np.diff(ranks) > 0).all() and 0 <= ranks[0] and ranks[-1] < n
    pre = np.zeros((T, LANES), dtype=np.uint64)
    rem = np.repeat(ranks[:, None], LANES, axis=1)
    cnt = np.full((T, LANES), n, dtype=np.int64)
    lane = np.arange(LANES)
    sweeps = 0
    found = None
    for digits in range(9):
        lead = np.ones((T, LANES), dtype=bool)                             # a rank whose prefix differs from its predecessor's
        lead[1:] = pre[1:] != pre[:-1]
        if digits == 8:                                                    # every digit settled: the prefixes are the keys
            found = pre
            break
        if ((cnt * lead).sum(axis=0) <= TQ_LIST).all():                    # every lane's lead buckets fit: collect, sort, done
            sweeps += 1
            found = np.zeros((T, LANES), dtype=np.uint64)
            for l in range(n_live):
                for t in range(T):
                    if lead[t, l]:
                        bucket = np.sort(keys[_under(keys[:, l], pre[t, l], digits), l])
                    found[t, l] = bucket[rem[t, l]]
            found[:, n_live:] = found[:, n_live - 1:n_live]
            break
        group = np.cumsum(lead, axis=0) - 1                                # per lane: the group index of every rank
        shift = np.uint64(56 - 8 * digits)
        digit = ((keys >> shift) & np.uint64(0xFF)).astype(np.int64)
        above = keys >> np.uint64(64 - 8 * digits) if digits else None
        for g in range(int(group[-1].max()) + 1):                          # one sweep per group index; lanes with fewer idle
            sweeps += 1
            mine = group == g                                              # [T, 64]
            on = mine.any(axis=0)
            P = pre[np.argmax(mine, axis=0), lane]                         # the group's prefix, per lane
            take = np.broadcast_to(on, keys.shape) if digits == 0 else on[None, :] & (above == P[None, :])
            hist = np.bincount((digit * LANES + lane[None, :])[take], minlength=256 * LANES).reshape(256, LANES)
            upto = np.cumsum(hist, axis=0)
            for t in range(T):
                ls = np.flatnonzero(mine[t])
                if len(ls) == 0:
                    continue
                d = np.argmax(upto[:, ls] > rem[t, ls][None, :], axis=0)  # the first bin the rank does not pass
                rem[t, ls] -= upto[d, ls] - hist[d, ls]
                cnt[t, ls] = hist[d, ls]
                pre[t, ls] = (P[ls] << _U8) | d.astype(np.uint64)
    return quantile_value(found)[:, :n_live], sweeps, sweeps * n * loads


def period_days(D, period_of_day=None, n_periods=None):
    """The day lists of a call: a list of int arrays, one per period."""
    if period_of_day is None:
        return [np.arange(D)]
    pod = np.asarray(period_of_day)
    P = (max(int(pod.max()) + 1, 1) if D else 1) if n_periods is None else n_periods
    order = np.flatnonzero(pod >= 0)
    bounds = np.searchsorted(pod[order], np.arange(P + 1))                 # the named periods do not decrease
    return [order[bounds[p]:bounds[p + 1]] for p in range(P)]


def time_quantiles(x, q, period_of_day=None, n_periods=None, loads=None):
    """A whole simplyp_time_quantiles call on the series x [n_series, D, R, E]: every (64 member slots, period, series, reach)
    is one ``time_select``.  loads [n_series] as in ``time_select`` (default 1 each).
    Returns (lower, upper [K, n_series, P, R, E] -- NaN for a period without days --, n_sweeps = the maximum over the
    workgroups, bytes_read = 512 x the sum of their rows)."""
    x = np.asarray(x, dtype=np.float64)
    n_series, D, R, E = x.shape
    periods = period_days(D, period_of_day, n_periods)
    loads = [1] * n_series if loads is None else list(loads)
    K = len(q)
    lower = np.full((K, n_series, len(periods), R, E), np.nan)
    upper = lower.copy()
    n_sweeps, rows = 0, 0
    n_blocks = -(-E // LANES)
    # one-day periods all at once: a period of <= 128 days is collected in its first sweep, and its only day is every rank's answer
    one = np.array([p for p, days in enumerate(periods) if len(days) == 1], dtype=np.int64)
    if len(one):
        day = np.array([periods[p][0] for p in one])
        lower[:, :, one] = upper[:, :, one] = x[:, day][None]
        n_sweeps = 1
        rows += len(one) * n_blocks * R * sum(loads)
    for p, days in enumerate(periods):
        if len(days) <= 1:
            continue
        k_lo, k_hi = linear_ranks(q, len(days))
        ranks = np.unique(np.concatenate([k_lo, k_hi]))
        for si in range(n_series):
            for r in range(R):
                for e0 in range(0, E, LANES):
                    v, s, n = time_select(x[si, :, r, e0:e0 + LANES], days, ranks, loads[si])
                    lower[:, si, p, r, e0:e0 + LANES] = v[np.searchsorted(ranks, k_lo)]
                    upper[:, si, p, r, e0:e0 + LANES] = v[np.searchsorted(ranks, k_hi)]
                    n_sweeps = max(n_sweeps, s)
                    rows += n
    return lower, upper, n_sweeps, 512 * rows
