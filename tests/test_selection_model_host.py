"""The model of the two radix selects (tests/selection_model.py) against np.sort and simplyp_amd/weighted.py, on the CPU: the
model's own check.  The device tests compare the kernels' sweep counts with the model's, so here the model's counts for the
rows built to sit on a limit are compared with numbers worked out by hand (tests/selection_cases.py and below).

Every value comparison is bit for bit, zeros of either sign counting as equal."""

import numpy as np
import pytest

import selection_cases as sc
import selection_model as sm
import weighted_cases as wc
from simplyp_amd import weighted

Q_FIXED = [0.0, 0.025, 0.5, 0.975, 1.0]
Q_TIME = [0.05, 0.5, 0.95]


def q_random(seed=2016):
    return list(np.random.default_rng(seed).uniform(0.0, 1.0, 16))


def same(got, want):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    ok = (got.view(np.int64) == want.view(np.int64)) | ((got == 0.0) & (want == 0.0)) | (np.isnan(got) & np.isnan(want))
    assert bool(ok.all()), (int((~ok).sum()), np.argwhere(~ok)[:5], got[~ok][:5], want[~ok][:5])
    return True


def select_row(row, q, include=None, **kw):
    """The model on one row for probabilities q: (lower, upper, sweeps) against np.sort."""
    x = row if include is None else row[np.asarray(include) != 0]
    k_lo, k_hi = sm.linear_ranks(q, len(x))
    v, sweeps = sm.member_select(row, np.concatenate([k_lo, k_hi]), include=include, **kw)
    s = np.sort(x)                                                         # NaN last
    same(v, np.concatenate([s[k_lo], s[k_hi]]))
    return sweeps


def weighted_row(row, w, probs, include=None, **kw):
    take = w > 0 if include is None else (w > 0) & (np.asarray(include) != 0)
    T = sum(int(v) for v in w[take])
    v, sweeps = sm.member_select(row, [weighted.threshold(p, T) for p in probs], weights=w, include=include, **kw)
    same(v, weighted.quantiles(row, w, probs, include=include))
    return sweeps


def test_keys_keep_np_sorts_order_and_come_back():
    x = np.array([-np.inf, -1e300, -1.0, -5e-324, -0.0, 0.0, 5e-324, 0.5, 1.0, 2.0, 2.0 ** 20, 1e300, np.inf, np.nan, -np.nan])
    k = sm.quantile_key(x)
    assert (k[1:13] > k[:12]).all() and k[13] == k[14] == sm.KEY_NAN > k[12]
    assert np.array_equal(sm.quantile_value(k[:13]).view(np.int64), x[:13].view(np.int64)) and np.isnan(sm.quantile_value(k[13:])).all()
    # the first digits the constructed rows rely on
    assert [int(v >> np.uint64(56)) for v in sm.quantile_key([0.5, 0.999, 2.0, 3.999, 2.0 ** 20, 2.0 ** 21 - 1])] == [0xBF, 0xBF, 0xC0, 0xC0, 0xC1, 0xC1]
    second = (sm.quantile_key(sc.ramp(2.0, 65)) >> np.uint64(48)) & np.uint64(0xFF)
    assert len(np.unique(second)) == 16 and (sm.quantile_key(sc.ramp(2.0, 65, narrow=True)) >> np.uint64(48) == 0xC000).all()


@pytest.mark.parametrize('E,sort_max,list_len', [(300, 0, 4), (300, 0, 64), (1000, 0, 1), (sc.E_SELECT, None, None), (4096, None, None)])
def test_member_select_equals_np_sort(E, sort_max, list_len):
    """Rows of every kind the device tests use, the limits lowered so that short rows take many digits too."""
    rng = np.random.default_rng(E)
    kw = {} if sort_max is None else dict(sort_max=sort_max, list_len=list_len)
    rows = [rng.normal(size=E) * 1e3, rng.choice(np.array([-3.5, -0.0, 0.0, 2.0 ** -1040, 7.25e11]), size=E), np.full(E, -0.0),
            wc.values('special', (E,), rng)]
    inc = rng.random(E) < 0.6
    for row in rows:
        for q in (Q_FIXED, q_random()):
            sweeps = select_row(row, q, **kw)
            assert 1 <= sweeps <= 8 and (sweeps == 1) == (E <= sm.QSORT_MAX and sort_max is None)
            select_row(row, q, include=inc, **kw)
    assert select_row(rows[2], Q_FIXED, **kw) == (1 if E == 4096 else 8)  # a flat row: every digit, then the prefix is the key


@pytest.mark.parametrize('E,sort_max,list_len', [(300, 0, 2), (300, 0, 32), (sc.E_WSELECT, None, None), (2048, None, None)])
def test_weighted_member_select_equals_the_integer_rule(E, sort_max, list_len):
    rng = np.random.default_rng(E + 1)
    kw = {} if sort_max is None else dict(sort_max=sort_max, list_len=list_len)
    inc = rng.random(E) < 0.7
    for vp in wc.VALUE_PATTERNS:
        row = wc.values(vp, (E,), rng)
        for wp in ('ones', 'all_max', 'one_heavy', 'zeros30', 'one_survivor'):
            w = wc.weights(wp, E, rng)
            sweeps = weighted_row(row, w, wc.PROBS + [float(p) for p in rng.uniform(0, 1, 11)], **kw)
            assert 1 <= sweeps <= 8
            if int(((w > 0) & inc).sum()):
                weighted_row(row, w, wc.PROBS, include=inc, **kw)


@pytest.mark.parametrize('case', sc.member_cases(), ids=lambda c: c[0])
def test_member_rows_on_the_list_limit(case):
    """Sweeps by hand (selection_cases.member_cases): 2 when the wanted bucket holds 64 after the first digit, 3 when it holds
    65 that part in the second, 4 when they share the second; a collect that waits for the larger of two groups."""
    name, n_top, n_far, narrow, probs, sweeps = case
    table = sc.member_table(case, 3, np.random.default_rng(len(name)))
    for row in table:
        assert ((row >= 2) & (row < 4)).sum() == n_top and (row >= 2.0 ** 20).sum() == n_far
        assert select_row(row, probs) == sweeps
    # the same row one member shorter is sorted in LDS: one sweep
    assert sm.member_select(table[0][:4096], [4000])[1] == 1


@pytest.mark.parametrize('case', sc.weighted_cases(), ids=lambda c: c[0])
def test_weighted_rows_on_the_list_limit(case):
    rng = np.random.default_rng(len(case[0]))
    w = wc.weights('zeros30', sc.E_WSELECT, rng)
    table, probs, (T, w_top, w_far) = sc.weighted_table(case, w, 3, rng)
    lo, hi = T - w_far - w_top, T - w_far
    thr = [weighted.threshold(p, T) for p in probs]
    assert all(lo < t <= hi or (t > hi and 'both' in case[0]) for t in thr) and any(lo < t <= hi for t in thr)
    for row in table:
        top = (row >= 2) & (row < 4)
        assert (top & (w > 0)).sum() == case[1] and (top & (w == 0)).sum() == case[2] and ((row >= 2.0 ** 20) & (w > 0)).sum() == case[3]
        assert weighted_row(row, w, probs) == case[5]


def test_base_rows_of_the_capped_tables():
    rng = np.random.default_rng(6)
    for q in (Q_FIXED, q_random()):
        sweeps = [select_row(row, q) for row in sc.base_rows(sc.E_SELECT, sm.QLIST, rng)]
        assert max(sweeps) == sweeps[2] == 8                               # the flat row
    w = wc.weights('zeros30', sc.E_WSELECT, rng)
    for probs in (wc.PROBS, wc.PROBS + [float(p) for p in rng.uniform(0, 1, 11)]):
        sweeps = [weighted_row(row, w, probs) for row in sc.base_rows(sc.E_WSELECT, sm.WQLIST, rng, weights=w)]
        assert max(sweeps) == sweeps[2] == 8


# ---- day axis ------------------------------------------------------------------------------------------------------------------

def check_time(x, q, pod=None, n_periods=None, loads=None):
    lower, upper, n_sweeps, bytes_read = sm.time_quantiles(x, q, pod, n_periods, loads)
    D = x.shape[1]
    pod_ = np.zeros(D, dtype=np.int64) if pod is None else pod
    P = int(pod_.max()) + 1 if n_periods is None else n_periods
    want_lo, want_hi, _ = sc.sorted_periods(x, q, pod_, P)
    same(lower, want_lo)
    same(upper, want_hi)
    return n_sweeps, bytes_read


@pytest.mark.parametrize('D', [1, 2, 127, 128, 129, 300])
def test_time_select_equals_np_sort(D):
    """A period of at most 128 days is collected in its first sweep; 129 days cost a digit first."""
    rng = np.random.default_rng(D)
    for kind in sc.KINDS:
        x = sc.time_table(kind, (1, D, 2, 70), rng)
        for q in ([0.0], [1.0], Q_TIME, q_random(D)):
            n_sweeps, bytes_read = check_time(x, q)
            assert (n_sweeps == 1) == (D <= 128) and bytes_read >= 512 * n_sweeps * D
            if D <= 128:
                assert bytes_read == 512 * D * 2 * 2                       # one sweep by 2 reaches x 2 member blocks
    # one lane alone: the shadows of the last member decide nothing
    ends = sorted({0, D - 1})
    v, sweeps, rows = sm.time_select(x[0, :, 0, :1], np.arange(D), ends, loads=3)
    same(v[:, 0], np.sort(x[0, :, 0, 0])[ends])
    assert rows == sweeps * D * 3


def test_lanes_whose_lead_buckets_total_128_and_129():
    """D = 300: 172 FILL, 64 TOP and 64 (65) FAR values per lane, ranks among TOP and FAR.  Digit 1 is one sweep (300 > 128);
    then a lane has two groups of 64 + 64 = 128 keys: collect, 2 sweeps.  With 64 + 65 = 129 in ONE lane the whole wave goes
    on: digit 2 costs a sweep per group, 2, and leaves buckets of at most 5: collect, 1 + 2 + 1 = 4 sweeps."""
    D, E = 300, 70
    q = [0.6, 0.9, 1.0]                                                    # ranks 179, 180 (TOP), 269, 270, 299 (FAR)
    rng = np.random.default_rng(128)
    x = sc.lead_bucket_table((2, D, 1, E), 64, rng)
    assert check_time(x, q) == (2, 512 * 2 * D * 2 * 2)                    # 2 sweeps by 2 series x 2 member blocks
    x = sc.lead_bucket_table((2, D, 1, E), 64, rng, odd_lane=(5, 65))
    assert check_time(x, q) == (4, 512 * (4 + 2) * D * 2)                  # the first wave 4, the second (6 lanes) 2
    x = sc.lead_bucket_table((2, D, 1, E), 65, rng)
    assert check_time(x, q) == (4, 512 * 4 * D * 2 * 2)
    # a rank among the FILL values as well: three groups, 172 + 64 + 64 keys: a sweep per group for digit 2
    assert check_time(x[:1], [0.1, 0.6, 0.9])[0] >= 1 + 3 + 1


@pytest.mark.parametrize('D', [300, 1000])
def test_mixed_waves(D):
    """Lanes of different kinds in one wave: the wave sweeps as long as its slowest lane and as often as its lane with the
    most groups."""
    rng = np.random.default_rng(D)
    shape = (1, D, 1, 130)
    pod = sc.periods_130_1_200(D)
    for x in (sc.mixed_table(shape, rng), sc.lone_lanes_table(shape, rng)):
        for q in ([0.0], Q_TIME, q_random()):
            n_sweeps, _ = check_time(x, q)
            assert n_sweeps >= 8                                           # the 'equal' lanes: 8 digits, no collect
            check_time(x, q, pod, 4)
    # the lone lanes hold their own waves back, not the middle one: q = 0 wants ranks 0 and 1, the 'equal' lane keeps them in one
    # group through 8 digits while its smooth neighbours part them and pay two sweeps a digit from there on
    x = sc.lone_lanes_table(shape, rng)
    per_wave = [sm.time_quantiles(x[..., e0:e1], [0.0])[2] for e0, e1 in ((0, 64), (64, 128), (128, 130))]
    assert per_wave[1] < 8 < per_wave[0] and per_wave[1] < per_wave[2]
    assert sm.time_quantiles(x[..., 17:18], [0.0])[2] == 8 and sm.time_quantiles(x, [0.0])[2] == max(per_wave)


def test_periods_past_the_grid_cap():
    rng = np.random.default_rng(65535)
    x, pod, P = sc.capped_period_table(2, 3, 65535, rng)
    kind, n = sc.capped_periods(65535)
    assert P == 65535 + 70 and len(pod) == n.sum() and n[64] == n[65535 + 33] == 0 and n[65535 + 64] == 250
    n_sweeps, bytes_read = check_time(x, Q_TIME, pod, P)
    assert n_sweeps >= 8 and bytes_read > 512 * 2 * n.sum()
