"""Per-member quantiles over time selected on the device (simplyp_time_quantiles): the order statistics against np.sort along
the day axis on made-up tables of every shape the kernel's paths take (periods of <= 128 days are collected at once, longer
ones refined digit by digit; full and partial waves; one and several reaches), periods with holes and without days, the six
derived series against their numpy restatement, slot order, determinism, argument errors, and the statistic through
run_simply_p_ensemble -- one device, two contexts, windows, and the band across members of the per-member statistics.

Reference everywhere: numpy on the host -- s = np.sort(x, axis=0) over the period's days, expected s[k_lo], s[k_hi] with
k_lo = floor(q (n - 1)), k_hi = min(k_lo + 1, n - 1).  Order statistics are elements of their series: compared BIT FOR BIT,
except where both values are zeros (either zero may come back; compared with ==), as tests/test_gpu_quantiles.py does.
The derived series are compared bit for bit too: the kernel evaluates the reference's expressions operation for operation."""

import ctypes as C

import numpy as np
import pytest

import helpers
import selection_cases as sc
import selection_model as sm
import simplyp_amd as sp
from simplyp_amd import abi, engine, marshal

pytestmark = pytest.mark.gpu

COL = {c: i for i, c in enumerate(marshal.ALL_COLUMNS)}
MASK2 = (1 << COL['Vr']) | (1 << COL['Qr'])
FLUX4 = ['Qr', 'Msus_kg/day', 'TDP_kg/day', 'PP_kg/day']
MASK5 = marshal.mask_of_columns(['Vr'] + FLUX4)
DERIVED = [abi.TQ_DERIVED + v for v in range(6)]
Q_BAND = [0.05, 0.5, 0.95]


def q_random(seed=2016):
    return list(np.random.default_rng(seed).uniform(0.0, 1.0, 16))


def expected(x, q, period_of_day=None, n_periods=None):
    """np.sort's view of x [n_series, D, R, E]: lower, upper [K, n_series, P, R, E] and n_days [P]."""
    D = x.shape[1]
    pod = np.zeros(D, dtype=np.int64) if period_of_day is None else np.asarray(period_of_day)
    P = (max(int(pod.max()) + 1, 1) if D else 1) if n_periods is None else n_periods
    lo = np.full((len(q), x.shape[0], P) + x.shape[2:], np.nan)
    hi = lo.copy()
    n_days = np.zeros(P, dtype=np.int64)
    for p in range(P):
        days = np.flatnonzero(pod == p)
        n = n_days[p] = len(days)
        if n == 0:
            continue
        s = np.sort(x[:, days], axis=1)                                    # NaN last
        h = np.asarray(q, dtype=np.float64) * np.float64(n - 1)
        k_lo = np.floor(h).astype(np.int64)
        k_hi = np.minimum(k_lo + 1, n - 1)
        lo[:, :, p] = np.moveaxis(s[:, k_lo], 1, 0)
        hi[:, :, p] = np.moveaxis(s[:, k_hi], 1, 0)
    return lo, hi, n_days


def same(got, want):
    """Bit for bit, except that a zero matches a zero of either sign."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    ok = (got.view(np.int64) == want.view(np.int64)) | ((got == 0.0) & (want == 0.0)) | (np.isnan(got) & np.isnan(want))
    assert bool(ok.all()), (int((~ok).sum()), np.argwhere(~ok)[:5], got[~ok][:5], want[~ok][:5])
    return True


make_table, KINDS = sc.time_table, sc.KINDS                               # [n_cols, D, R, E] of one kind


def dev(engine0, a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(engine0.tdev)


def check(engine0, table, mask, q, series, x, period_of_day=None, n_periods=None, **kw):
    """Engine.time_quantiles on `table` (numpy [n_cols, D, R, E]) against np.sort of x [n_series, D, R, E]."""
    lower, upper, info = engine0.time_quantiles(dev(engine0, table), mask, q, series=series, period_of_day=period_of_day,
                                                n_periods=n_periods, **kw)
    want_lo, want_hi, n_days = expected(x, q, period_of_day, n_periods)
    assert tuple(lower.shape) == tuple(upper.shape) == want_lo.shape
    assert np.array_equal(info['n_days'], n_days) and info['n_periods'] == len(n_days)
    same(lower.cpu().numpy(), want_lo)
    same(upper.cpu().numpy(), want_hi)
    return info


def check_model(engine0, table, mask, q, series, x, period_of_day=None, n_periods=None, loads=None, **kw):
    """``check``, and the call's n_sweeps and bytes_read against tests/selection_model.py (whose values must be np.sort's too)."""
    info = check(engine0, table, mask, q, series, x, period_of_day, n_periods, **kw)
    lo, hi, n_sweeps, bytes_read = sm.time_quantiles(x, q, period_of_day, n_periods, loads)
    want_lo, want_hi, _ = expected(x, q, period_of_day, n_periods)
    same(lo, want_lo)
    same(hi, want_hi)
    assert (info['n_sweeps'], info['bytes_read']) == (n_sweeps, bytes_read)
    return info


@pytest.mark.parametrize('E', [1, 63, 64, 65, 130])
@pytest.mark.parametrize('D', [1, 2, 127, 128, 129, 255, 256, 257, 1000])
def test_order_statistics_are_exact(engine0, E, D):
    """D = 127, 128, 129: TQ_LIST = 128, the days a lane collects in its first sweep; one more costs a digit first."""
    rng = np.random.default_rng(1000 * D + E)
    cols = [COL['Vr'], COL['Qr']]
    for kind in KINDS:
        for R in (1, 3):
            table = make_table(kind, (2, D, R, E), rng)
            for q in ([0.0], [0.5], [1.0], q_random(D + E)):
                info = (check_model if D == 129 else check)(engine0, table, MASK2, q, cols, table)
                assert 1 <= info['n_sweeps'] <= 8 * 2 * len(q) + 1
                if D <= 128:
                    assert info['n_sweeps'] == 1                           # collected at once
                if D == 129:
                    assert info['n_sweeps'] >= 2                           # a digit, then the collect (or more digits)
            # one series, the second column alone, the order reversed
            check(engine0, table, MASK2, Q_BAND, [COL['Qr']], table[1:])
            check(engine0, table, MASK2, Q_BAND, cols[::-1], table[::-1])


def test_default_series_are_the_columns_of_the_mask(engine0):
    rng = np.random.default_rng(3)
    table = make_table('smooth', (2, 300, 2, 70), rng)
    check(engine0, table, MASK2, Q_BAND, None, table)


PERIOD_CASES = {
    'every day its own': lambda D: np.arange(D),
    'unequal lengths': lambda D: np.repeat(np.arange(4), [130, 1, 200, D - 331]),
    'holes at the start, in the middle and at the end': lambda D: np.concatenate(
        [np.full(17, -1), np.zeros(150), np.full(40, -1), np.ones(129), np.full(D - 336, -1)]).astype(np.int64),
    'holes inside a period': lambda D: np.where(np.arange(D) % 3 == 1, -1, np.arange(D) // 200),
    'an empty period in the middle': lambda D: np.where(np.arange(D) < 180, 0, 2),
    'no day at all': lambda D: np.full(D, -1),
}


@pytest.mark.parametrize('case', list(PERIOD_CASES))
def test_periods(engine0, case):
    D, R, E = 400, 2, 70
    rng = np.random.default_rng(len(case))
    pod = PERIOD_CASES[case](D)
    assert pod.shape == (D,)
    for kind in ('smooth', 'special'):
        table = make_table(kind, (2, D, R, E), rng)
        for q in (Q_BAND, q_random(5)):
            info = check(engine0, table, MASK2, q, [COL['Vr'], COL['Qr']], table, period_of_day=pod)
    if case == 'an empty period in the middle':
        assert list(info['n_days']) == [180, 0, 220]
        lower, upper, _ = engine0.time_quantiles(dev(engine0, table), MASK2, Q_BAND, period_of_day=pod)
        assert bool(lower[:, :, 1].isnan().all()) and bool(upper[:, :, 1].isnan().all())
        assert not bool(lower[:, :, 0].isnan().all()) and not bool(lower[:, :, 2].isnan().all())
    if case == 'no day at all':
        assert list(info['n_days']) == [0]
    # trailing periods that no day names exist when the caller says so
    check(engine0, table, MASK2, Q_BAND, [COL['Qr']], table[1:], period_of_day=pod, n_periods=int(pod.max()) + 3)


def test_lanes_whose_lead_buckets_total_128_and_129(engine0):
    """tq_select collects when __all(total <= TQ_LIST), total = the keys in a lane's lead buckets.  D = 300: every lane holds 172
    FILL, 64 TOP and 64 FAR values (three first digits), the ranks lie among TOP and FAR: after the first digit (1 sweep) a lane
    has two groups of 64 + 64 = 128 keys -> collect: n_sweeps = 2.  One lane with 65 FAR values (129) sends its whole wave
    through the second digit, a sweep per group, before the collect: 1 + 2 + 1 = 4, while the other wave (6 lanes) makes 2."""
    D, E = 300, 70
    q = [0.6, 0.9, 1.0]                                                    # ranks 179, 180 (TOP), 269, 270, 299 (FAR)
    rng = np.random.default_rng(128)
    cols = [COL['Vr'], COL['Qr']]
    table = sc.lead_bucket_table((2, D, 1, E), 64, rng)
    info = check_model(engine0, table, MASK2, q, cols, table)
    assert (info['n_sweeps'], info['bytes_read']) == (2, 512 * 2 * D * 2 * 2)          # 2 sweeps by 2 series x 2 waves
    table = sc.lead_bucket_table((2, D, 1, E), 64, rng, odd_lane=(5, 65))
    info = check_model(engine0, table, MASK2, q, cols, table)
    assert (info['n_sweeps'], info['bytes_read']) == (4, 512 * (4 + 2) * D * 2)
    table = sc.lead_bucket_table((2, D, 1, E), 65, rng)
    info = check_model(engine0, table, MASK2, q, cols, table)
    assert (info['n_sweeps'], info['bytes_read']) == (4, 512 * 4 * D * 2 * 2)


@pytest.mark.parametrize('D', [300, 1000])
@pytest.mark.parametrize('lanes', ['every kind in every wave', 'one equal lane, one lastbits lane'])
def test_mixed_waves(engine0, lanes, D):
    """tq_select decides for the 64 lanes together: __all(total <= TQ_LIST) before the collect, while (__any(cur < T)) over the
    group indices, and the break at level == 8 that ends a wave no lane of which could collect.  Here the lanes of a wave differ: member
    e is of kind KINDS[e % 5], or all are smooth but one 'equal' lane in the first wave and one 'lastbits' lane in the partial
    third (E = 130) -- lanes that need 8 digits beside lanes that settle after two, lanes with one group beside lanes with
    several (idle, on == false, in the extra sweeps)."""
    E, R = 130, 2
    rng = np.random.default_rng(D + len(lanes))
    table = (sc.mixed_table if lanes.startswith('every') else sc.lone_lanes_table)((2, D, R, E), rng)
    pod = sc.periods_130_1_200(D)
    for q in ([0.0], Q_BAND, q_random()):
        info = check_model(engine0, table, MASK2, q, [COL['Qr']], table[1:])
        assert info['n_sweeps'] >= 8                                       # the 'equal' lane's wave: 8 digits and no collect
        check_model(engine0, table, MASK2, q, [COL['Qr']], table[1:], period_of_day=pod, n_periods=4)


def test_periods_past_the_grid_cap(engine0):
    """The launch caps grid.y at 65535 and tq_periods strides over the periods (p += gridDim.y), re-initialising the per-lane
    state and reusing hist as list.  65535 + 70 periods (selection_cases.capped_periods): a workgroup takes period y and then
    65535 + y -- 200 days and then 129-300 or one, 200 days that take all 8 digits and then a smooth period, a full period and
    then an empty one, an empty one and then a full one, one day and then a long period of each kind."""
    P0, E = 65535, 3
    rng = np.random.default_rng(P0)
    table, pod, P = sc.capped_period_table(5, E, P0, rng)
    assert P == P0 + 70 and table.shape[1] == len(pod)
    A, f = rng.uniform(5.0, 80.0, size=(1, E)), rng.uniform(0.3, 0.95, size=E)
    rp = np.zeros((len(marshal.PR_NAMES), 1, E))
    rp[marshal.PR_NAMES.index('A_catch')] = A
    x = np.stack([table[0], derived_numpy(table, A, f)[0]])                # the column Vr and the derived Q_cumecs
    lower, upper, info = engine0.time_quantiles(dev(engine0, table), MASK5, Q_BAND, series=[COL['Vr'], DERIVED[0]], period_of_day=pod,
                                                n_periods=P, f_tdp=f, reach_params=rp)
    want_lo, want_hi, n_days = sc.sorted_periods(x, Q_BAND, pod, P)        # np.sort per period, the one-day periods at once
    assert np.array_equal(info['n_days'], n_days) and n_days[64] == n_days[P0 + 33] == 0 and n_days[P0 + 64] == 250
    same(lower.cpu().numpy(), want_lo)
    same(upper.cpu().numpy(), want_hi)
    lo, hi, n_sweeps, bytes_read = sm.time_quantiles(x, Q_BAND, pod, P)
    same(lo, want_lo)
    same(hi, want_hi)
    assert (info['n_sweeps'], info['bytes_read']) == (n_sweeps, bytes_read) and n_sweeps >= 8


def derived_numpy(table5, A, f):
    """The six df_R series from the table's Qr and flux columns (columns of MASK5: Vr, Qr, Msus, TDP, PP), A [R, E], f [E]:
    the reference's expressions (model.py:784-793, :842-845) one operation after the other."""
    qr, ms, td, pp = table5[1], table5[2], table5[3], table5[4]
    with np.errstate(all='ignore'):
        Q = qr * A * 1000 / 86400
        SS = (ms / qr) / A
        TDP = (td / qr) / A
        PP = (pp / qr) / A
        TP = TDP + PP
        SRP = TDP * f
    return np.stack([Q, SS, TDP, PP, TP, SRP])


def derived_problem(rng, D, S, E, zeros=True):
    table = make_table('smooth', (5, D, S, E), rng)
    table[2:] *= 10.0 ** rng.integers(-2, 3, size=(3, 1, 1, 1))
    if zeros:                                                              # dry days: 0/0 = NaN, x/0 = inf -- sorted like numpy
        hit = rng.random(size=table.shape[1:]) < 0.02
        table[1][hit] = 0.0
        table[3][hit & (rng.random(size=hit.shape) < 0.5)] = 0.0
    A = rng.uniform(5.0, 80.0, size=(S, E))
    f = rng.uniform(0.3, 0.95, size=E)
    rp = np.zeros((len(marshal.PR_NAMES), S, E))
    rp[marshal.PR_NAMES.index('A_catch')] = A
    return table, A, f, rp


@pytest.mark.parametrize('D,E', [(100, 65), (700, 130)])
def test_derived_series_bit_for_bit(engine0, D, E):
    rng = np.random.default_rng(D)
    S = 2
    table, A, f, rp = derived_problem(rng, D, S, E)
    x = derived_numpy(table, A, f)
    pod = np.repeat(np.arange(2), [D // 3, D - D // 3])
    for q in (Q_BAND, q_random(D)):
        check(engine0, table, MASK5, q, DERIVED, x, f_tdp=f, reach_params=rp)
        check(engine0, table, MASK5, q, DERIVED, x, period_of_day=pod, f_tdp=f, reach_params=rp)
    # mixed with plain columns, and on a subset of the reaches (A_catch is looked up by reach id)
    check(engine0, table, MASK5, Q_BAND, [COL['Qr'], DERIVED[5], COL['Vr'], DERIVED[0]], np.stack([table[1], x[5], table[0], x[0]]),
          f_tdp=f, reach_params=rp)
    sub = np.ascontiguousarray(table[:, :, 1:])
    check(engine0, sub, MASK5, Q_BAND, DERIVED, derived_numpy(sub, A[1:], f), f_tdp=f, reach_params=rp, out_reaches=[1])


def test_slot_order(engine0):
    D, S, E = 300, 2, 130
    rng = np.random.default_rng(12)
    table, A, f, rp = derived_problem(rng, D, S, E)
    x = np.concatenate([table[:2], derived_numpy(table, A, f)])
    series = [COL['Vr'], COL['Qr']] + DERIVED
    perm = rng.permutation(E).astype(np.int32)                             # slot j holds member perm[j]
    want_lo, want_hi, _ = expected(x, Q_BAND)
    lo_m, up_m, _ = engine0.time_quantiles(dev(engine0, table), MASK5, Q_BAND, series=series, f_tdp=f, reach_params=rp)
    lo_s, up_s, _ = engine0.time_quantiles(dev(engine0, table[..., perm]), MASK5, Q_BAND, series=series, f_tdp=f, reach_params=rp,
                                           member_of_slot=dev(engine0, perm))
    same(lo_m.cpu().numpy(), want_lo)
    same(up_m.cpu().numpy(), want_hi)
    assert np.array_equal(lo_s.cpu().numpy().view(np.int64), lo_m.cpu().numpy()[..., perm].view(np.int64))
    assert np.array_equal(up_s.cpu().numpy().view(np.int64), up_m.cpu().numpy()[..., perm].view(np.int64))


def test_deterministic_and_table_untouched(engine0):
    import torch
    rng = np.random.default_rng(77)
    table, A, f, rp = derived_problem(rng, 500, 1, 200)
    table[0] = make_table('special', (1, 500, 1, 200), rng)[0]
    t = dev(engine0, table)
    before = t.view(torch.int64).clone()
    series = [COL['Vr'], COL['Qr']] + DERIVED
    pod = np.arange(500) // 170
    a = engine0.time_quantiles(t, MASK5, q_random(), series=series, period_of_day=pod, f_tdp=f, reach_params=rp)
    b = engine0.time_quantiles(t, MASK5, q_random(), series=series, period_of_day=pod, f_tdp=f, reach_params=rp)
    for x, y in zip(a[:2], b[:2]):
        assert bool(torch.equal(x.view(torch.int64), y.view(torch.int64)))
    assert a[2]['n_sweeps'] == b[2]['n_sweeps'] and a[2]['bytes_read'] == b[2]['bytes_read'] > 0
    assert bool(torch.equal(t.view(torch.int64), before))


def test_argument_errors(engine0):
    import torch
    L = engine.lib()
    E, D, S = 100, 40, 2
    t = torch.ones((5, D, S, E), dtype=torch.float64, device=engine0.tdev)
    out = torch.full((2, 16, 32, 3, S, E), -7.0, dtype=torch.float64, device=engine0.tdev)
    ft = torch.ones(E, dtype=torch.float64, device=engine0.tdev)
    rp = torch.ones((len(marshal.PR_NAMES), S, E), dtype=torch.float64, device=engine0.tdev)
    info = abi.TqInfo()
    i32 = C.POINTER(C.c_int32)

    def call(mask=MASK5, table=True, f=True, r=True, series=(COL['Qr'],), n_series=None, pod=None, P=0, q=(0.5,), K=None,
             stats=True, E_=E, D_=D):
        qa = None if q is None else np.ascontiguousarray(q, dtype=np.float64)
        sa = None if series is None else np.ascontiguousarray(series, dtype=np.int32)
        pa = None if pod is None else np.ascontiguousarray(pod, dtype=np.int32)
        dims = abi.Dims(E_, S, D_, 1)
        with torch.cuda.device(engine0.tdev):
            return L.simplyp_time_quantiles(engine0._h, C.byref(dims), mask, None, S, t.data_ptr() if table else None, None,
                                            ft.data_ptr() if f else None, rp.data_ptr() if r else None,
                                            None if sa is None else sa.ctypes.data_as(i32), (0 if sa is None else len(sa)) if n_series is None else n_series,
                                            None if pa is None else pa.ctypes.data_as(i32), P,
                                            None if qa is None else qa.ctypes.data_as(C.POINTER(C.c_double)),
                                            (0 if qa is None else len(qa)) if K is None else K,
                                            out.data_ptr() if stats else None, None, C.byref(info))
    no_flux = marshal.mask_of_columns(['Vr', 'Qr', 'TDP_kg/day', 'PP_kg/day'])
    bad = [dict(q=(), K=0), dict(q=[0.5] * 17), dict(q=(-1e-9,)), dict(q=(1.0 + 1e-9,)), dict(q=(0.5, np.nan)),
           dict(series=(COL['VsA'],)),                                     # a column that is not in the mask
           dict(series=(abi.TQ_DERIVED + 6,)), dict(series=(40,)), dict(series=(-1,)),
           dict(series=(DERIVED[0],), mask=no_flux),                       # derived without Msus_kg/day
           dict(series=(DERIVED[1],), mask=MASK5 & ~(1 << COL['Qr'])),     # derived without Qr
           dict(series=(DERIVED[5],), f=False), dict(series=(DERIVED[0],), r=False),
           dict(pod=np.r_[np.ones(20), np.zeros(20)], P=2),                # decreasing
           dict(pod=np.r_[np.zeros(10), np.full(5, -1), np.ones(20), np.zeros(5)], P=2),
           dict(pod=np.full(D, 2), P=2), dict(pod=np.full(D, -2), P=2),    # outside [-1, n_periods)
           dict(series=(), n_series=0), dict(series=[COL['Qr']] * 33), dict(series=None, n_series=1),
           dict(table=False), dict(q=None, K=1), dict(stats=False), dict(E_=0), dict(D_=-1)]
    for kw in bad:
        assert call(**kw) == -1, kw                                        # SIMPLYP_ERR_ARG
        assert b'simplyp_time_quantiles' in L.simplyp_last_error(engine0._h), kw
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())                                       # nothing was written
    # a valid call afterwards works: K = 1, one series, one period -> the first 2 * S * E outputs
    assert call() == 0
    flat = out.flatten()
    assert bool((flat[:2 * S * E] == 1.0).all()) and bool((flat[2 * S * E:] == -7.0).all())
    assert info.n_periods == 1 and info.n_sweeps == 1
    # D = 0: succeeds, every output NaN
    assert call(D_=0) == 0 and bool(flat[:2 * S * E].isnan().all()) and bool((flat[2 * S * E:] == -7.0).all())
    with pytest.raises(ValueError):
        engine0.time_quantiles(t[..., ::2], MASK5, [0.5])                  # not contiguous


# ---- through the public call ----------------------------------------------------------------------------------------------

SERIES = ['Qr', 'Q_cumecs', 'SRP_mgl']


def overrides_for(name, E, seed=3):
    """a_Q, T_g, E_M, fc of the scenario's workbook scaled by seeded uniform factors (the ranges of
    tests/test_gpu_quantiles.py::overrides_for), and a per-member f_TDP, as `overrides`."""
    base = helpers.marshal_scenario(name, E=1)['member_params'][:, 0]
    rng = np.random.default_rng(seed)
    over = {pname: base[marshal.PM_NAMES.index(pname)] * rng.uniform(lo, hi, E)
            for pname, lo, hi in (('a_Q', 0.6, 1.6), ('T_g', 0.7, 1.4), ('E_M', 0.5, 2.0), ('fc', 0.85, 1.15))}
    over['f_TDP'] = rng.uniform(0.4, 0.9, E)
    return over


def call(name, E, over=None, windows=None, met_slice=None, **kw):
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(name)
    if met_slice is not None:
        met = met.iloc[met_slice]
    over = overrides_for(name, E) if over is None else over
    if windows is not None:
        return list(sp.run_simply_p_ensemble_windows(met, p_struc, p_SU, p_LU, p_SC, p, dyn, window=windows, overrides=over, **kw))
    return sp.run_simply_p_ensemble(met, p_struc, p_SU, p_LU, p_SC, p, dyn, overrides=over, **kw)


def series_from_table(res, names, A, f):
    """[n_series, D, n_reaches, E] of the named series from the host table of the same call."""
    col = lambda c: res['data'][res['columns'].index(c)]
    t5 = np.stack([col('Qr')] + [col(c) for c in FLUX4])
    d = derived_numpy(t5, A, f)
    return np.stack([d[abi.TQ_DERIVED_SERIES.index(n)] if n in abi.TQ_DERIVED_SERIES else col(n) for n in names])


def matches_numpy(tq, x, q, pod=None, members=None):
    """lower / upper against np.sort for every member; data against np.quantile for `members` (np.quantile answers NaN for a
    series that holds one, whatever q)."""
    want_lo, want_hi, n_days = expected(x, q, pod)
    assert np.array_equal(tq['n_days'], n_days)
    same(tq['lower'], want_lo)
    same(tq['upper'], want_hi)
    for p, n in enumerate(n_days):
        days = np.arange(x.shape[1]) if pod is None else np.flatnonzero(pod == p)
        want = np.quantile(x[:, days], q, axis=1, method='linear')
        keep = slice(None) if members is None else members
        same(tq['data'][:, :, p][..., keep], want[..., keep])


E_2004 = 130


@pytest.fixture(scope='module')
def run_2004(engine0):
    name = 'tarland_2004_dynamic'
    res = call(name, E_2004, time_quantiles=Q_BAND, time_quantile_series=SERIES)
    A = float(helpers.scenario_inputs(name)[4].loc['A_catch', 1])
    return res, A, overrides_for(name, E_2004)['f_TDP']


def test_public_call_equals_numpy_on_its_own_table(run_2004):
    res, A, f = run_2004
    assert (res['status'] & abi.STATUS_NONFINITE == 0).all()
    assert set(FLUX4) <= set(res['columns']) and res['data'].shape[1:] == (366, 1, E_2004)
    tq = res['time_quantiles']
    assert tq['q'] == Q_BAND and tq['series'] == SERIES and tq['periods'] is None
    assert tq['data'].shape == tq['lower'].shape == tq['upper'].shape == (3, 3, 1, 1, E_2004)
    assert list(tq['n_days']) == [366] and tq['info']['n_sweeps'] >= 1
    matches_numpy(tq, series_from_table(res, SERIES, A, f), Q_BAND)


def bits_equal(a, b):
    for k in ('data', 'lower', 'upper'):
        assert np.array_equal(a[k].view(np.int64), b[k].view(np.int64)), k
    assert np.array_equal(a['n_days'], b['n_days'])


def test_keep_daily_false_streams_nothing(run_2004):
    res = call('tarland_2004_dynamic', E_2004, time_quantiles=Q_BAND, time_quantile_series=SERIES, keep_daily=False)
    assert res['data'] is None and res['stats']['streamed_chunks'] == 0
    bits_equal(res['time_quantiles'], run_2004[0]['time_quantiles'])


def test_slot_order_with_balancing_gives_the_same_rows(run_2004):
    res = call('tarland_2004_dynamic', E_2004, time_quantiles=Q_BAND, time_quantile_series=SERIES,
               solver=dict(out_slot_order=1, balance=1))
    bits_equal(res['time_quantiles'], run_2004[0]['time_quantiles'])


def test_two_contexts_concatenate(run_2004):
    res = call('tarland_2004_dynamic', E_2004, time_quantiles=Q_BAND, time_quantile_series=SERIES, devices=[0, 0])
    assert len(res['stats']['bounds']) == 2 and res['stats']['bounds'][-1][1] == E_2004
    bits_equal(res['time_quantiles'], run_2004[0]['time_quantiles'])
    assert np.array_equal(res['data'], run_2004[0]['data'])


def test_default_series_are_the_outputs(engine0):
    res = call('tarland_2004_dynamic', 65, time_quantiles=[0.5], met_slice=slice(0, 90))
    tq = res['time_quantiles']
    assert tq['series'] == list(marshal.REACH5_COLUMNS) == res['columns']
    matches_numpy(tq, res['data'], [0.5])


E_LONG = 70


@pytest.fixture(scope='module')
def run_long(engine0):
    name = 'tarland_1981_2010_dynamic'
    res = call(name, E_LONG, time_quantiles=Q_BAND, time_quantile_series=SERIES, time_quantile_periods='annual')
    A = float(helpers.scenario_inputs(name)[4].loc['A_catch', 1])
    return res, A, overrides_for(name, E_LONG)['f_TDP']


def test_annual_periods_equal_numpy_per_calendar_year(run_long):
    res, A, f = run_long
    tq = res['time_quantiles']
    years = np.asarray(helpers.scenario_inputs('tarland_1981_2010_dynamic')[0].index.year)
    assert list(tq['periods']) == list(range(1981, 2011)) and tq['data'].shape == (3, 3, 30, 1, E_LONG)
    assert list(tq['n_days']) == [int((years == y).sum()) for y in range(1981, 2011)]
    matches_numpy(tq, series_from_table(res, SERIES, A, f), Q_BAND, pod=years - 1981)


def test_annual_windows_yield_the_rows_of_the_one_call(run_long):
    one = run_long[0]['time_quantiles']
    items = call('tarland_1981_2010_dynamic', E_LONG, windows='annual', time_quantiles=Q_BAND, time_quantile_series=SERIES,
                 keep_daily=False)
    assert len(items) == 30
    for p, w in enumerate(items):
        tq = w['time_quantiles']
        assert w['data'] is None and tq['data'].shape == (3, 3, 1, 1, E_LONG) and list(tq['n_days']) == [one['n_days'][p]]
        for k in ('data', 'lower', 'upper'):
            assert np.array_equal(tq[k][:, :, 0].view(np.int64), one[k][:, :, p].view(np.int64)), (p, k)


def test_band_across_members_of_the_per_member_statistics(run_2004):
    q_band = [0.025, 0.975]
    res = call('tarland_2004_dynamic', E_2004, time_quantiles=Q_BAND, time_quantile_series=SERIES, quantiles=q_band)
    bits_equal(res['time_quantiles'], run_2004[0]['time_quantiles'])
    band = res['time_quantiles']['quantiles']
    assert band['q'] == q_band and band['n_members'] == E_2004 and band['data'].shape == (2, 3, 3, 1, 1)
    same(band['data'], np.quantile(res['time_quantiles']['data'], q_band, axis=-1, method='linear'))
    assert res['quantiles']['data'].shape == (2, len(res['columns']), 366, 1)      # the daily band is still there


def test_poisoned_member_is_left_out_of_the_band_and_sorted_last_in_its_own_rows(run_2004):
    _, A, f = run_2004
    over = overrides_for('tarland_2004_dynamic', E_2004)
    over['T_g'] = over['T_g'].copy()
    over['T_g'][7] = np.nan                                                # marshal.validate_ensemble does not look at T_g
    q_band = [0.025, 0.975]
    res = call('tarland_2004_dynamic', E_2004, over=over, time_quantiles=Q_BAND + [1.0], time_quantile_series=SERIES, quantiles=q_band)
    bad = (res['status'] & abi.STATUS_NONFINITE) != 0
    assert np.flatnonzero(bad).tolist() == [7]
    tq = res['time_quantiles']
    keep = np.flatnonzero(~bad)
    matches_numpy(tq, series_from_table(res, SERIES, A, f), Q_BAND + [1.0], members=keep)   # np.sort puts the member's NaN last too
    assert np.isnan(tq['upper'][3, :, 0, 0, 7]).all()                              # q = 1 of the poisoned member
    assert np.isfinite(tq['data'][..., keep]).all()
    band = tq['quantiles']
    assert band['n_members'] == E_2004 - 1
    same(band['data'], np.quantile(tq['data'][..., keep], q_band, axis=-1, method='linear'))
