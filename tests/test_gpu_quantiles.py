"""Ensemble percentile bands selected on the device (simplyp_quantiles): the order statistics against np.sort on made-up
tables of every shape the two kernels take, the member mask and slot order, determinism, and the band through
run_simply_p_ensemble against np.quantile on the table the same call returns.  Rows built to sit on the select's list limit
and a table with more rows than the select's grid has workgroups also pin n_passes to tests/selection_model.py's count.

Bounds: order statistics are elements of their rows -- compared as values, exactly (np.array_equal; -0.0 == +0.0, NaN ==
NaN).  The interpolated band against np.quantile: 4 * eps * max(|lo|, |hi|) absolute -- three roundings (difference,
product, sum) of quantities of magnitude at most 2 max(|lo|, |hi|); see tests/test_quantiles_host.py."""

import ctypes as C

import numpy as np
import pytest

import helpers
import selection_cases as sc
import selection_model as sm
import simplyp_amd as sp
from simplyp_amd import abi, engine, marshal

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
Q_FIXED = [0.0, 0.025, 0.5, 0.975, 1.0]
Q_BAND = [0.025, 0.5, 0.975]


def q_random():
    return list(np.random.default_rng(2016).uniform(0.0, 1.0, 16))


def expected(table, q, keep=None):
    """np.sort's view: (lower, upper [K, n_rows], n) of table [n_rows, E] over the kept columns."""
    x = table if keep is None else table[:, keep]
    n = x.shape[1]
    if n == 0:
        nan = np.full((len(q), table.shape[0]), np.nan)
        return nan, nan, 0
    s = np.sort(x, axis=1)                                                 # NaN last
    h = np.asarray(q, dtype=np.float64) * np.float64(n - 1)
    k_lo = np.floor(h).astype(np.int64)
    k_hi = np.minimum(k_lo + 1, n - 1)
    return s[:, k_lo].T, s[:, k_hi].T, n


def make_table(kind, n_rows, E, rng):
    if kind == 'normal':                                                   # mixed signs, rows of different scales
        return rng.normal(size=(n_rows, E)) * 10.0 ** rng.integers(-3, 4, size=(n_rows, 1))
    if kind == 'ties':                                                     # 5 distinct numbers
        return rng.choice(np.array([-3.5, -0.0, 0.0, 2.0 ** -1040, 7.25e11]), size=(n_rows, E))
    if kind == 'constant':
        return np.repeat(rng.normal(size=(n_rows, 1)), E, axis=1)
    assert kind == 'special'                                               # +-inf, denormals, signed zeros, NaN of both signs
    t = rng.normal(size=(n_rows, E))
    specials = np.array([np.inf, -np.inf, 5e-324, -5e-324, 1e-310, -1e-310, -0.0, 0.0, np.nan, -np.nan,
                         np.finfo(np.float64).max, -np.finfo(np.float64).max])
    hit = rng.random(size=(n_rows, E)) < 0.3
    t[hit] = rng.choice(specials, size=int(hit.sum()))
    return t


def check(engine0, table, q, include=None, perm=None):
    """Engine.quantiles on `table` [n_rows, E] (numpy) against np.sort.  perm: member_of_slot -- the table handed to the
    device has member perm[j] in column j."""
    import torch
    dev_table = table if perm is None else table[:, perm]
    t = torch.from_numpy(np.ascontiguousarray(dev_table)).to(engine0.tdev)
    mos = None if perm is None else torch.from_numpy(np.ascontiguousarray(perm, dtype=np.int32)).to(engine0.tdev)
    lower, upper, info = engine0.quantiles(t, q, include=include, member_of_slot=mos)
    want_lo, want_hi, n = expected(table, q, None if include is None else np.flatnonzero(include))
    assert tuple(lower.shape) == tuple(upper.shape) == (len(q), table.shape[0])
    assert info['n_used'] == n and info['bytes_table'] == table.size * 8
    lo, hi = lower.cpu().numpy(), upper.cpu().numpy()
    assert np.array_equal(lo, want_lo, equal_nan=True), (np.argwhere(~((lo == want_lo) | (np.isnan(lo) & np.isnan(want_lo))))[:5])
    assert np.array_equal(hi, want_hi, equal_nan=True), (np.argwhere(~((hi == want_hi) | (np.isnan(hi) & np.isnan(want_hi))))[:5])
    return info


@pytest.mark.parametrize('E', [1, 2, 63, 64, 65, 1000, 2048, 4096, 4097, 9000, 100000])
@pytest.mark.parametrize('n_rows', [1, 7, 300])
def test_order_statistics_are_exact(engine0, E, n_rows):
    rng = np.random.default_rng(1000 * n_rows + E)
    for kind in ('normal', 'ties', 'constant', 'special'):
        table = make_table(kind, n_rows, E, rng)
        for q in (Q_FIXED, q_random()):
            info = check(engine0, table, q)
            assert 1 <= info['n_passes'] <= 8


def test_few_very_long_rows(engine0):
    rng = np.random.default_rng(5)
    table = np.exp(rng.normal(size=(4, 1200000)))
    table[1] = rng.choice(np.array([1.0, 2.0, 3.0]), size=1200000)
    check(engine0, table, Q_FIXED)
    check(engine0, table, q_random())


def model_of(table, q):
    """tests/selection_model.py on every row: (lower, upper [K, n_rows], the largest sweep count)."""
    k_lo, k_hi = sm.linear_ranks(q, table.shape[1])
    got = [sm.member_select(row, np.concatenate([k_lo, k_hi])) for row in table]
    v = np.stack([g[0] for g in got], axis=1)
    return v[:len(q)], v[len(q):], max(g[1] for g in got)


@pytest.mark.parametrize('case', sc.member_cases(), ids=lambda c: c[0])
@pytest.mark.parametrize('n_rows', [1, 3, 17])
def test_rows_on_the_list_limit(engine0, case, n_rows):
    """QLIST = 64, the bucket size at which quantile_select_kernel stops refining and collects: rows of E = 4097 (the shortest
    the select takes) whose wanted buckets hold exactly 64 or 65 members after the first digit.  n_passes tells the path:
    2 = first digit, collect; 3 = the 65 part in the second digit; 4 = they share it and part in the third; with two groups of
    64 and 65 the collect waits for the larger (3), unless no rank lies in it (2).  tests/selection_cases.py derives the numbers."""
    name, n_top, n_far, narrow, probs, sweeps = case
    table = sc.member_table(case, n_rows, np.random.default_rng(100 * n_rows + len(name)))
    assert table.shape == (n_rows, sm.QSORT_MAX + 1)
    info = check(engine0, table, probs)
    lo, hi, model_sweeps = model_of(table, probs)
    want_lo, want_hi, _ = expected(table, probs)
    assert np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi)
    assert info['n_passes'] == model_sweeps == sweeps


@pytest.fixture(scope='module')
def capped(engine0):
    """65536 + 36 rows of 4097 members (2.15 GB), made on the device from six base rows and a power of two per row."""
    import torch
    rng = np.random.default_rng(65536)
    base = sc.base_rows(sc.E_SELECT, sm.QLIST, rng)
    kind, scale = sc.capped_rows(65536, len(base), rng)
    table = torch.from_numpy(base).to(engine0.tdev)[torch.from_numpy(kind).to(engine0.tdev)]
    table.mul_(torch.from_numpy(scale).to(engine0.tdev)[:, None])
    made = dict(base=base, kind=kind, scale=scale, table=table)
    del table
    yield made
    made.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize('q', [Q_FIXED, q_random()], ids=['K=5', 'K=16'])
def test_rows_past_the_grid_cap(engine0, capped, q):
    """select_launch caps the grid at 65536 workgroups and radix_select strides over the rows (r += gridDim.x), carrying
    collect, G, prefix, count and list_n in LDS from one row to the next behind one barrier.  Workgroup i < 36 selects row i
    and then row 65536 + i: every ordered pair of six kinds of row (distinct, ties, flat, specials, wanted bucket of 64, of 65).
    A power of two scales order statistics exactly, so the expected values are the base rows' times the row's scale.  The
    flat rows take all 8 digits at any scale, so n_passes is 8: the model's maximum over the kinds."""
    base, kind, scale, table = capped['base'], capped['kind'], capped['scale'], capped['table']
    N = len(kind)
    assert N == 65536 + 36 and tuple(table.shape) == (N, 4097)
    assert {(int(kind[i]), int(kind[65536 + i])) for i in range(36)} == {(a, b) for a in range(6) for b in range(6)}
    lower, upper, info = engine0.quantiles(table, q)
    lo, hi, model_sweeps = model_of(base, q)
    want_lo, want_hi, _ = expected(base, q)
    assert np.array_equal(lo, want_lo, equal_nan=True) and np.array_equal(hi, want_hi, equal_nan=True)
    for got, want in ((lower, want_lo), (upper, want_hi)):
        got, want = got.cpu().numpy(), want[:, kind] * scale
        assert got.shape == want.shape == (len(q), N)
        assert np.array_equal(got, want, equal_nan=True), np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5]
    assert info['n_passes'] == model_sweeps == 8 and info['n_used'] == 4097 and info['bytes_table'] == N * 4097 * 8


@pytest.mark.parametrize('E', [65, 1000, 4096, 4097, 20000])
def test_member_mask_and_slot_order(engine0, E):
    rng = np.random.default_rng(E)
    table = make_table('special', 23, E, rng)
    mask = rng.random(E) < 0.6
    perm = rng.permutation(E).astype(np.int32)
    # column j of the device table holds member perm[j]; numpy's view of it: table[:, inv_perm][:, mask] of the device table
    dev = table[:, perm]
    inv = np.argsort(perm)
    assert np.array_equal(dev[:, inv][:, mask], table[:, mask], equal_nan=True)
    for q in (Q_FIXED, q_random()):
        check(engine0, table, q, include=mask, perm=perm)
        check(engine0, table, q, include=mask)
        check(engine0, table, q, perm=perm)
    info = check(engine0, table, Q_FIXED, include=np.zeros(E, dtype=bool), perm=perm)
    assert info['n_used'] == 0
    one = np.zeros(E, dtype=bool); one[E // 2] = True
    check(engine0, table, Q_FIXED, include=one, perm=perm)


@pytest.mark.parametrize('E', [1000, 50000])
def test_deterministic_and_table_untouched(engine0, E):
    import torch
    rng = np.random.default_rng(E + 1)
    t = torch.from_numpy(make_table('special', 40, E, rng)).to(engine0.tdev)
    before = t.view(torch.int64).clone()
    mask = rng.random(E) < 0.5
    a = engine0.quantiles(t, q_random(), include=mask)
    b = engine0.quantiles(t, q_random(), include=mask)
    for x, y in zip(a[:2], b[:2]):
        assert bool(torch.equal(x.view(torch.int64), y.view(torch.int64)))
    assert bool(torch.equal(t.view(torch.int64), before))


def test_argument_errors(engine0):
    import torch
    L = engine.lib()
    E, n_rows = 100, 3
    t = torch.zeros((n_rows, E), dtype=torch.float64, device=engine0.tdev)
    out = torch.full((2, 16, n_rows), -7.0, dtype=torch.float64, device=engine0.tdev)
    info = abi.QuantileInfo()

    def call(E_=E, n_rows_=n_rows, table=True, q=(0.5,), K=None, stats=True):
        qa = None if q is None else np.ascontiguousarray(q, dtype=np.float64)
        with torch.cuda.device(engine0.tdev):
            return L.simplyp_quantiles(engine0._h, E_, n_rows_, t.data_ptr() if table else None, None, None,
                                       None if qa is None else qa.ctypes.data_as(C.POINTER(C.c_double)),
                                       (0 if qa is None else len(qa)) if K is None else K,
                                       out.data_ptr() if stats else None, C.byref(info))
    bad = [dict(q=(), K=0), dict(q=[0.5] * 17), dict(q=(-1e-9,)), dict(q=(1.0 + 1e-9,)), dict(q=(0.5, np.nan)),
           dict(E_=0), dict(n_rows_=-1), dict(table=False), dict(q=None, K=1), dict(stats=False)]
    for kw in bad:
        assert call(**kw) == -1, kw                                        # SIMPLYP_ERR_ARG
        assert b'simplyp_quantiles' in L.simplyp_last_error(engine0._h), kw
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())                                       # nothing was written
    assert call(n_rows_=0) == 0 and bool((out == -7.0).all())              # no rows: succeeds, launches nothing
    assert call() == 0 and bool((out.flatten()[:2 * n_rows] == 0.0).all()) and bool((out.flatten()[2 * n_rows:] == -7.0).all())
    with pytest.raises(ValueError):
        engine0.quantiles(t[:, ::2], [0.5])                                # not contiguous


# ---- through the public call ----------------------------------------------------------------------------------------------

E_PUBLIC = 4097


def overrides_for(name, E, seed=3):
    """a_Q, T_g, E_M, fc of the scenario's workbook scaled by seeded uniform factors (the ranges of
    tests/test_gpu_gof.py::perturbed_run), as `overrides`."""
    base = helpers.marshal_scenario(name, E=1)['member_params'][:, 0]
    rng = np.random.default_rng(seed)
    return {pname: base[marshal.PM_NAMES.index(pname)] * rng.uniform(lo, hi, E)
            for pname, lo, hi in (('a_Q', 0.6, 1.6), ('T_g', 0.7, 1.4), ('E_M', 0.5, 2.0), ('fc', 0.85, 1.15))}


def tarland_call(name='tarland_2004_dynamic', over=None, **kw):
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(name)
    return sp.run_simply_p_ensemble(met, p_struc, p_SU, p_LU, p_SC, p, dyn,
                                    overrides=overrides_for(name, E_PUBLIC) if over is None else over, **kw)


def band_matches_numpy(band, table, q, keep=None):
    x = table if keep is None else table[..., keep]
    want = np.quantile(x, q, axis=-1)
    assert band['data'].shape == want.shape
    tol = 4 * EPS * np.maximum(np.abs(band['lower']), np.abs(band['upper']))
    err = np.abs(band['data'] - want)
    assert bool((err <= tol).all()), float((err / np.maximum(tol, 1e-300)).max())
    s = np.sort(x, axis=-1)
    n = x.shape[-1]
    k_lo = np.floor(np.asarray(q) * np.float64(n - 1)).astype(np.int64)
    assert np.array_equal(band['lower'], np.stack([s[..., k] for k in k_lo]))
    assert np.array_equal(band['upper'], np.stack([s[..., k] for k in np.minimum(k_lo + 1, n - 1)]))


@pytest.fixture(scope='module')
def base_run(engine0):
    obs_dict = helpers.observations('2004-01-01', '2004-12-31')
    return tarland_call(quantiles=Q_BAND, obs_dict=obs_dict)


def test_band_of_the_daily_table(base_run):
    res = base_run
    assert res['data'].shape == (5, 366, 1, E_PUBLIC) and np.isfinite(res['data']).all() and (res['status'] & abi.STATUS_NONFINITE == 0).all()
    band = res['quantiles']
    assert band['q'] == Q_BAND and band['n_members'] == E_PUBLIC and band['info']['n_used'] == E_PUBLIC
    assert band['data'].shape == (3, 5, 366, 1)
    band_matches_numpy(band, res['data'], Q_BAND)


def test_keep_daily_false_streams_nothing(base_run):
    res = tarland_call(quantiles=Q_BAND, keep_daily=False)
    assert res['data'] is None and res['stats']['streamed_chunks'] == 0
    for k in ('data', 'lower', 'upper'):
        assert np.array_equal(res['quantiles'][k].view(np.int64), base_run['quantiles'][k].view(np.int64)), k


def test_slot_order_with_balancing_gives_the_same_band(base_run):
    res = tarland_call(quantiles=Q_BAND, keep_daily=False, solver=dict(out_slot_order=1, balance=1, balance_pilot_days=60))
    assert res['stats']['balanced'] == 1
    for k in ('data', 'lower', 'upper'):
        assert np.array_equal(res['quantiles'][k].view(np.int64), base_run['quantiles'][k].view(np.int64)), k


def test_band_of_annual_sums(engine0):
    name = 'tarland_1981_2010_dynamic'
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(name)
    met = met.iloc[:1095]                                                  # 1981-1983
    assert list(np.unique(met.index.year)) == [1981, 1982, 1983]
    res = sp.run_simply_p_ensemble(met, p_struc, p_SU, p_LU, p_SC, p, dyn, overrides=overrides_for(name, E_PUBLIC),
                                   reduce='annual', quantiles=Q_BAND)
    assert res['data'].shape == (5, 3, 1, E_PUBLIC) and np.isfinite(res['data']).all()
    assert res['quantiles']['data'].shape == (3, 5, 3, 1)
    band_matches_numpy(res['quantiles'], res['data'], Q_BAND)


def test_waterbody_band(engine0):
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs('confluence3_nc_2004')
    E = 1000
    rng = np.random.default_rng(2)
    over = dict(fc=290 * rng.uniform(0.9, 1.1, E), f_TDP=rng.uniform(0.5, 0.9, E))
    res = sp.run_simply_p_ensemble(met, p_struc, p_SU, p_LU, p_SC, p, dyn, overrides=over, waterbody=[1, 3], quantiles=Q_BAND)
    wb = res['waterbody']
    assert wb['data'].shape == (11, 366, E) and np.isfinite(wb['data']).all()
    assert wb['quantiles']['data'].shape == (3, 11, 366) and wb['quantiles']['n_members'] == E
    band_matches_numpy(wb['quantiles'], wb['data'], Q_BAND)
    band_matches_numpy(res['quantiles'], res['data'], Q_BAND)


def test_poisoned_member_is_left_out(base_run):
    over = overrides_for('tarland_2004_dynamic', E_PUBLIC)
    over['T_g'] = over['T_g'].copy()
    over['T_g'][7] = np.nan                                                # marshal.validate_ensemble does not look at T_g
    res = tarland_call(over=over, quantiles=Q_BAND)
    bad = (res['status'] & abi.STATUS_NONFINITE) != 0
    assert np.flatnonzero(bad).tolist() == [7]                             # the only non-finite member ...
    keep = np.flatnonzero(~bad)
    assert np.isfinite(res['data'][..., keep]).all() and not np.isfinite(res['data'][..., 7]).all()   # ... in the table too
    assert res['quantiles']['n_members'] == E_PUBLIC - 1
    band_matches_numpy(res['quantiles'], res['data'], Q_BAND, keep=keep)


def test_behavioural_members_from_the_gof_table(base_run):
    g = base_run['gof']
    nse = g['data'][g['stats'].index('NSE'), g['variables'].index('Q'), 0, :]
    assert np.isfinite(nse).all()
    members = nse > np.median(nse)
    assert 0 < members.sum() < E_PUBLIC
    res = tarland_call(quantiles=Q_BAND, quantile_members=members)
    assert np.array_equal(res['data'], base_run['data'])
    assert res['quantiles']['n_members'] == int(members.sum())
    band_matches_numpy(res['quantiles'], res['data'], Q_BAND, keep=np.flatnonzero(members))
