"""Predictive bands on the device (simplyp_predictive_series, simplyp_predictive_bands): the normals against the NumPy mirror
of the stream (simplyp_amd/predictive.py), the generated values against the error model applied in NumPy to the device's own
normals, the bands against np.sort of the device-made table, the distribution of the overall band against the normal
quantiles it must reproduce, argument errors, and the public call.

Tolerances.
* z, device against mirror: |dz| <= 2^-45.  The integers are exact; what differs is the device's cospi(2u) against the
  mirror's, an argument rounding of at most 2 pi eps times r <= 8.58, plus about 1 ulp each for log and sqrt -- about 60 eps,
  doubled.  The test prints the measured maximum.
* values and order statistics: bit for bit (a NaN matches a NaN; among order statistics a zero matches a zero of either sign,
  as in tests/test_gpu_quantiles.py).
* the interpolated band against np.quantile: 4 eps max(|lo|, |hi|), the rule of tests/test_gpu_quantiles.py.
* distribution: five standard errors of a sample quantile of n = 100 000 draws of N(1, 0.1^2),
  0.1 sqrt(p (1 - p) / n) / phi(z_p): 4.3e-3 at p = 0.025 / 0.975, 2.0e-3 at the median."""

import ctypes as C

import numpy as np
import pytest

import helpers
import simplyp_amd as sp
from simplyp_amd import abi, engine, marshal, predictive

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
COL = {c: i for i, c in enumerate(marshal.ALL_COLUMNS)}
FLUX4 = ['Qr', 'Msus_kg/day', 'TDP_kg/day', 'PP_kg/day']
MASK5 = marshal.mask_of_columns(['Vr'] + FLUX4)
DERIVED = [abi.TQ_DERIVED + v for v in range(6)]
SERIES8 = [COL['Vr'], COL['Qr']] + DERIVED
SERIES3 = [COL['Vr'], DERIVED[0], DERIVED[4]]
Q_BAND = [0.025, 0.5, 0.975]
S, OUT_REACHES = 3, [0, 2]
SEED = (7 << 32) | 5
DAY0 = 1000


def dev(engine0, a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(engine0.tdev)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def same(got, want, zeros=False):
    """Bit for bit; a NaN matches a NaN; zeros=True: a zero matches a zero of either sign (order statistics)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    ok = (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))
    if zeros:
        ok |= (got == 0.0) & (want == 0.0)
    assert bool(ok.all()), (int((~ok).sum()), np.argwhere(~ok)[:5], got[~ok][:5], want[~ok][:5])
    return True


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


def problem(D, E, seed=0, special=True):
    """A made-up table [5, D, 2, E] of three model reaches' worth of parameters, output reaches 0 and 2."""
    rng = np.random.default_rng(1000 * D + E + seed)
    R = len(OUT_REACHES)
    table = np.exp(rng.normal(size=(5, D, R, E)))
    table[2:] *= 10.0 ** rng.integers(-2, 3, size=(3, 1, 1, 1))
    if special:                                                            # rows with NaN, 0, negative and inf values
        specials = np.array([np.nan, 0.0, -0.0, -1.5, np.inf, -np.inf])
        hit = rng.random(size=table.shape) < 0.08
        table[hit] = rng.choice(specials, size=int(hit.sum()))
    A = rng.uniform(5.0, 80.0, size=(S, E))
    f = rng.uniform(0.3, 0.95, size=E)
    rp = np.zeros((len(marshal.PR_NAMES), S, E))
    rp[marshal.PR_NAMES.index('A_catch')] = A
    return dict(table=table, A=A, f=f, rp=rp, D=D, E=E, kw=dict(f_tdp=f, reach_params=rp, out_reaches=OUT_REACHES))


def values_numpy(pr, series):
    """v [n_series, D, R, E] of the series ids."""
    d = derived_numpy(pr['table'], pr['A'][OUT_REACHES], pr['f'])
    cols = [c for c in range(26) if (MASK5 >> c) & 1]
    return np.stack([d[s - abi.TQ_DERIVED] if s >= abi.TQ_DERIVED else pr['table'][cols.index(s)] for s in series])


def mirror_z(series, D, E, seed=SEED, day0=DAY0, members=None):
    m = np.arange(E) if members is None else np.asarray(members)
    return predictive.standard_normal(seed, m[None, None, None, :], (day0 + np.arange(D))[None, :, None, None],
                                      np.asarray(OUT_REACHES)[None, None, :, None], np.asarray(series)[:, None, None, None])


def device_z(engine0, pr, series, seed=SEED, day0=DAY0, **kw):
    return engine0.predictive_series(dev(engine0, pr['table']), MASK5, series, err_m=0.1, seed=seed, day0=day0, normals=True,
                                     **dict(pr['kw'], **kw)).cpu().numpy()


def err_model(series, E, seed=0):
    return np.random.default_rng(seed).uniform(0.02, 0.4, size=(len(series), E))


# ---- the normals ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('E', [1, 63, 64, 65, 200])
def test_normals_match_the_mirror(engine0, E):
    worst = 0.0
    for D in (3, 70):
        pr = problem(D, E)
        got = device_z(engine0, pr, SERIES8)
        want = mirror_z(SERIES8, D, E)
        assert got.shape == want.shape == (8, D, 2, E)
        worst = max(worst, float(np.abs(got - want).max()))
    print('max |z_device - z_mirror| = %.3e = %.1f eps (E = %d)' % (worst, worst / EPS, E))
    assert worst <= 2.0 ** -45


def test_normals_belong_to_the_member_not_the_slot(engine0):
    pr = problem(70, 200)
    perm = np.random.default_rng(4).permutation(200).astype(np.int32)      # slot j holds member perm[j]
    z_m = device_z(engine0, pr, SERIES8)
    z_s = device_z(engine0, pr, SERIES8, member_of_slot=dev(engine0, perm))
    assert np.array_equal(bits(z_s), bits(z_m[..., perm]))


def test_normals_belong_to_the_absolute_day(engine0):
    pr = problem(70, 65)
    z0 = device_z(engine0, pr, SERIES8, day0=0)
    z7 = device_z(engine0, pr, SERIES8, day0=7)
    assert np.array_equal(bits(z7[:, :63]), bits(z0[:, 7:]))
    assert not (z7 == z0).any()


def test_reach_series_and_seed_enter(engine0):
    pr = problem(70, 65)
    z = device_z(engine0, pr, SERIES8)
    assert not (z[:, :, 0] == z[:, :, 1]).any()                            # model reaches 0 and 2
    for i in range(8):
        for j in range(i):
            assert not (z[i] == z[j]).any(), (i, j)
    assert not (device_z(engine0, pr, SERIES8, seed=SEED + 1) == z).any()
    assert not (device_z(engine0, pr, SERIES8, seed=SEED + (1 << 32)) == z).any()
    # the reach is the model's id, not the row: reach 2 alone draws what it drew as the second row
    sub = dict(pr, table=np.ascontiguousarray(pr['table'][:, :, 1:]), kw=dict(pr['kw'], out_reaches=[2]))
    assert np.array_equal(bits(device_z(engine0, sub, SERIES8)[:, :, 0]), bits(z[:, :, 1]))
    # the series is the id as passed, not the position in the list
    assert np.array_equal(bits(device_z(engine0, pr, SERIES8[::-1])), bits(z[::-1]))


# ---- the values -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('D,E', [(3, 65), (70, 200)])
def test_values_are_the_error_model_on_the_device_normals(engine0, D, E):
    pr = problem(D, E)
    t = dev(engine0, pr['table'])
    v = values_numpy(pr, SERIES8)
    for kind in ('nan', 'zero', 'neg', 'inf'):                             # every kind of special row is there
        pick = {'nan': np.isnan(v), 'zero': v == 0, 'neg': v < 0, 'inf': np.isinf(v)}[kind]
        assert pick.any(), kind
    same(engine0.predictive_series(t, MASK5, SERIES8, **pr['kw']).cpu().numpy(), v)          # err_m NULL: the series itself
    m = err_model(SERIES8, E)
    z = device_z(engine0, pr, SERIES8)
    got = engine0.predictive_series(t, MASK5, SERIES8, err_m=m, seed=SEED, day0=DAY0, **pr['kw']).cpu().numpy()
    same(got, predictive.perturb(v, m[:, None, None, :], z))
    # slot order: err_m, f_tdp and A_catch are looked up by member
    perm = np.random.default_rng(E).permutation(E).astype(np.int32)
    got_s = engine0.predictive_series(dev(engine0, pr['table'][..., perm]), MASK5, SERIES8, err_m=m, seed=SEED, day0=DAY0,
                                      member_of_slot=dev(engine0, perm), **pr['kw']).cpu().numpy()
    same(got_s, got[..., perm])


def test_days_past_the_grid_cap(engine0):
    """predictive_launch caps grid.y at 65535 batches of 4 days and pred_days strides over the rest
    (d0 += gridDim.y * PRED_BATCH): D = 4 * 65535 + 7 days in one launch give the first two batches a second trip, the last
    of them a partial one.  Day 262 140 is the first day of the second trip: its counter must be day0 + 262 140, its row its own."""
    D, E, first = 4 * 65535 + 7, 3, 4 * 65535
    pr = problem(D, E)
    table = np.ascontiguousarray(pr['table'][:, :, 1:])                    # one output reach: model reach 2
    kw = dict(pr['kw'], out_reaches=[2])
    series = [COL['Vr'], DERIVED[4]]                                       # a column and TP_mgl (three loads a day)
    t = dev(engine0, table)
    v = np.stack([table[0], derived_numpy(table, pr['A'][[2]], pr['f'])[4]])
    assert np.isnan(v[:, first - 1:first + 1]).sum() < v[:, first - 1:first + 1].size
    same(engine0.predictive_series(t, MASK5, series, **kw).cpu().numpy(), v)
    z = engine0.predictive_series(t, MASK5, series, err_m=0.1, seed=SEED, day0=DAY0, normals=True, **kw).cpu().numpy()
    want_z = predictive.standard_normal(SEED, np.arange(E)[None, None, None, :], (DAY0 + np.arange(D))[None, :, None, None],
                                        2, np.asarray(series)[:, None, None, None])
    assert z.shape == want_z.shape == (2, D, 1, E)
    worst = float(np.abs(z - want_z).max())
    print('max |z_device - z_mirror| = %.3e = %.1f eps over %d days' % (worst, worst / EPS, D))
    assert worst <= 2.0 ** -45
    assert float(np.abs(z[:, first - 1:first + 1] - want_z[:, first - 1:first + 1]).max()) <= 2.0 ** -45       # either side of the cap
    m = err_model(series, E)
    got = engine0.predictive_series(t, MASK5, series, err_m=m, seed=SEED, day0=DAY0, **kw).cpu().numpy()
    same(got, predictive.perturb(v, m[:, None, None, :], z))
    same(got[:, first - 1:first + 1], predictive.perturb(v, m[:, None, None, :], z)[:, first - 1:first + 1])


# ---- the bands --------------------------------------------------------------------------------------------------------------

def expected_stats(x, q, keep=None):
    """np.sort's view of x [..., E]: lower, upper [K, ...] and n."""
    x = x if keep is None else x[..., keep]
    n = x.shape[-1]
    if n == 0:
        nan = np.full((len(q),) + x.shape[:-1], np.nan)
        return nan, nan, 0
    s = np.sort(x, axis=-1)                                                # NaN last
    k_lo = np.floor(np.asarray(q, dtype=np.float64) * np.float64(n - 1)).astype(np.int64)
    k_hi = np.minimum(k_lo + 1, n - 1)
    return np.moveaxis(s[..., k_lo], -1, 0), np.moveaxis(s[..., k_hi], -1, 0), n


def bands(engine0, pr, t, q, series, m=None, **kw):
    lo, up, info = engine0.predictive_bands(t, MASK5, q, series, err_m=m, seed=SEED, day0=DAY0, **dict(pr['kw'], **kw))
    return lo.cpu().numpy(), up.cpu().numpy(), info


@pytest.mark.parametrize('E', [1, 64, 65, 1000, 4097, 5000])
def test_order_statistics_equal_np_sort_of_the_device_made_table(engine0, E):
    pr = problem(3, E)
    t = dev(engine0, pr['table'])
    q = Q_BAND + [0.0, 1.0, 0.31]
    for m in (None, err_model(SERIES3, E)):
        x = engine0.predictive_series(t, MASK5, SERIES3, err_m=m, seed=SEED, day0=DAY0, **pr['kw']).cpu().numpy()
        lo, up, info = bands(engine0, pr, t, q, SERIES3, m)
        want_lo, want_up, n = expected_stats(x, q)
        assert lo.shape == up.shape == (len(q), 3, 3, 2) and info['n_used'] == n == E and info['n_chunks'] == 1
        same(lo, want_lo, zeros=True)
        same(up, want_up, zeros=True)
        assert info['bytes_read'] == (1 + 1 + 3) * 3 * 2 * E * 8 and info['bytes_workspace'] == 3 * 3 * 2 * E * 8
        assert info['n_passes'] >= 1 and info['kernel_ms'] >= info['gen_ms'] > 0


@pytest.mark.parametrize('E', [65, 4097])
def test_result_does_not_depend_on_the_chunk_length(engine0, monkeypatch, E):
    pr = problem(70, E)
    t = dev(engine0, pr['table'])
    m = err_model(SERIES3, E)
    monkeypatch.delenv('SIMPLYP_PRED_CHUNK_DAYS', raising=False)
    lo, up, info = bands(engine0, pr, t, Q_BAND, SERIES3, m)
    assert info['n_chunks'] == 1
    x = engine0.predictive_series(t, MASK5, SERIES3, err_m=m, seed=SEED, day0=DAY0, **pr['kw']).cpu().numpy()
    want_lo, want_up, _ = expected_stats(x, Q_BAND)
    same(lo, want_lo, zeros=True)
    same(up, want_up, zeros=True)
    for days, chunks in ((32, 3), (1, 70), (70, 1), (1000, 1)):
        monkeypatch.setenv('SIMPLYP_PRED_CHUNK_DAYS', str(days))
        lo_c, up_c, info_c = bands(engine0, pr, t, Q_BAND, SERIES3, m)
        assert info_c['n_chunks'] == chunks and info_c['bytes_workspace'] == min(days, 70) * 3 * 2 * E * 8
        assert np.array_equal(bits(lo_c), bits(lo)) and np.array_equal(bits(up_c), bits(up)), days


def test_include_mask_slot_order_and_nobody_left(engine0):
    E = 200
    pr = problem(70, E)
    m = err_model(SERIES3, E)
    rng = np.random.default_rng(8)
    inc = rng.random(E) < 0.6
    t = dev(engine0, pr['table'])
    x = engine0.predictive_series(t, MASK5, SERIES3, err_m=m, seed=SEED, day0=DAY0, **pr['kw']).cpu().numpy()
    lo, up, info = bands(engine0, pr, t, Q_BAND, SERIES3, m, include=inc)
    want_lo, want_up, n = expected_stats(x, Q_BAND, keep=np.flatnonzero(inc))
    assert info['n_used'] == n == int(inc.sum())
    same(lo, want_lo, zeros=True)
    same(up, want_up, zeros=True)
    # the same members in another slot order: the mask, the error model and the draws follow the member
    perm = rng.permutation(E).astype(np.int32)
    lo_s, up_s, info_s = bands(engine0, pr, dev(engine0, pr['table'][..., perm]), Q_BAND, SERIES3, m, include=inc,
                               member_of_slot=dev(engine0, perm))
    assert info_s['n_used'] == n
    same(lo_s, lo, zeros=True)
    same(up_s, up, zeros=True)
    lo_0, up_0, info_0 = bands(engine0, pr, t, Q_BAND, SERIES3, m, include=np.zeros(E, dtype=bool))
    assert info_0['n_used'] == 0 and np.isnan(lo_0).all() and np.isnan(up_0).all() and lo_0.shape == lo.shape


def test_deterministic_and_table_untouched(engine0):
    import torch
    pr = problem(70, 4097)
    m = err_model(SERIES3, 4097)
    t = dev(engine0, pr['table'])
    before = t.view(torch.int64).clone()
    a = bands(engine0, pr, t, Q_BAND, SERIES3, m)
    b = bands(engine0, pr, t, Q_BAND, SERIES3, m)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
    assert a[2]['n_passes'] == b[2]['n_passes']
    assert bool(torch.equal(t.view(torch.int64), before))


def test_no_error_is_the_parameter_only_band(engine0):
    pr = problem(70, 300, special=False)
    t = dev(engine0, pr['table'])
    po = bands(engine0, pr, t, Q_BAND, SERIES8)
    ov = bands(engine0, pr, t, Q_BAND, SERIES8, 0.0)
    assert np.isfinite(po[0]).all()
    assert np.array_equal(bits(po[0]), bits(ov[0])) and np.array_equal(bits(po[1]), bits(ov[1]))


# ---- the distribution ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('seed', [2016, SEED])
def test_overall_band_of_a_constant_series_is_the_normal_band(engine0, seed):
    E, D = 100000, 4
    table = np.ones((1, D, 2, E))
    mask = 1 << COL['Qr']
    lo, up, info = engine0.predictive_bands(dev(engine0, table), mask, Q_BAND, [COL['Qr']], err_m=0.1, seed=seed,
                                            out_reaches=OUT_REACHES)
    data = engine.interpolate_quantiles(lo.cpu().numpy(), up.cpu().numpy(), Q_BAND, info['n_used'])
    assert data.shape == (3, 1, D, 2) and info['n_used'] == E
    want = np.array([1 - 0.196, 1.0, 1 + 0.196]).reshape(3, 1, 1, 1)
    bound = np.array([4.3e-3, 2.0e-3, 4.3e-3]).reshape(3, 1, 1, 1)
    err = np.abs(data - want)
    print('worst deviation of the 2.5 / 50 / 97.5 %% values: %s' % err.reshape(3, -1).max(axis=1))
    assert bool((err <= bound).all()), err.reshape(3, -1).max(axis=1)


# ---- argument errors ----------------------------------------------------------------------------------------------------------

def test_argument_errors(engine0):
    import torch
    L = engine.lib()
    E, D = 100, 40
    R = len(OUT_REACHES)
    t = torch.ones((5, D, R, E), dtype=torch.float64, device=engine0.tdev)
    stats = torch.full((2, 16, 32, D, R), -7.0, dtype=torch.float64, device=engine0.tdev)
    table = torch.full((32, D, R, E), -7.0, dtype=torch.float64, device=engine0.tdev)
    ft = torch.ones(E, dtype=torch.float64, device=engine0.tdev)
    rp = torch.ones((len(marshal.PR_NAMES), S, E), dtype=torch.float64, device=engine0.tdev)
    em = torch.full((32, E), 0.1, dtype=torch.float64, device=engine0.tdev)
    info = abi.PredInfo()
    i32 = C.POINTER(C.c_int32)
    oreach = np.ascontiguousarray(OUT_REACHES, dtype=np.int32)

    def head(mask, out, D_, E_):
        return (engine0._h, C.byref(abi.Dims(E_, S, D_, 1)), mask, oreach.ctypes.data_as(i32), R, t.data_ptr() if out else None, None)

    def series_args(f, r, series, n_series, m):
        sa = None if series is None else np.ascontiguousarray(series, dtype=np.int32)
        return sa, (ft.data_ptr() if f else None, rp.data_ptr() if r else None, None if sa is None else sa.ctypes.data_as(i32),
                    (0 if sa is None else len(sa)) if n_series is None else n_series, em.data_ptr() if m else None)

    def call_bands(mask=MASK5, out=True, f=True, r=True, series=(COL['Qr'],), n_series=None, m=True, day0=0, q=(0.5,), K=None,
                   res=True, D_=D, E_=E):
        qa = None if q is None else np.ascontiguousarray(q, dtype=np.float64)
        sa, mid = series_args(f, r, series, n_series, m)
        with torch.cuda.device(engine0.tdev):
            return L.simplyp_predictive_bands(*(head(mask, out, D_, E_) + (None,) + mid + (C.c_uint64(1), day0,
                                                None if qa is None else qa.ctypes.data_as(C.POINTER(C.c_double)),
                                                (0 if qa is None else len(qa)) if K is None else K,
                                                stats.data_ptr() if res else None, C.byref(info))))

    def call_series(mask=MASK5, out=True, f=True, r=True, series=(COL['Qr'],), n_series=None, m=True, day0=0, which=0, res=True,
                    D_=D, E_=E):
        sa, mid = series_args(f, r, series, n_series, m)
        with torch.cuda.device(engine0.tdev):
            return L.simplyp_predictive_series(*(head(mask, out, D_, E_) + mid + (C.c_uint64(1), day0, which,
                                                 table.data_ptr() if res else None)))

    no_flux = marshal.mask_of_columns(['Vr', 'Qr', 'TDP_kg/day', 'PP_kg/day'])
    shared = [dict(series=(), n_series=0), dict(series=[COL['Qr']] * 33), dict(series=None, n_series=1),      # n_series, NULL series
              dict(series=(COL['VsA'],)),                                  # a column that is not in the mask
              dict(series=(abi.TQ_DERIVED + 6,)), dict(series=(40,)), dict(series=(-1,)),
              dict(series=(DERIVED[0],), mask=no_flux),                    # derived without Msus_kg/day
              dict(series=(DERIVED[1],), mask=MASK5 & ~(1 << COL['Qr'])),  # derived without Qr
              dict(series=(DERIVED[5],), f=False), dict(series=(DERIVED[0],), r=False),
              dict(day0=-1), dict(out=False), dict(res=False),
              dict(D_=-1), dict(E_=0)]                                     # no table of daily rows
    only_bands = [dict(q=(), K=0), dict(q=[0.5] * 17), dict(q=(-1e-9,)), dict(q=(1.0 + 1e-9,)), dict(q=(0.5, np.nan)),
                  dict(q=None, K=1)]
    only_series = [dict(which=2), dict(which=-1), dict(which=1, m=False)]
    for kw in shared + only_bands:
        assert call_bands(**kw) == -1, kw                                  # SIMPLYP_ERR_ARG
        assert b'simplyp_predictive_bands' in L.simplyp_last_error(engine0._h), kw
    for kw in shared + only_series:
        assert call_series(**kw) == -1, kw
        assert b'simplyp_predictive_series' in L.simplyp_last_error(engine0._h), kw
    torch.cuda.synchronize()
    assert bool((stats == -7.0).all()) and bool((table == -7.0).all())     # nothing was written
    # D = 0 succeeds and writes nothing
    assert call_bands(D_=0) == 0 and call_series(D_=0) == 0
    torch.cuda.synchronize()
    assert bool((stats == -7.0).all()) and bool((table == -7.0).all())
    # valid calls afterwards work: K = 1, one series of ones with m = 0.1
    assert call_series() == 0 and call_bands() == 0
    flat = table.flatten()
    assert bool((flat[:D * R * E] != -7.0).all()) and bool((flat[D * R * E:] == -7.0).all())
    assert bool(((flat[:D * R * E] - 1.0).abs() <= 0.1 * 8.58).all())
    sflat = stats.flatten()
    assert bool((sflat[:2 * D * R] != -7.0).all()) and bool((sflat[2 * D * R:] == -7.0).all())
    assert info.n_used == E and info.n_chunks == 1
    with pytest.raises(ValueError):
        engine0.predictive_bands(t[..., ::2], MASK5, [0.5], [COL['Qr']])   # not contiguous
    with pytest.raises(ValueError):
        engine0.predictive_series(t, MASK5, [COL['Qr']], err_m=np.ones((2, E)))


# ---- through the public call ----------------------------------------------------------------------------------------------

NAME = 'tarland_2004_dynamic'
E_PUBLIC = 4097
NAMES = ['Q_cumecs', 'TDP_mgl']
M_PUBLIC = {'Q_cumecs': 0.1, 'TDP_mgl': 0.25}
SEED_PUBLIC = 2016


def overrides_for(name, E, seed=3):
    """a_Q, T_g, E_M, fc of the scenario's workbook scaled by seeded uniform factors (the ranges of
    tests/test_gpu_quantiles.py::overrides_for), as `overrides`."""
    base = helpers.marshal_scenario(name, E=1)['member_params'][:, 0]
    rng = np.random.default_rng(seed)
    return {pname: base[marshal.PM_NAMES.index(pname)] * rng.uniform(lo, hi, E)
            for pname, lo, hi in (('a_Q', 0.6, 1.6), ('T_g', 0.7, 1.4), ('E_M', 0.5, 2.0), ('fc', 0.85, 1.15))}


def public_call(windows=None, **kw):
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
    kw = dict(dict(overrides=overrides_for(NAME, E_PUBLIC), quantiles=Q_BAND, predictive_series=NAMES, predictive_m=M_PUBLIC,
                   predictive_seed=SEED_PUBLIC), **kw)
    if windows is not None:
        return list(sp.run_simply_p_ensemble_windows(met, p_struc, p_SU, p_LU, p_SC, p, dyn, window=windows, **kw))
    return sp.run_simply_p_ensemble(met, p_struc, p_SU, p_LU, p_SC, p, dyn, **kw)


@pytest.fixture(scope='module')
def base_run(engine0):
    return public_call()


def test_public_param_only_band_equals_numpy_on_the_returned_table(base_run):
    res = base_run
    assert (res['status'] & abi.STATUS_NONFINITE == 0).all()
    assert set(FLUX4) <= set(res['columns']) and res['data'].shape[1:] == (366, 1, E_PUBLIC)
    pred = res['predictive']
    assert pred['q'] == Q_BAND and pred['series'] == NAMES and pred['n_members'] == E_PUBLIC
    assert pred['seed'] == SEED_PUBLIC and pred['day0'] == 0
    A = float(helpers.scenario_inputs(NAME)[4].loc['A_catch', 1])
    col = lambda c: res['data'][res['columns'].index(c)]
    x = np.stack([col('Qr') * A * 1000 / 86400, (col('TDP_kg/day') / col('Qr')) / A])
    band = pred['param_only']
    want = np.quantile(x, Q_BAND, axis=-1)
    assert band['data'].shape == want.shape == (3, 2, 366, 1)
    tol = 4 * EPS * np.maximum(np.abs(band['lower']), np.abs(band['upper']))
    err = np.abs(band['data'] - want)
    assert bool((err <= tol).all()), float((err / np.maximum(tol, 1e-300)).max())
    want_lo, want_up, _ = expected_stats(x, Q_BAND)
    assert np.array_equal(band['lower'], want_lo) and np.array_equal(band['upper'], want_up)


def test_public_overall_band_equals_np_sort_of_the_realisations(engine0, base_run):
    res = base_run
    sc = helpers.scenario_inputs(NAME)
    A = float(sc[4].loc['A_catch', 1])
    rp = np.zeros((len(marshal.PR_NAMES), 1, E_PUBLIC))
    rp[marshal.PR_NAMES.index('A_catch')] = A
    ids = [abi.TQ_DERIVED + abi.TQ_DERIVED_SERIES.index(n) for n in NAMES]
    m = np.stack([np.full(E_PUBLIC, M_PUBLIC[n]) for n in NAMES])
    x = engine0.predictive_series(dev(engine0, res['data']), marshal.mask_of_columns(res['columns']), ids, err_m=m,
                                  seed=SEED_PUBLIC, day0=0, f_tdp=float(sc[5]['f_TDP']), reach_params=rp).cpu().numpy()
    want_lo, want_up, _ = expected_stats(x, Q_BAND)
    ov = res['predictive']['overall']
    assert np.array_equal(ov['lower'], want_lo) and np.array_equal(ov['upper'], want_up)
    assert np.array_equal(ov['data'], engine.interpolate_quantiles(want_lo, want_up, Q_BAND, E_PUBLIC))
    # wider than the parameter-only band
    po = res['predictive']['param_only']
    for i in range(len(NAMES)):
        assert (ov['data'][2, i] - ov['data'][0, i]).mean() > (po['data'][2, i] - po['data'][0, i]).mean()


def bands_equal(a, b):
    for which in ('param_only', 'overall'):
        for k in ('data', 'lower', 'upper'):
            assert np.array_equal(bits(a[which][k]), bits(b[which][k])), (which, k)


def test_public_keep_daily_false_streams_nothing(base_run):
    res = public_call(keep_daily=False)
    assert res['data'] is None and res['stats']['streamed_chunks'] == 0
    bands_equal(res['predictive'], base_run['predictive'])


def test_public_without_error_model_has_no_overall_band(engine0):
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
    res = sp.run_simply_p_ensemble(met.iloc[:60], p_struc, p_SU, p_LU, p_SC, p, dyn, overrides=overrides_for(NAME, 65),
                                   quantiles=[0.5], predictive_series=['Qr', 'SRP_mgl'])
    pred = res['predictive']
    assert pred['overall'] is None and pred['info']['overall'] is None and pred['param_only']['data'].shape == (1, 2, 60, 1)
    want_lo, want_up, _ = expected_stats(res['data'][res['columns'].index('Qr')], [0.5])
    assert np.array_equal(pred['param_only']['lower'][:, 0], want_lo) and np.array_equal(pred['param_only']['upper'][:, 0], want_up)


def test_public_two_windows_laid_end_to_end_are_the_single_call(base_run):
    items = public_call(windows=183, keep_daily=False)
    assert [w['window'][2:] for w in items] == [(0, 183), (183, 366)]
    assert [w['predictive']['day0'] for w in items] == [0, 183]
    one = base_run['predictive']
    for which in ('param_only', 'overall'):
        for k in ('data', 'lower', 'upper'):
            laid = np.concatenate([w['predictive'][which][k] for w in items], axis=2)
            assert np.array_equal(bits(laid), bits(one[which][k])), (which, k)


def test_public_call_refuses_reduce_and_devices(engine0):
    with pytest.raises(ValueError, match='reduce'):
        public_call(reduce='annual')
    with pytest.raises(ValueError, match='devices'):
        public_call(devices=[0, 0])
