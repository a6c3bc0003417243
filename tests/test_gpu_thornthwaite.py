"""Thornthwaite PET from each member's own air temperature, on the device (simplyp_forcing_pet_kernel): the kept forcing table
against the NumPy statement (forcing.thornthwaite_rows) and against the reference's golden values, the composition with the PET
scale and error, the run that reads the table, member blocks, and the refusals.

Tarland 2003-2006 (D = 1461: no multiple of 64 or 256, months straddle every tile edge of the day loops, 48 months in one tile of
64), its one reach, the snow module in the kernel, E = 8 members that differ in what the forcing-error layer gives them:

    member  0      1      2       3  4  5   6     7
    T_air   base   + 3    - 20    base      base  base        (offset, degC; member 2: every year has I = 0, NaN)
    PET     x 1    x 1    x 1     x 1       x 1.1 x 0.9       (scale)

``sigma`` and ``rho`` belong to a forcing row, not to a member, so the errors of the members' list -- T_air sigma = 2 on daily
groups, the same with rho = 0.8, PET sigma = 0.1 on monthly groups -- are calls of their own of these eight members, and one
with errors on both rows (CONFIGS): each test
runs over every configuration it applies to, so every member meets every kernel path (independent and AR(1) generator, F read
or not).

Device against statement, given the same T_air rows: sums, quotients and products are IEEE operations in one order on both
sides, so the monthly means are equal and only x ** y differs, sp_exp(y sp_log(x)) against libm's within 2 (1 + 3 |y ln x|) 2^-52
(tests/test_gpu_elementary.py pins sp_exp and sp_log below 1 ulp; tests/thornthwaite_bounds.py carries that through I, a, PET_m
and the interpolation, month by month with the month's own |y ln x|: up to 2.1 without a T_air error, 1.514 |ln(T_m / 5)| of a
month whose mean a draw leaves near 0 with one: 5.4 here; each test prints the largest it met).  F of the statement is the
mirror's own draw: within 2^-43 relative of the device's (tests/test_gpu_forcing.py derives that).  Measured values on MI355X
stand in each test's docstring."""

import numpy as np
import pandas as pd
import pytest

import helpers
import simplyp_amd as sp
import thornthwaite_bounds as bounds
from simplyp_amd import abi, engine, forcing, marshal, synthetic

pytestmark = pytest.mark.gpu

E, D, SEED, LATITUDE = 8, 1461, 20031, 57.1
OFFSET = np.array([0.0, 3.0, -20.0, 0.0, 0.0, 0.0, 0.0, 0.0])
SCALE = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.1, 0.9])
F_TOL = 2.0 ** -43
CONFIGS = {'plain': ({}, {}),
           'tair_iid': ({}, {'sigma': 2.0, 'groups': 'day'}),
           'tair_ar1': ({}, {'sigma': 2.0, 'groups': 'day', 'rho': 0.8}),
           'pet_noise': ({'sigma': 0.1, 'groups': 'month'}, {}),
           'both_ar1': ({'sigma': 0.1, 'groups': 'month', 'rho': 0.5}, {'sigma': 2.0, 'groups': 'day'})}
MASK = marshal.mask_of_columns(marshal.FLUX_COLUMNS)
QR = marshal.columns_of_mask(MASK).index('Qr')


def inputs():
    return synthetic.tarland_inputs('2003-01-01', '2006-12-31')


@pytest.fixture(scope='module')
def problem():
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = inputs()
    marshal.prologue(p_SU, p_LU, p_SC, p)
    up_ptr, up_idx, _ = marshal.topology(p_struc, p)
    f, doy = marshal.forcing_arrays(met, snow=True)
    opts = abi.make_opts(None, dynamic_epc0=dyn['Dynamic_EPC0'] == 'y', dynamic_erod=dyn['Dynamic_erodibility'] == 'y',
                         run_mode_cal=p_SU.run_mode == 'cal', sc_qr0=marshal.sc_list(p).index(int(p['SC_Qr0'])), out_mask=MASK, snow=True)
    assert f.shape == (1, 3, D)
    return dict(forcing=f, doy=doy, member_params=marshal.member_params(p, p_LU, E), reach_params=marshal.reach_params(p_SC, p, E),
                up_ptr=up_ptr, up_idx=up_idx, opts=opts, met=met)


def spec(config, model=True, lo=0, hi=E):
    pet, t_air = (dict(d) for d in CONFIGS[config])
    pet['scale'], t_air['offset'] = SCALE[lo:hi], OFFSET[lo:hi]
    if model:
        pet['model'], pet['latitude'] = 'thornthwaite', LATITUDE
    return {'PET': pet, 'T_air': t_air}


def run(eng, m, lo=0, hi=E, **kw):
    out, status, stats = eng.run(m['forcing'], m['doy'], np.ascontiguousarray(m['member_params'][:, lo:hi]),
                                 np.ascontiguousarray(m['reach_params'][:, :, lo:hi]), m['up_ptr'], m['up_idx'], m['opts'], **kw)
    return out.cpu().numpy(), status.cpu().numpy(), stats


def same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def same_but_nan(a, b):
    """NaN where the other is NaN (whatever its payload) and the same bits everywhere else."""
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and same(np.where(nan, 0.0, a), np.where(nan, 0.0, b))


@pytest.fixture(scope='module')
def calls(engine0, problem):
    """{config: (out, status, kept table)} of the whole call of each configuration, made once."""
    made = {}

    def get(config):
        if config not in made:
            fe = forcing.resolve(spec(config), problem['met'].index, E, True, SEED)
            out, status, stats = run(engine0, problem, forcing_error=fe, keep_forcing_table=True)
            made[config] = (out, status, stats['forcing_table'].cpu().numpy())
        return made[config]
    return get


@pytest.fixture(scope='module')
def golden():
    with np.load(helpers.GOLDEN + '/thornthwaite_pet.npz') as z:
        return {k: z[k] for k in z.files}


def device_bound(t_air, plan):
    """(absolute bound [E, D] of TH on the device against the statement on the rows ``t_air``, the statement's TH, the largest
    |y ln x|): from the statement's own monthly values."""
    th, t_m, pet_m = forcing.thornthwaite_rows(t_air, plan, monthly=True)
    tol, t_max = np.empty_like(th), 0.0
    for e in range(len(th)):
        tol_m, t = bounds.monthly(t_m[e], pet_m[e], 0.0, bounds.e_pow_device)
        tol[e], t_max = bounds.daily(tol_m, pet_m[e], plan), max(t_max, t)
    return tol, th, t_max


# ---- 1. the kept table against the statement -------------------------------------------------------------------------------

@pytest.mark.parametrize('config', list(CONFIGS))
def test_table_matches_the_statement(calls, problem, config):
    """PET = TH(the table's own T_air rows) x F within the derived bound; P and T_air are what the generator writes without the
    model, bit for bit; member 2 is NaN on both sides in every year (I = 0 throughout at - 20 degC) and nowhere else is anything.
    Measured on MI355X: worst error / bound over the five configurations 0.075 ('tair_ar1', whose draws leave a monthly mean
    near 0: |y ln x| = 5.4); largest absolute error 1.8e-15 mm/day, largest relative error 8.7e-16."""
    _, status, got = calls(config)
    index = problem['met'].index
    fe = forcing.resolve(spec(config), index, E, True, SEED)
    off = forcing.table(problem['forcing'], forcing.resolve(spec(config, model=False), index, E, True, SEED), E=E)
    ones = problem['forcing'].copy()
    ones[:, 1] = 1.0
    f = forcing.table(ones, forcing.resolve(spec(config, model=False), index, E, True, SEED), E=E)[:, 1]
    assert got.shape == (E, 3, D)
    assert same(got[:, 0], np.ascontiguousarray(off[:, 0]))      # P: no entry, the base row
    if not CONFIGS[config][1]:                                   # no T_air error: base + offset exactly
        assert same(got[:, 2], np.ascontiguousarray(off[:, 2]))
    tol, th, t_max = device_bound(got[:, 2], fe['pet'])
    want = th * f
    has_f = bool(CONFIGS[config][0])
    tol = tol * np.abs(f) + (F_TOL if has_f else 2.0 * bounds.U) * np.abs(want)      # (no draw: the product's rounding on either side)
    nan = np.isnan(want)
    assert np.array_equal(nan, np.isnan(got[:, 1])) and nan[2].all() and not np.delete(nan, 2, axis=0).any()
    err = np.abs(got[:, 1] - want)[~nan]
    print('%s: max |y ln x| %.2f; PET max abs err %.3e, worst err / bound %.3f, max rel err %.3e'
          % (config, t_max, err.max(), (err / tol[~nan]).max(), helpers.max_rel_err(got[:, 1][~nan], want[~nan], floor=1e-300)))
    assert (err <= tol[~nan]).all()
    assert (status[2] & abi.STATUS_NONFINITE) and not np.delete(status, 2).any()


# ---- 2. members 0-2 against the reference ----------------------------------------------------------------------------------

def test_members_without_error_match_the_reference(calls, problem, golden):
    """No sigma: T_air is base + offset, PET x 1, so rows 0-2 are the reference's daily_PET of Tarland's series, + 3 and - 20 degC.
    Tolerance: the device's bound against the statement plus the statement's against the reference (tests/test_thornthwaite_host.py).
    Measured on MI355X: largest error 2.7e-15 mm/day (+ 3 degC) where the bound is 2.4e-13."""
    _, _, got = calls('plain')
    plan = forcing.thornthwaite_plan(problem['met'].index, LATITUDE)
    for e, case in enumerate(('base', 'plus3', 'minus20')):
        assert same(got[e, 2], golden[case + '/T_air'])
        want = golden[case + '/PET']
        dT = bounds.DT_SUM * np.abs(golden[case + '/T_air']).max()
        tol_m, _ = bounds.monthly(golden[case + '/T_m'], golden[case + '/PET_m'], dT, bounds.e_pow_libm)
        tol_dev, _ = bounds.monthly(golden[case + '/T_m'], golden[case + '/PET_m'], 0.0, bounds.e_pow_device)
        tol = bounds.daily(tol_m, golden[case + '/PET_m'], plan) + bounds.daily(tol_dev, golden[case + '/PET_m'], plan)
        assert np.array_equal(np.isnan(got[e, 1]), np.isnan(want)) and np.isnan(want).all() == (e == 2)
        ok = ~np.isnan(want)
        err = np.abs(got[e, 1] - want)[ok]
        print('%s: max abs err %.3e (bound there %.3e)' % (case, err.max(initial=0.0), tol[ok][err.argmax()] if err.size else 0.0))
        assert (err <= tol[ok]).all()


# ---- 3. TH x F -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('config', ['plain', 'pet_noise', 'both_ar1'])
def test_pet_is_th_times_f_bit_for_bit(engine0, calls, problem, config):
    """F: the PET row of a second call without the model on a base PET of all ones (so members 6 and 7 carry their scale, and
    with 'pet_noise' / 'both_ar1' their draw).  TH: the PET row of a third call with the model and neither scale nor PET error,
    its T_air rows being the same bits.  PET = TH x F in IEEE arithmetic, for every member."""
    _, _, got = calls(config)
    index = problem['met'].index
    ones = dict(problem, forcing=problem['forcing'].copy())
    ones['forcing'][:, 1] = 1.0
    _, _, st = run(engine0, ones, forcing_error=forcing.resolve(spec(config, model=False), index, E, True, SEED), keep_forcing_table=True)
    f = st['forcing_table'].cpu().numpy()
    bare = spec(config)
    bare['PET'] = {'model': 'thornthwaite', 'latitude': LATITUDE}
    _, _, st = run(engine0, problem, forcing_error=forcing.resolve(bare, index, E, True, SEED), keep_forcing_table=True)
    th = st['forcing_table'].cpu().numpy()
    assert same(f[:, 2], got[:, 2]) and same(th[:, 2], got[:, 2]) and same(f[:, 0], got[:, 0])
    assert same_but_nan(got[:, 1], th[:, 1] * f[:, 1]) and np.isnan(got[2, 1]).all() and not np.isnan(np.delete(got[:, 1], 2, axis=0)).any()
    assert (f[:6, 1] == 1.0).all() if config == 'plain' else len(np.unique(f[:, 1])) > 8 * 40
    assert same_but_nan(got[:6, 1], th[:6, 1]) if config == 'plain' else True
    assert not same(got[6, 1], th[6, 1]) and not same(got[7, 1], th[7, 1])


# ---- 4. the run consumes the table -----------------------------------------------------------------------------------------

@pytest.mark.parametrize('config', ['plain', 'both_ar1'])
def test_run_reads_exactly_the_kept_table(engine0, calls, problem, config):
    out, status, table = calls(config)
    out2, status2, _ = run(engine0, dict(problem, forcing=table), forcing_of_member=np.arange(E, dtype=np.int32))
    assert same(out, out2) and same(status, status2)
    plain, _, _ = run(engine0, problem)
    assert not same(out[..., 0], plain[..., 0])                  # (member 0: the derived PET, not the met file's column)


# ---- 5. the loop closes ----------------------------------------------------------------------------------------------------

def test_a_warmer_member_evaporates_more_and_runs_off_less(calls, problem):
    """Member 1 (+ 3 degC) against member 0, per calendar year: more PET, less discharge.  (Before the PET model a T_air offset
    reached the snow module alone and left PET as it was.)"""
    out, status, table = calls('plain')
    year = np.asarray(problem['met'].index.year)
    assert status[0] == 0 and status[1] == 0
    for y in range(2003, 2007):
        pet0, pet1 = (table[e, 1, year == y].sum() for e in (0, 1))
        q0, q1 = (out[QR, year == y, 0, e].sum() for e in (0, 1))
        print('%d: PET %.1f -> %.1f mm, Qr %.4g -> %.4g' % (y, pet0, pet1, q0, q1))
        assert pet1 > pet0 > 0.0 and 0.0 < q1 < q0


def test_the_public_call_takes_the_option(calls, problem):
    """run_simply_p_ensemble(forcing_error={'PET': {'model': 'thornthwaite', ...}}): the engine call's result, and the same bits
    as two device blocks."""
    out, status, _ = calls('both_ar1')
    fc = float(inputs()[5]['fc'])
    kw = dict(overrides={'fc': np.full(E, fc)}, forcing_error=spec('both_ar1'), forcing_seed=SEED, snow_in_kernel=True,
              outputs=marshal.FLUX_COLUMNS)
    res = sp.run_simply_p_ensemble(*inputs(), **kw)
    data = np.ascontiguousarray(res['data'])
    assert data.shape == out.shape and np.array_equal(np.asarray(res['status']), status)
    live = np.delete(np.arange(E), 2)                            # (two valid integrations of one problem: the working tolerance)
    assert np.isnan(data[..., 2]).any() and helpers.max_rel_err(data[..., live], out[..., live], floor=1e-12) <= helpers.TOL_WORKING
    two = sp.run_simply_p_ensemble(*inputs(), devices=[0, 0], **kw)
    assert two['stats']['bounds'] == [[0, 4], [4, 8]] and same_but_nan(np.ascontiguousarray(two['data']), data)
    assert np.array_equal(np.asarray(two['status']), np.asarray(res['status']))


# ---- 6. member blocks ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('config', list(CONFIGS))
def test_a_member_block_is_its_rows_of_the_whole_call(engine0, calls, problem, config):
    out, status, table = calls(config)
    fe = forcing.resolve(spec(config), problem['met'].index, E, True, SEED)
    blk = forcing.member_block(fe, 3, E)
    assert blk['member0'] == 3
    out_b, status_b, st = run(engine0, problem, 3, E, forcing_error=blk, keep_forcing_table=True)
    assert same(st['forcing_table'].cpu().numpy(), np.ascontiguousarray(table[3:]))
    assert same(out_b, np.ascontiguousarray(out[..., 3:])) and same(status_b, status[3:])


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------

def _plan_opts(eng, m, pet_only=False):
    s = {'PET': {'model': 'thornthwaite', 'latitude': LATITUDE, 'scale': SCALE}} if pet_only else spec('plain')
    fe = forcing.resolve(s, m['met'].index, E, True, SEED)
    o, keep = eng._forcing_opts(m['opts'], fe, E, D, 3)
    keep[0].fill_(-777.0)
    return o, keep


def _refused(eng, m, o, keep, match):
    out = eng.torch.full((len(marshal.FLUX_COLUMNS), D, 1, E), -777.0, dtype=eng.torch.float64, device=eng.tdev)
    f = m['forcing'] if o.snow else np.ascontiguousarray(m['forcing'][:, :2])
    with pytest.raises(engine.EngineError, match=match):
        eng.run(f, m['doy'], m['member_params'], m['reach_params'], m['up_ptr'], m['up_idx'], o, out=out)
    eng.torch.cuda.synchronize()
    assert bool((keep[0] == -777.0).all()) and bool((out == -777.0).all())


@pytest.mark.parametrize('edit,match', [
    (dict(forcing_pet_model=2), r'forcing_pet_model must be 0 \(off\) or 1'),
    (dict(forcing_pet_model=-1), r'forcing_pet_model must be 0 \(off\) or 1'),
    (dict(snow=0), 'forcing_pet_model = 1 derives PET from the member.s T_air row'),
    (dict(forcing_error=0), 'forcing_pet_model needs forcing_error = 1')])
def test_the_library_refuses_a_bad_model_and_launches_nothing(engine0, problem, edit, match):
    """Every refusal stands before the generator's launch: the table workspace and the output keep their fill.  (snow = 0: a
    call with the PET scale alone and two base rows, so that nothing but the model asks for the T_air row.  forcing_error = 0:
    the model is the one forcing field left set.)"""
    o, keep = _plan_opts(engine0, problem, pet_only='snow' in edit)
    if 'forcing_error' in edit:
        plain = problem['opts'].copy()
        plain.forcing_pet_model = o.forcing_pet_model
        o = plain
    else:
        for k, v in edit.items():
            setattr(o, k, v)
    _refused(engine0, problem, o, keep, match)


@pytest.mark.parametrize('days,match', [
    (364, 'needs whole calendar years of daily values: D = 364'),                    # less than a year
    (1464, 'needs whole calendar years of daily values: D = 1464'),                  # four years and four days: one leap day too many
    (65 * 365 + 16, r'takes at most 64 years')])                                    # the cap, whatever the plan says
def test_the_library_refuses_days_that_are_no_whole_years(engine0, problem, days, match):
    """Through the C ABI with a fabricated run of ``days`` days (the workspace is sized for it; nothing in it is read before the
    refusal): the library derives the years from D alone, Y = D / 365 with at most Y / 4 + 1 leap days, at most 64."""
    torch = engine0.torch
    f = np.zeros((1, 3, days))
    doy = np.ones(days, dtype=np.int32)
    work = torch.full((E * 3 * days + (abi.forcing_pet_plan_bytes(days) + 7) // 8,), -777.0, dtype=torch.float64, device=engine0.tdev)
    o = problem['opts'].copy()
    o.forcing_error, o.forcing_pet_model, o.forcing_table = 1, 1, work.data_ptr()
    out = torch.full((len(marshal.FLUX_COLUMNS), days, 1, E), -777.0, dtype=torch.float64, device=engine0.tdev)
    with pytest.raises(engine.EngineError, match=match):
        engine0.run(f, doy, problem['member_params'], problem['reach_params'], problem['up_ptr'], problem['up_idx'], o, out=out)
    torch.cuda.synchronize()
    assert bool((work == -777.0).all()) and bool((out == -777.0).all())


def test_the_public_calls_refuse_before_any_device_call(problem, monkeypatch):
    """Partial years, no snow module, a latitude off the globe, windows and the filter: ValueError, and the engine is never
    reached (Engine.run is replaced by a tripwire)."""
    def tripwire(*a, **k):
        raise AssertionError('a refused call reached the device')
    monkeypatch.setattr(engine.Engine, 'run', tripwire)
    args = inputs()
    fc = float(args[5]['fc'])
    kw = dict(overrides={'fc': np.full(E, fc)}, forcing_seed=SEED, snow_in_kernel=True)
    fe = {'PET': {'model': 'thornthwaite', 'latitude': LATITUDE}}
    short = (args[0].iloc[:1460],) + tuple(args[1:])
    with pytest.raises(ValueError, match='whole calendar years'):
        sp.run_simply_p_ensemble(*short, forcing_error=fe, **kw)
    with pytest.raises(ValueError, match='snow module'):
        sp.run_simply_p_ensemble(*inputs(), forcing_error=fe, **dict(kw, snow_in_kernel=False))
    with pytest.raises(ValueError, match=r'latitude must lie in \[-90, 90\]'):
        sp.run_simply_p_ensemble(*inputs(), forcing_error={'PET': {'model': 'thornthwaite', 'latitude': 91.0}}, **kw)
    index = args[0].index
    with pytest.raises(ValueError, match='run_simply_p_ensemble_windows: the daily interpolation .* crosses year boundaries'):
        sp.run_simply_p_ensemble_windows(*inputs(), window=[index[0], index[365]], forcing_error=fe, **kw)
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = inputs()
    priors = {nm: (0.7 * float(p[nm]), 1.3 * float(p[nm])) for nm in ('fc', 'T_g', 'a_Q')}
    priors['m_Q'] = (0.01, 1.0)
    with pytest.raises(ValueError, match='assimilate: the daily interpolation .* crosses year boundaries'):
        sp.assimilate(met, p_struc, p_SU, p_LU, p_SC, p, dyn, helpers.observations('2003-01-01', '2006-12-31'), priors=priors,
                      variables=['Q'], n_particles=E, window=365, seed=SEED, forcing_error=fe)
