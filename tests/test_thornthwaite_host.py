"""Thornthwaite PET on the host (no GPU): ``simplyp_amd.thornthwaite_PET`` and the rule's one statement,
``forcing.thornthwaite_rows``, against what the unmodified reference ``daily_PET`` computed (tests/golden/thornthwaite_pet.npz,
made by tests/golden/make_pet_golden.py; the reference's own function ran, under two pandas shims that touch no arithmetic):
Tarland's air temperature 2003-2006 as it is, + 3 degC and - 20 degC (every year has I = 0 there: NaN), and 1981-2010.

The tolerance is derived, from the golden values and never from the code under test: tests/thornthwaite_bounds.py states the
derivation, with dT = 38 u max|T_air| for the monthly means (pandas' sum against the left-to-right one) and libm's pow error.
Measured (the largest absolute error of the four cases, and the bound at that month / day): monthly 8.5e-14 mm/month against
6.1e-12, daily 2.7e-15 mm/day against 1.7e-13.  The bounds stand about 65 times above what is seen: they are worst-case sums of
roundings that mostly cancel, and dT allows for 31 same-signed summation errors."""

import os
import shutil

import numpy as np
import pandas as pd
import pytest

import helpers
import simplyp_amd as sp
import thornthwaite_bounds as bounds
from simplyp_amd import forcing

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'thornthwaite_pet.npz')
SHORT = ('base', 'plus3', 'minus20')


@pytest.fixture(scope='module')
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def case_index(golden, case):
    return pd.date_range(str(golden[case + '/first_day']), periods=len(golden[case + '/T_air']))


def tolerances(golden, case, plan):
    """(absolute bound of PET_m [M], of the daily PET [D]) from the golden values alone."""
    dT = bounds.DT_SUM * np.abs(golden[case + '/T_air']).max()
    tol_m, _ = bounds.monthly(golden[case + '/T_m'], golden[case + '/PET_m'], dT, bounds.e_pow_libm)
    return tol_m, bounds.daily(tol_m, golden[case + '/PET_m'], plan)


def check(golden, case, plan, th, pet_m):
    """The case's monthly and daily values against the golden ones; returns the worst error / bound ratios."""
    want_m, want_d = golden[case + '/PET_m'], golden[case + '/PET']
    tol_m, tol_d = tolerances(golden, case, plan)
    assert np.array_equal(np.isnan(pet_m), np.isnan(want_m)) and np.array_equal(np.isnan(th), np.isnan(want_d))
    ok_m, ok_d = ~np.isnan(want_m), ~np.isnan(want_d)
    err_m, err_d = np.abs(pet_m - want_m)[ok_m], np.abs(th - want_d)[ok_d]
    print('%s: PET_m max abs err %.3e (bound there %.3e), daily %.3e (bound there %.3e)'
          % (case, err_m.max(initial=0.0), tol_m[ok_m][err_m.argmax()] if err_m.size else 0.0,
             err_d.max(initial=0.0), tol_d[ok_d][err_d.argmax()] if err_d.size else 0.0))
    assert (err_m <= tol_m[ok_m]).all(), (case, 'monthly', err_m.max())
    assert (err_d <= tol_d[ok_d]).all(), (case, 'daily', err_d.max())
    return ok_d


def test_golden_has_the_cases_the_rule_turns_on(golden):
    """2004 is the record's first leap year; at - 20 degC every year is dead (NaN throughout); the long series has months at 0."""
    assert len(golden['base/PET']) == 1461 and len(golden['full/PET']) == 10957
    assert np.isnan(golden['minus20/PET']).all() and (golden['minus20/T_m'] <= 0).all()
    for case in ('base', 'plus3', 'full'):
        assert np.isfinite(golden[case + '/PET']).all()
    assert (golden['full/PET_m'] == 0.0).any() and (golden['full/T_m'] < 0).any()


@pytest.mark.parametrize('case', SHORT + ('full',))
def test_thornthwaite_pet_matches_the_reference(golden, case):
    index = case_index(golden, case)
    met = pd.DataFrame({'T_air': golden[case + '/T_air'], 'PET': 7.0}, index=index)
    out = sp.thornthwaite_PET(57.1, met)
    assert list(out.columns) == ['T_air', 'PET'] and out.index.equals(index) and (met['PET'] == 7.0).all()
    plan = forcing.thornthwaite_plan(index, 57.1, max_years=None)
    _, _, pet_m = forcing.thornthwaite_rows(golden[case + '/T_air'][None], plan, monthly=True)
    check(golden, case, plan, out['PET'].to_numpy(), pet_m[0])


def test_the_leap_year_daylight_table_sticks(golden):
    """2003 reads the normal-year table, 2004 and every year after it the leap-year one -- 2005 and 2006 too, as in the reference
    (its loop never assigns the normal table back).  With the calendar-true table 2005 would differ from the golden by far more
    than the bound."""
    plan = forcing.thornthwaite_plan(case_index(golden, 'base'), 57.1)
    normal, leap = np.array(forcing.daylight_hours(57.1, False)), np.array(forcing.daylight_hours(57.1, True))
    L = plan['daylight'].reshape(4, 12)
    assert np.array_equal(L[0], normal) and all(np.array_equal(L[y], leap) for y in (1, 2, 3)) and not np.array_equal(normal[2:], leap[2:])
    fixed = dict(plan, daylight=np.concatenate([normal, leap, normal, normal]))
    th = forcing.thornthwaite_rows(golden['base/T_air'][None], fixed)[0]
    _, tol_d = tolerances(golden, 'base', plan)
    year3 = slice(365 + 366 + 31, 365 + 366 + 334)
    assert (np.abs(th - golden['base/PET'])[year3] > 1e6 * tol_d[year3]).all()


def test_rows_stacked_match_the_reference(golden):
    """The three 2003-2006 series as three members of one call, and the long series: row e is case e."""
    plan = forcing.thornthwaite_plan(case_index(golden, 'base'), 57.1)
    th, t_m, pet_m = forcing.thornthwaite_rows(np.stack([golden[c + '/T_air'] for c in SHORT]), plan, monthly=True)
    assert th.shape == (3, 1461) and t_m.shape == pet_m.shape == (3, 48)
    for e, case in enumerate(SHORT):
        check(golden, case, plan, th[e], pet_m[e])
        want = golden[case + '/T_m'] * (golden[case + '/T_m'] >= 0)
        assert np.abs(t_m[e] - want).max() <= bounds.DT_SUM * np.abs(golden[case + '/T_air']).max()
    assert np.isnan(th[2]).all() and np.isfinite(th[:2]).all()
    plan = forcing.thornthwaite_plan(case_index(golden, 'full'), 57.1)
    th, _, pet_m = forcing.thornthwaite_rows(golden['full/T_air'][None], plan, monthly=True)
    check(golden, 'full', plan, th[0], pet_m[0])


def test_plan_nodes_sit_on_the_16th(golden):
    index = case_index(golden, 'base')
    plan = forcing.thornthwaite_plan(index, 57.1)
    dom, m_of_day = np.asarray(index.day), (np.asarray(index.year) - 2003) * 12 + np.asarray(index.month) - 1
    assert (plan['k'][dom == 16] == 0).all() and (plan['node'][dom == 16] == m_of_day[dom == 16]).all()
    assert (plan['k'][:15] == 0).all() and (plan['node'][:15] == 0).all()             # the first node's value
    assert (plan['k'][-15:] == 0).all() and (plan['node'][-15:] == 47).all()          # the last node's value
    mid = slice(15, 1461 - 16)
    assert (plan['k'][mid] < plan['n'][mid]).all() and set(plan['n'][mid]) == {28, 29, 30, 31}
    assert np.array_equal(plan['days'], [pd.Timestamp(2003 + m // 12, m % 12 + 1, 1).daysinmonth for m in range(48)])


@pytest.mark.parametrize('days,latitude,match', [
    (slice(0, 1460), 57.1, 'whole calendar years'), (slice(1, 1461), 57.1, 'whole calendar years'),
    (slice(0, 1461), 91.0, r'latitude must lie in \[-90, 90\]'), (slice(0, 1461), float('nan'), 'latitude')])
def test_refusals(golden, days, latitude, match):
    index = case_index(golden, 'base')[days]
    with pytest.raises(ValueError, match=match):
        sp.thornthwaite_PET(latitude, pd.DataFrame({'T_air': golden['base/T_air'][days]}, index=index))
    with pytest.raises(ValueError, match=match):
        forcing.resolve({'PET': {'model': 'thornthwaite', 'latitude': latitude}}, index, 4, True)


def test_resolve_words_its_refusals(golden):
    index = case_index(golden, 'base')
    with pytest.raises(ValueError, match='snow module'):
        forcing.resolve({'PET': {'model': 'thornthwaite', 'latitude': 57.1}}, index, 4, False)
    with pytest.raises(ValueError, match="must be one of"):
        forcing.resolve({'PET': {'model': 'penman', 'latitude': 57.1}}, index, 4, True)
    with pytest.raises(ValueError, match="needs .*latitude"):
        forcing.resolve({'PET': {'model': 'thornthwaite'}}, index, 4, True)
    with pytest.raises(ValueError, match="at most 64 years"):
        forcing.resolve({'PET': {'model': 'thornthwaite', 'latitude': 57.1}}, pd.date_range('1901-01-01', '1965-12-31'), 4, True)
    fe = forcing.resolve({'PET': {'model': 'thornthwaite', 'latitude': 57.1}}, index, 4, True)
    assert fe['pet']['model'] == 1 and fe['pet']['years'] == 4 and fe['pet']['months'] == 48
    with pytest.raises(ValueError, match='windows'):
        forcing.day_window(fe, 0, 366)
    for where in ('run_simply_p_ensemble_windows', 'assimilate'):
        with pytest.raises(ValueError, match='%s: the daily interpolation .* crosses year boundaries' % where):
            forcing.refuse_pet_model({'PET': {'model': 'thornthwaite', 'latitude': 57.1}}, where)
    assert forcing.resolve({'PET': {'sigma': 0.1}}, index, 4, True)['pet'] is None


def test_the_table_mirror_composes_th_and_f(golden):
    """forcing.table with the model: PET = TH(final T_air) * F, F = the PET row of the same spec on a base PET of ones."""
    index = case_index(golden, 'base')
    E, D = 4, len(index)
    base = np.stack([np.full(D, 2.0), np.full(D, 123.0), golden['base/T_air']])[None]
    spec = {'PET': {'sigma': 0.1, 'groups': 'month', 'scale': [1.1, 0.9, 1.0, 1.0]}, 'T_air': {'offset': [0.0, 3.0, 0.0, 0.0], 'sigma': 0.5}}
    fe = forcing.resolve(dict(spec, PET=dict(spec['PET'], model='thornthwaite', latitude=57.1)), index, E, True, 11)
    got = forcing.table(base, fe, E=E)
    ones = base.copy()
    ones[:, 1] = 1.0
    f = forcing.table(ones, forcing.resolve(spec, index, E, True, 11), E=E)
    assert np.array_equal(got[:, 2], f[:, 2]) and np.array_equal(got[:, 0], f[:, 0])
    assert np.array_equal(got[:, 1], forcing.thornthwaite_rows(got[:, 2], fe['pet']) * f[:, 1])
    plain = forcing.table(base, forcing.resolve({'PET': {'model': 'thornthwaite', 'latitude': 57.1}}, index, E, True, 11), E=E)
    assert np.array_equal(plain[0, 1], forcing.thornthwaite_rows(base[0, 2:3], fe['pet'])[0])


def test_read_input_data_derives_pet_when_the_met_file_has_none(tmp_path, capsys):
    """The Tarland met file without its PET column, 2003-2006: read_input_data used to end in NotImplementedError."""
    rel = tmp_path / 'Current_Release' / 'v0-2A'
    rel.mkdir(parents=True)
    workbook = str(rel / 'Parameters_v0-2A_Tarland.xlsx')
    shutil.copy(os.path.join(helpers.DATA, 'Parameters_v0-2A_Tarland.xlsx'), workbook)
    met = pd.read_csv(os.path.join(helpers.DATA, 'Tarland_MetData_1981-2010.csv'), index_col=0)
    assert 'PET' in met.columns
    met_path = str(tmp_path / 'met_without_pet.csv')
    met.drop(columns=['PET']).to_csv(met_path)
    over = {'metdata_fpath': met_path, 'st_dt': '2003-01-01', 'end_dt': '2006-12-31', 'Qobsdata_fpath': None, 'chemObsData_fpath': None}
    p_SU, _, p, _, _, _, met_df, _ = sp.read_input_data(workbook, setup_overrides=over)
    assert 'PET estimated using the Thornthwaite method' in capsys.readouterr().out
    assert len(met_df) == 1461 and 'PET' in met_df.columns and np.isfinite(met_df['PET']).all()
    want = sp.thornthwaite_PET(p['latitude'], met_df.drop(columns=['PET']))
    assert np.array_equal(met_df['PET'].to_numpy(), want['PET'].to_numpy())
    with pytest.raises(ValueError, match='whole calendar years'):
        sp.read_input_data(workbook, setup_overrides=dict(over, end_dt='2006-06-30'))
    with pytest.raises(NotImplementedError):
        sp.daily_PET(57.1, met_df)
