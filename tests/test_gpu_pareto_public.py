"""Pareto ranks through the public calls: ``run_simply_p_ensemble(pareto=[...])`` and ``sp.pareto_ranks`` on a Tarland ensemble of
300 members over the shortest stretch of 2004 in which discharge has more than 10 observations, against ``pareto.ranks`` applied
to the rows of the goodness-of-fit table the same call returns.  Equality of integers throughout."""

import numpy as np
import pytest

import helpers
import simplyp_amd as sp
from simplyp_amd import abi, marshal, pareto

pytestmark = pytest.mark.gpu

NAME = 'tarland_2004_dynamic'
E = 300
OUTS = ('rank', 'dominated_by', 'dominates')


def stretch():
    """(days, obs_dict, objectives): the first days of the record that hold 11 discharge observations; a chemistry variable is
    added when it has at least 3 observations there (NSE needs a variance of the observations)."""
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
    obs_dict = helpers.observations(p_SU['st_dt'], p_SU['end_dt'])
    q = obs_dict[1]['Q'].reindex(met.index)
    n_days = int(np.flatnonzero(q.notna().cumsum().to_numpy() > 10)[0]) + 1
    objectives = [('NSE', 'Q'), ('log NSE', 'Q'), ('Bias (%)', 'Q')]
    for var in abi.GOF_VARS[1:]:
        if var in obs_dict[1].columns and int(obs_dict[1][var].reindex(met.index[:n_days]).notna().sum()) >= 3:
            objectives.append(('NSE', var))
            break
    return n_days, obs_dict, objectives


def overrides(nan_member=None):
    base = helpers.marshal_scenario(NAME, E=1)['member_params'][:, 0]
    rng = np.random.default_rng(E)
    over = {nm: base[marshal.PM_NAMES.index(nm)] * rng.uniform(lo, hi, E)
            for nm, lo, hi in (('a_Q', 0.6, 1.6), ('T_g', 0.7, 1.4), ('E_M', 0.5, 2.0), ('fc', 0.85, 1.15))}
    if nan_member is not None:
        over['T_g'][nan_member] = np.nan                             # marshal.validate_ensemble does not look at T_g
    return over


def ensemble(nan_member=None, **kw):
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
    n_days, obs_dict, objectives = stretch()
    args = dict(overrides=overrides(nan_member), outputs=['Qr', 'Msus_kg/day', 'TDP_kg/day', 'PP_kg/day'], obs_dict=obs_dict, pareto=objectives)
    args.update(kw)
    return sp.run_simply_p_ensemble(met.iloc[:n_days], p_struc, p_SU, p_LU, p_SC, p, dyn, **args)


def rows_of(res, objectives):
    """The objectives' rows of the returned table, by hand."""
    data = np.asarray(res['gof']['data'])
    rows, sense = [], []
    for stat, var in objectives:
        row = data[abi.GOF_STATS.index(stat), abi.GOF_VARS.index(var), 0]
        rows.append(np.abs(row) if stat == 'Bias (%)' else row)
        sense.append(1 if stat in ('NSE', 'log NSE') else -1)
    return np.stack(rows), sense


def same(got, want, include_ints=True):
    for k in OUTS:
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got['front'], np.flatnonzero(want['rank'] == 0))
    if include_ints:
        assert got['n_members'] == want['n_used'] and got['n_fronts'] == want['n_fronts']
        assert got['info']['n_front0'] == want['n_front0'] and got['info']['pair_tests'] == want['pair_tests']


@pytest.fixture(scope='module')
def plain(engine0):
    return ensemble()


def test_ensemble_call_equals_the_rule_on_its_own_table(plain):
    n_days, _, objectives = stretch()
    assert n_days >= 11 and int(np.asarray(plain['gof']['data'])[0, 0, 0, 0]) == 11
    obj, sense = rows_of(plain, objectives)
    want = pareto.ranks(obj, sense)
    pa = plain['pareto']
    same(pa, want)
    assert pa['sense'] == sense and pa['objectives'][:3] == ['NSE(Q)', 'log NSE(Q)', '|Bias (%)|(Q)']
    assert pa['rank'].dtype == np.int32 and pa['n_members'] == E and 0 < len(pa['front']) < E and pa['n_fronts'] > 1
    assert (plain['status'] & abi.STATUS_NONFINITE == 0).all()


def test_pareto_ranks_of_a_returned_table(plain):
    _, _, objectives = stretch()
    again = sp.pareto_ranks(plain['gof'], objectives)
    for k in OUTS + ('front',):
        assert np.array_equal(again[k], plain['pareto'][k]), k
    assert again['n_fronts'] == plain['pareto']['n_fronts'] and again['objectives'] == plain['pareto']['objectives']
    # a device table, a mask, a bound on the fronts, an explicit sense
    dev = ensemble(to_host=False)
    assert not isinstance(dev['gof']['data'], np.ndarray)
    for k in OUTS:
        assert np.array_equal(dev['pareto'][k], plain['pareto'][k]), k
    members = np.arange(E) % 3 != 0
    obj, sense = rows_of(plain, objectives)
    got = sp.pareto_ranks(dev['gof'], objectives, members=members, max_fronts=2)
    same(got, pareto.ranks(obj, sense, include=members, max_fronts=2))
    assert (got['rank'] == abi.PARETO_UNRANKED).any() and (got['rank'][~members] == abi.PARETO_EXCLUDED).all()
    raw = sp.pareto_ranks(plain['gof'], [('Bias (%)', 'Q', 0, -1), ('N obs', 'Q', 0, 1)])      # the signed bias, minimised
    data = np.asarray(plain['gof']['data'])
    same(raw, pareto.ranks(np.stack([data[4, 0, 0], data[0, 0, 0]]), [-1, 1]))
    with pytest.raises(ValueError):
        sp.pareto_ranks(plain['gof'], [('N obs', 'Q')])
    with pytest.raises(ValueError):
        sp.pareto_ranks(plain['gof'], [('spearman', 'Q')])
    with pytest.raises(ValueError):
        sp.pareto_ranks(plain['gof'], objectives, members=np.ones(E + 1, dtype=bool))


def test_without_the_daily_table(plain):
    res = ensemble(keep_daily=False)
    for k in OUTS:
        assert np.array_equal(res['pareto'][k], plain['pareto'][k]), k


def test_nonfinite_member_and_quantile_members(plain):
    _, _, objectives = stretch()
    res = ensemble(nan_member=7)
    assert res['status'][7] & abi.STATUS_NONFINITE
    ok = (res['status'] & abi.STATUS_NONFINITE) == 0
    obj, sense = rows_of(res, objectives)
    same(res['pareto'], pareto.ranks(obj, sense, include=ok))
    assert all(res['pareto'][k][7] == abi.PARETO_EXCLUDED for k in OUTS) and res['pareto']['n_members'] == int(ok.sum()) == E - 1
    members = np.arange(E) < 120
    part = ensemble(quantile_members=members, pareto_max_fronts=3)
    obj, sense = rows_of(plain, objectives)
    want = pareto.ranks(obj, sense, include=members, max_fronts=3)
    same(part['pareto'], want)
    assert part['pareto']['n_members'] == 120 and (part['pareto']['rank'][120:] == abi.PARETO_EXCLUDED).all()
    assert part['pareto']['n_fronts'] <= 3 and 'quantiles' not in part


def test_spearman_objective():
    res = ensemble(spearman=True, pareto=[('spearman', 'Q'), ('nRMSD (%)', 'Q')])
    obj = np.stack([np.asarray(res['gof']['spearman'])[0, 0], np.asarray(res['gof']['data'])[abi.GOF_STATS.index('nRMSD (%)'), 0, 0]])
    same(res['pareto'], pareto.ranks(obj, [1, -1]))


def test_errors():
    with pytest.raises(ValueError, match='obs_dict'):
        ensemble(obs_dict=None)
    with pytest.raises(ValueError, match='devices'):
        ensemble(devices=[0])
    with pytest.raises(ValueError):
        ensemble(pareto=[('N obs', 'Q')])
    with pytest.raises(ValueError):
        ensemble(pareto=[('spearman', 'Q')])                         # the table holds none without spearman=True
    with pytest.raises(ValueError):
        ensemble(pareto_max_fronts=-1)
    with pytest.raises(ValueError):
        ensemble(pareto=[('NSE', 'Q', 1)])                           # one output reach


def test_band_of_the_front(plain):
    front = plain['pareto']['front']
    mask = np.zeros(E, dtype=bool)
    mask[front] = True
    assert np.array_equal(mask, plain['pareto']['rank'] == 0)
    res = ensemble(pareto=None, quantiles=[0.025, 0.5, 0.975], quantile_members=plain['pareto']['rank'] == 0)
    assert res['quantiles']['n_members'] == len(front) and 'pareto' not in res
