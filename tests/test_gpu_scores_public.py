"""Scores through the public calls: ``run_simply_p_ensemble(score=True)``, ``run_simply_p_ensemble_windows`` and
``assimilate(score=True)`` on Tarland 2004 with 256 members, against ``simplyp_amd.score`` applied to what
``Engine.predictive_series`` materialises (counts ==, A and B within 1e-12 of their exact values relative to themselves: the bound
of tests/test_gpu_scores.py), and against each other bit for bit: without the daily table, window by window, continued through
``state=``, and a filter window recomputed by an ensemble call from the record."""

from fractions import Fraction

import numpy as np
import pytest

import helpers
import simplyp_amd as sp
from simplyp_amd import abi, marshal, particle, score, visualise_results as vr

pytestmark = pytest.mark.gpu

NAME = 'tarland_2004_dynamic'
FLUX = ['Qr', 'Msus_kg/day', 'TDP_kg/day', 'PP_kg/day']
E, SEED = 256, 29
REL = Fraction(1, 10 ** 12)
ARRAYS = ('crps', 'abs_err', 'spread', 'below', 'at_or_below', 'pit')


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype.itemsize == 8 else a


def overrides():
    base = helpers.marshal_scenario(NAME, E=1)['member_params'][:, 0]
    rng = np.random.default_rng(E)
    return {nm: base[marshal.PM_NAMES.index(nm)] * rng.uniform(lo, hi, E)
            for nm, lo, hi in (('a_Q', 0.6, 1.6), ('T_g', 0.7, 1.4), ('E_M', 0.5, 2.0), ('fc', 0.85, 1.15))}


def ensemble(days=slice(None), windows=None, **kw):
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
    obs_dict = kw.pop('obs_dict', helpers.observations(p_SU['st_dt'], p_SU['end_dt']))
    args = dict(overrides=overrides(), outputs=FLUX, obs_dict=obs_dict, score=True, predictive_seed=SEED)
    args.update(kw)
    if windows is not None:
        return list(sp.run_simply_p_ensemble_windows(met.iloc[days], p_struc, p_SU, p_LU, p_SC, p, dyn, window=windows, **args))
    return sp.run_simply_p_ensemble(met.iloc[days], p_struc, p_SU, p_LU, p_SC, p, dyn, **args)


def same_scores(a, b, days=slice(None)):
    for key in ('param_only', 'overall'):
        if a[key] is None or b[key] is None:
            assert a[key] is None and b[key] is None, key
            continue
        for k in ARRAYS:
            assert np.array_equal(bits(a[key][k][:, days]), bits(b[key][k])), (key, k)


def against_the_rule(engine0, res, weights=None, m=None):
    """``res['scores']`` against score.scores of the materialised series on the observed days."""
    sc = res['scores']
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
    rp = np.zeros((len(marshal.PR_NAMES), 1, E))
    rp[marshal.PR_NAMES.index('A_catch')] = float(p_SC.loc['A_catch', 1])
    ids = [abi.TQ_DERIVED + abi.TQ_DERIVED_SERIES.index(c) for c in sc['series']]
    obs = vr.observation_array(helpers.observations(p_SU['st_dt'], p_SU['end_dt']), [1], met.index)[0]     # [6, D]
    mask = marshal.mask_of_columns(res['columns'])
    n = 0
    for key, err_m in (('param_only', None), ('overall', m)):
        if key == 'overall' and m is None:
            assert sc['overall'] is None
            continue
        series = engine0.predictive_series(res['data'], mask, ids, err_m=err_m, seed=SEED, f_tdp=float(p['f_TDP']),
                                           reach_params=rp).cpu().numpy()
        part = sc[key]
        for si, name in enumerate(sc['series']):
            y = obs[abi.TQ_DERIVED_SERIES.index(name)]
            days = np.flatnonzero(~np.isnan(y))
            assert len(days) > 0 and part['n_obs'][si, 0] == len(days)
            want = score.scores(series[si, days, 0], y[days], weights)
            assert sc['weight_total'] == want['T']
            assert np.array_equal(part['below'][si, days, 0], want['below']) and np.array_equal(part['at_or_below'][si, days, 0], want['at_or_below'])
            for k, d in enumerate(days):
                A, B = want['exact'][k]
                assert abs(Fraction(float(part['abs_err'][si, d, 0])) - A) <= REL * A and abs(Fraction(float(part['spread'][si, d, 0])) - B) <= REL * B
                n += 1
            assert np.array_equal(bits(part['crps'][si]), bits(part['abs_err'][si] - part['spread'][si]))
            assert np.array_equal(part['pit'][si, days, 0], score.pit(want['below'], want['at_or_below'], want['T']))
            assert ((part['pit'][si, days, 0] >= 0) & (part['pit'][si, days, 0] <= 1)).all()
            rest = np.setdiff1d(np.arange(len(y)), days)                 # nothing observed: NaN and 0
            assert np.isnan(part['crps'][si, rest, 0]).all() and np.isnan(part['pit'][si, rest, 0]).all() and not part['below'][si, rest, 0].any()
            assert part['mean_crps'][si, 0] == pytest.approx(np.nanmean(part['crps'][si, :, 0]), rel=1e-13)
            assert (part['crps'][si, days, 0] >= -1e-12 * (part['abs_err'][si, days, 0] + part['spread'][si, days, 0])).all()
    return n


@pytest.fixture(scope='module')
def plain(engine0):
    return ensemble(to_host=False)


def test_scores_of_the_ensemble_call(engine0, plain):
    sc = plain['scores']
    assert sc['series'][0] == 'Q_cumecs' and len(sc['series']) >= 2 and sc['reaches'] == [1] and sc['n_members'] == E
    assert sc['param_only']['crps'].shape == (len(sc['series']), 366, 1) and sc['param_only']['mean_crps'].shape == (len(sc['series']), 1)
    assert sc['param_only']['below'].dtype == np.uint64 and sc['weight_total'] == E and sc['seed'] == SEED and sc['day0'] == 0
    assert against_the_rule(engine0, plain) > 366
    assert 'predictive' not in plain and 'quantiles' not in plain and 'gof' in plain
    po = sc['param_only']
    seen = ~np.isnan(po['crps'][0, :, 0])                                # an unobserved day is 0 and 0 too: it must be masked out
    hist = score.pit_histogram(po['below'][0, :, 0], po['at_or_below'][0, :, 0], E, 10, observed=seen)
    assert abs(hist.sum() - po['n_obs'][0, 0]) < 1e-9 and 0 < po['n_obs'][0, 0] == seen.sum()
    assert np.array_equal(hist, score.pit_histogram(po['below'][0, seen, 0], po['at_or_below'][0, seen, 0], E, 10))


def test_scores_under_log_weights_and_with_the_error_model(engine0):
    rng = np.random.default_rng(3)
    lw = rng.normal(0.0, 3.0, E)
    lw[::17] = -np.inf
    q = particle.weights(lw)['q']
    res = ensemble(to_host=False, quantile_log_weights=lw, predictive_series=['Q_cumecs', 'TDP_mgl'])
    assert res['scores']['series'] == ['Q_cumecs', 'TDP_mgl'] and res['scores']['n_members'] == int((q > 0).sum()) < E
    against_the_rule(engine0, res, weights=q)
    m = np.stack([rng.uniform(0.05, 0.4, E), np.full(E, 0.2)])
    res = ensemble(to_host=False, predictive_series=['Q_cumecs', 'TDP_mgl'], predictive_m={'Q_cumecs': m[0], 'TDP_mgl': 0.2})
    against_the_rule(engine0, res, m=m)
    po, ov = res['scores']['param_only'], res['scores']['overall']
    assert not np.array_equal(bits(po['crps']), bits(ov['crps'])) and (ov['n_obs'] == po['n_obs']).all()
    # the scores and the bands of one call describe one distribution: an observation under the 2.5 % value has F(y) <= 0.025
    both = ensemble(to_host=False, quantiles=[0.025], quantile_weights=np.exp(lw - lw.max()), predictive_series=['Q_cumecs'])
    band = both['predictive']['param_only']['data'][0, 0, :, 0]
    obs = vr.observation_array(helpers.observations(*[helpers.scenario_inputs(NAME)[2][k] for k in ('st_dt', 'end_dt')]), [1],
                               helpers.scenario_inputs(NAME)[0].index)[0, 0]
    T = both['scores']['weight_total']
    F_y = both['scores']['param_only']['at_or_below'][0, :, 0].astype(np.float64) / T
    seen = ~np.isnan(obs)
    assert (F_y[seen & (obs < band)] < 0.025).all() and (F_y[seen & (obs >= band)] >= 0.025).all() and seen.sum() > 300


def test_keep_daily_false_and_windows(engine0, plain):
    lean = ensemble(keep_daily=False)
    assert lean['data'] is None
    same_scores(plain['scores'], lean['scores'])
    rng = np.random.default_rng(5)
    kw = dict(quantile_weights=rng.uniform(0.0, 1.0, E), predictive_m=0.3, predictive_day0=1000, keep_daily=False)
    whole = ensemble(**kw)['scores']
    at = 0
    for item in ensemble(windows=100, **kw):
        lo, hi = item['window'][2:]
        assert lo == at and item['scores']['series'] == whole['series'] and item['scores']['day0'] == 1000 + lo
        same_scores(whole, item['scores'], days=slice(lo, hi))
        at = hi
    assert at == 366


def test_errors(engine0):
    for kw, msg in ((dict(obs_dict=None), 'score needs obs_dict'), (dict(reduce='annual'), 'cannot be combined with reduce'),
                    (dict(devices=[0]), r'devices=\[...\]'), (dict(predictive_m={'nonsense': 0.1}), 'predictive_m names'),
                    (dict(predictive_seed=-1), 'predictive_seed')):
        with pytest.raises(ValueError, match=msg):
            ensemble(**kw)
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
    with pytest.raises(ValueError, match='given without quantiles'):        # unchanged without score
        sp.run_simply_p_ensemble(met, p_struc, p_SU, p_LU, p_SC, p, dyn, overrides=overrides(), quantile_members=np.ones(E, dtype=bool))
    # observations of another reach only: nothing to score, and the call succeeds
    none = ensemble(obs_dict={7: helpers.observations(p_SU['st_dt'], p_SU['end_dt'])[1]}, days=slice(0, 40))['scores']
    assert none['series'] == [] and none['param_only']['crps'].shape == (0, 40, 1) and none['overall'] is None


# ---- the particle filter ---------------------------------------------------------------------------------------------------------

def filt(days=slice(None), **kw):
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
    obs_dict = helpers.observations(p_SU['st_dt'], p_SU['end_dt'])
    priors = {nm: (0.7 * float(p[nm]), 1.3 * float(p[nm])) for nm in ('fc', 'T_g', 'a_Q')}
    priors['m_Q'] = (0.01, 1.0)
    args = dict(priors=priors, variables=['Q'], n_particles=E, window=30, seed=SEED, record=True, score=True, resample_threshold=0.5)
    args.update(kw)
    return sp.assimilate(met.iloc[days], p_struc, p_SU, p_LU, p_SC, p, dyn, obs_dict, **args)


@pytest.fixture(scope='module')
def year(engine0):
    return filt()


def test_filter_windows_recomputed_from_the_record(engine0, year):
    res = year
    sc = res['scores']
    n = len(res['windows'])
    assert sc['series'][0] == 'Q_cumecs' and sc['param_only']['crps'].shape == (len(sc['series']), 366, 1)
    assert len(res['kernel_ms']['score']) == n == len(sc['weight_total']) and min(res['kernel_ms']['score']) > 0
    print('resampled:', res['resampled'].astype(int))
    fresh = [w for w in range(1, n) if res['resampled'][w - 1]]
    carried = [w for w in range(1, n) if not res['resampled'][w - 1]]
    assert fresh and carried, res['resampled']
    for w in (fresh[0], carried[0]):
        _, _, d_lo, d_hi = res['windows'][w]
        th = res['theta_before'][w]
        entering = np.ones(E) if res['resampled'][w - 1] else res['q'][w - 1].astype(np.float64)
        assert res['resampled'][w - 1] or len(np.unique(res['q'][w - 1])) > 1
        ens = ensemble(days=slice(d_lo, d_hi), overrides={nm: th[d] for d, nm in enumerate(res['names'][:3])},
                       initial_state=res['state_in'][w], quantile_weights=entering, predictive_m={'Q_cumecs': th[3]},
                       predictive_day0=d_lo, keep_daily=False)
        assert int(ens['status'].max()) == 0 and ens['scores']['series'] == sc['series']
        same_scores(sc, ens['scores'], days=slice(d_lo, d_hi))
        assert ens['scores']['weight_total'] == sc['weight_total'][w] and ens['scores']['n_members'] == sc['n_members'][w]
    # the first window is entered with equal weights: the plain ensemble call
    th = res['theta_before'][0]
    ens = ensemble(days=slice(0, 30), overrides={nm: th[d] for d, nm in enumerate(res['names'][:3])}, predictive_m={'Q_cumecs': th[3]},
                   keep_daily=False)
    for k in ('crps', 'abs_err', 'spread', 'pit'):
        assert np.array_equal(bits(ens['scores']['overall'][k]), bits(sc['overall'][k][:, :30])), k


def test_two_filter_calls_joined_by_state(engine0, year):
    first = filt(days=slice(0, 150))
    second = filt(days=slice(150, None), state=first['state'])
    for key in ('param_only', 'overall'):
        for k in ARRAYS:
            joined = np.concatenate([first['scores'][key][k], second['scores'][key][k]], axis=1)
            assert np.array_equal(bits(joined), bits(year['scores'][key][k])), (key, k)
    assert first['scores']['weight_total'] + second['scores']['weight_total'] == year['scores']['weight_total']
    quiet = filt(days=slice(0, 60), score=False)
    assert 'scores' not in quiet and 'score' not in quiet['kernel_ms']
    assert np.array_equal(bits(quiet['theta']), bits(first['theta_after'][1]))          # scoring does not touch the filter
