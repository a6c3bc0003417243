"""Weighted bands through the public calls: ``run_simply_p_ensemble(quantile_weights= / quantile_log_weights=)`` and
``assimilate(forecast_weighted=True)`` against the Python-integer statement of the rule (simplyp_amd/weighted.py) on the tables
the calls return.  Bit for bit, -0.0 and +0.0 counting as equal; no tolerance.

Where numpy's own ``method='inverted_cdf'`` is the yardstick (equal weights), the member counts and probabilities are such that
numpy's fp64 product p n cannot round across an integer: n = 300 gives 7.5 / 150 / 292.5 and n = 256 gives 6.4 / 128 / 249.6
for p = 0.025 / 0.5 / 0.975 (0.5 is exact)."""

import numpy as np
import pytest

import helpers
import simplyp_amd as sp
from simplyp_amd import abi, marshal, particle, weighted

import weighted_cases as wc

pytestmark = pytest.mark.gpu

NAME = 'tarland_2004_dynamic'
FLUX = ['Qr', 'Msus_kg/day', 'TDP_kg/day', 'PP_kg/day']
Q_BAND = [0.025, 0.5, 0.975]
E_ENS = 300
SEED_ENS = 41
M_Q = 0.15


def dev(eng, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(eng.tdev)


def overrides_for(E, seed=3):
    base = helpers.marshal_scenario(NAME, E=1)['member_params'][:, 0]
    rng = np.random.default_rng(seed)
    return {pname: base[marshal.PM_NAMES.index(pname)] * rng.uniform(lo, hi, E)
            for pname, lo, hi in (('a_Q', 0.6, 1.6), ('T_g', 0.7, 1.4), ('E_M', 0.5, 2.0), ('fc', 0.85, 1.15))}


def ensemble(days=120, **kw):
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
    kw = dict(dict(overrides=overrides_for(E_ENS), outputs=FLUX, quantiles=Q_BAND), **kw)
    return sp.run_simply_p_ensemble(met.iloc[:days], p_struc, p_SU, p_LU, p_SC, p, dyn, **kw)


def q_cumecs(res):
    """The df_R series Q_cumecs [1, D, 1, E] of a returned table, the reference's operations one after the other."""
    A = float(helpers.scenario_inputs(NAME)[4].loc['A_catch', 1])
    return (res['data'][res['columns'].index('Qr')] * A * 1000 / 86400)[None]


def check_every_band(engine0, res, q):
    """Every band across the members the call returned against the mirror on the tables it returned."""
    assert (res['status'] & abi.STATUS_NONFINITE == 0).all()
    T, n_used = sum(int(v) for v in q), int((np.asarray(q) > 0).sum())
    band = res['quantiles']
    assert band['rule'] == 'inverted_cdf' and band['weight_total'] == T and band['n_members'] == n_used
    assert band['data'].shape == (3,) + res['data'].shape[:-1]
    assert wc.same_bits(band['data'], weighted.quantiles(res['data'], q, Q_BAND))
    assert band['lower'] is band['data'] or wc.same_bits(band['lower'], band['data']) and wc.same_bits(band['upper'], band['data'])
    tq = res['time_quantiles']
    assert tq['quantiles']['rule'] == 'inverted_cdf' and tq['quantiles']['weight_total'] == T
    assert wc.same_bits(tq['quantiles']['data'], weighted.quantiles(tq['data'], q, Q_BAND))
    pred = res['predictive']
    assert pred['rule'] == 'inverted_cdf' and pred['weight_total'] == T and pred['n_members'] == n_used
    x = q_cumecs(res)
    assert pred['param_only']['data'].shape == (3, 1, x.shape[1], 1)
    assert wc.same_bits(pred['param_only']['data'], weighted.quantiles(x, q, Q_BAND))
    rp = np.zeros((len(marshal.PR_NAMES), 1, E_ENS))
    rp[marshal.PR_NAMES.index('A_catch')] = float(helpers.scenario_inputs(NAME)[4].loc['A_catch', 1])
    noisy = engine0.predictive_series(dev(engine0, res['data']), marshal.mask_of_columns(res['columns']),
                                      [abi.TQ_DERIVED + abi.TQ_DERIVED_SERIES.index('Q_cumecs')], err_m=np.full((1, E_ENS), M_Q),
                                      seed=SEED_ENS, day0=0, f_tdp=0.5, reach_params=rp).cpu().numpy()
    assert wc.same_bits(pred['overall']['data'], weighted.quantiles(noisy, q, Q_BAND))
    return x


ALL = dict(time_quantiles=[0.05, 0.5], time_quantile_series=['Q_cumecs'], predictive_series=['Q_cumecs'],
           predictive_m={'Q_cumecs': M_Q}, predictive_seed=SEED_ENS)


def test_ensemble_log_weights(engine0):
    lw = np.random.default_rng(8).uniform(-40.0, -3.0, E_ENS)                 # some members fall below 2^-40 of the best
    lw[[5, 77]] = -np.inf, np.nan
    q = particle.weights(lw)['q']
    assert 0 < int((q == 0).sum()) < E_ENS // 2
    check_every_band(engine0, ensemble(quantile_log_weights=lw, **ALL), q)


def test_ensemble_linear_weights(engine0):
    w = np.random.default_rng(9).uniform(0.0, 5.0, E_ENS) ** 4
    w[[3, 200]] = 0.0
    check_every_band(engine0, ensemble(quantile_weights=w, **ALL), weighted.linear_weights(w))


def test_ensemble_unit_weights_give_numpys_inverted_cdf(engine0):
    res = ensemble(quantile_weights=np.ones(E_ENS), **ALL)
    x = check_every_band(engine0, res, np.full(E_ENS, 1 << 40, dtype=np.uint64))
    assert res['quantiles']['n_members'] == E_ENS
    assert wc.same_bits(res['quantiles']['data'], np.quantile(res['data'], Q_BAND, axis=-1, method='inverted_cdf'))
    assert wc.same_bits(res['predictive']['param_only']['data'], np.quantile(x, Q_BAND, axis=-1, method='inverted_cdf'))
    # without weights nothing changes: the 'linear' band, no rule key
    plain = ensemble()
    assert 'rule' not in plain['quantiles'] and np.allclose(plain['quantiles']['data'], np.quantile(plain['data'], Q_BAND, axis=-1), rtol=1e-14)


def test_ensemble_quantile_members_and_reduce(engine0):
    rng = np.random.default_rng(10)
    w = rng.uniform(0.0, 1.0, E_ENS)
    keep = rng.random(E_ENS) < 0.6
    res = ensemble(quantile_weights=w, quantile_members=keep, reduce='annual')
    q = weighted.linear_weights(w)
    assert res['data'].shape[1] == 1
    assert wc.same_bits(res['quantiles']['data'], weighted.quantiles(res['data'], q, Q_BAND, include=keep))
    assert res['quantiles']['weight_total'] == sum(int(v) for v in q[keep])


def test_ensemble_errors(engine0):
    ok = np.ones(E_ENS)
    for kw, msg in ((dict(quantile_weights=np.ones(E_ENS + 1)), 'one weight per member'),
                    (dict(quantile_log_weights=np.zeros((2, E_ENS))), 'one log weight per member'),
                    (dict(quantile_weights=-ok), 'finite and >= 0'), (dict(quantile_weights=ok * np.nan), 'finite and >= 0'),
                    (dict(quantile_weights=ok * np.inf), 'finite and >= 0'), (dict(quantile_weights=0 * ok), 'all weights are zero'),
                    (dict(quantile_log_weights=ok * -np.inf), 'all weights are zero'),
                    (dict(quantile_weights=ok, quantile_log_weights=ok), 'mutually exclusive'),
                    (dict(quantile_weights=ok, quantiles=None), 'without quantiles'),
                    (dict(quantile_log_weights=ok, quantiles=None), 'without quantiles'),
                    (dict(quantile_weights=ok, devices=[0]), 'devices')):
        with pytest.raises(ValueError, match=msg):
            ensemble(days=20, **kw)


# ---- assimilate(forecast_weighted=True): the scenario and particle count of tests/test_gpu_particle.py --------------------------
E_PUB, SEED_PUB = 256, 11


def public(days=slice(0, 90), **kw):
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
    obs_dict = helpers.observations(p_SU['st_dt'], p_SU['end_dt'])
    priors = {nm: (0.7 * float(p[nm]), 1.3 * float(p[nm])) for nm in ('fc', 'T_g', 'a_Q')}
    priors['m_Q'] = (0.01, 1.0)
    args = dict(priors=priors, variables=['Q'], n_particles=E_PUB, window=30, seed=SEED_PUB, record=True, quantiles=Q_BAND,
                forecast_weighted=True, resample_threshold=0.5)
    args.update(kw)
    return sp.assimilate(met.iloc[days], p_struc, p_SU, p_LU, p_SC, p, dyn, obs_dict, **args)


def window_series(res, w):
    """Q_cumecs [1, 30, 1, E] of window w from an independent ensemble call started from the recorded state and positions."""
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
    th = res['theta_before'][w]
    ens = sp.run_simply_p_ensemble(met.iloc[30 * w:30 * (w + 1)], p_struc, p_SU, p_LU, p_SC, p, dyn, outputs=FLUX,
                                   overrides={nm: th[d] for d, nm in enumerate(res['names'][:3])},
                                   initial_state=res['state_in'][w])
    return q_cumecs(ens)


# 0.5: the issue's case (on this scenario every window's ESS falls below 128, so every window resamples); 0.0: never resample,
# so that every window after the first enters with the weights the log weights have accumulated -- the path 0.5 leaves unrun
@pytest.fixture(scope='module', params=[0.5, 0.0])
def filtered(engine0, request):
    return public(resample_threshold=request.param), request.param


def test_forecast_bands_carry_the_weights_the_particles_enter_with(engine0, filtered):
    res, threshold = filtered
    fc = res['forecast']
    assert threshold > 0 or not res['resampled'].any()
    assert fc['rule'] == 'inverted_cdf' and fc['param_only'].shape == (3, 1, 90, 1) == fc['overall'].shape
    print('resampled:', res['resampled'], 'ess:', res['ess'])
    equal = np.full(E_PUB, 1 << 40, dtype=np.uint64)
    for w in range(2):
        q = equal if res['resampled'][w] else res['q'][w]
        x = window_series(res, w + 1)
        assert wc.same_bits(fc['param_only'][:, :, 30 * (w + 1):30 * (w + 2)], weighted.quantiles(x, q, Q_BAND)), w
    # the first window: the start is equally weighted
    assert wc.same_bits(fc['param_only'][:, :, :30], weighted.quantiles(window_series(res, 0), equal, Q_BAND))
    assert (fc['overall'][0] <= fc['overall'][2]).all() and np.isfinite(fc['overall']).all()


def test_always_resampling_gives_numpys_inverted_cdf_bands(engine0):
    res = public(resample_threshold=1.0)
    assert res['resampled'].all() and res['forecast']['rule'] == 'inverted_cdf'
    for w in range(3):
        want = np.quantile(window_series(res, w), Q_BAND, axis=-1, method='inverted_cdf')
        assert wc.same_bits(res['forecast']['param_only'][:, :, 30 * w:30 * (w + 1)], want), w


def test_two_calls_joined_by_state_equal_the_single_call(engine0, filtered):
    res, threshold = filtered
    first = public(days=slice(0, 60), resample_threshold=threshold)
    second = public(days=slice(60, 90), state=first['state'], seed=999, resample_threshold=threshold)     # the state's seed holds
    for k in ('param_only', 'overall'):
        joined = np.concatenate([first['forecast'][k], second['forecast'][k]], axis=2)
        assert np.array_equal(joined.view(np.uint64), res['forecast'][k].view(np.uint64)), k
    assert np.array_equal(np.concatenate([first['resampled'], second['resampled']]), res['resampled'])


def test_the_default_still_refuses_unweighted_bands_of_weighted_particles(engine0):
    with pytest.raises(ValueError, match='forecast_weighted=True'):
        public(days=slice(0, 60), forecast_weighted=False)
    res = public(days=slice(0, 60), forecast_weighted=False, resample_threshold=1.0)
    assert 'rule' not in res['forecast']
