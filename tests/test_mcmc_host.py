"""The stretch move's NumPy statement (simplyp_amd/mcmc.py), the sampler's C ABI surface and the host-side checks of
sample_posterior.  No GPU.

Stationarity bounds: every walker's marginal stays the target under the move, so the W = 4096 final positions of a chain started
from exact N(0, I) draws have |mean| <= 5 / sqrt(W) = 0.078 and |var - 1| <= 5 sqrt(2 / W) = 0.110 per dimension -- five standard
errors of independent samples.  Measured with the seeds below: 0.022 / 0.006 (n_dim 2) and 0.024 / 0.039 (n_dim 5).  With the
(n_dim - 1) ln z term removed from mcmc.accept by hand the variances fell to 0.68-0.71 (n_dim 2) and 0.33-0.38 (n_dim 5): the
test fails then."""

import re

import numpy as np
import pytest

import helpers
import simplyp_amd as sp
from simplyp_amd import engine, mcmc

from c_header import header_text

NAME = 'tarland_2004_dynamic'


def gauss(x):
    return -0.5 * (x * x).sum(axis=0)


def test_exports():
    engine.build()
    L = engine.lib()
    declared = set(re.findall(r'\b(simplyp_mcmc_[a-z0-9_]+)\s*\(', header_text()))
    assert declared == {'simplyp_mcmc_propose', 'simplyp_mcmc_log_prob', 'simplyp_mcmc_accept'}
    for name in declared:
        assert name in engine.ABI_SYMBOLS and hasattr(L, name), name
    assert sp.sample_posterior is not None and 'sample_posterior' in sp.__all__


@pytest.mark.parametrize('n_dim', [2, 5])
def test_mirror_keeps_the_target(n_dim):
    W = 4096
    th = np.random.default_rng(100 + n_dim).standard_normal((n_dim, W))
    r = mcmc.run_chain(gauss, th, gauss(th), 50, [-np.inf] * n_dim, [np.inf] * n_dim, seed=1)
    f = r['theta']
    worst_mean, worst_var = np.abs(f.mean(axis=1)).max(), np.abs(f.var(axis=1) - 1.0).max()
    print('n_dim %d: |mean| %.4f, |var - 1| %.4f, acceptance %.3f' % (n_dim, worst_mean, worst_var, r['n_accept'].mean() / 50))
    assert worst_mean <= 5 / np.sqrt(W) and worst_var <= 5 * np.sqrt(2.0 / W)
    assert np.array_equal(r['lp'], gauss(f))
    assert 0.3 < r['n_accept'].mean() / 50 < 0.9


def test_structure_of_the_move():
    n_dim, W, h = 3, 64, 32
    lo, hi = np.array([0.0, -1.0, 2.0]), np.array([1.0, 1.0, 2.5])
    rng = np.random.default_rng(5)
    th = lo[:, None] + (hi - lo)[:, None] * rng.uniform(size=(n_dim, W))
    seen_outside = 0
    for a in (2.0, 3.5):
        for t in range(20):
            for half in (0, 1):
                i, j, z = mcmc.stretch(W, half, t, a, seed=9)
                assert np.array_equal(i, half * h + np.arange(h))
                assert ((j >= (1 - half) * h) & (j < (2 - half) * h)).all()          # the partner is in the other half
                assert (z >= 1 / a).all() and (z <= a).all()
                pr = mcmc.propose(th, half, t, lo, hi, a, seed=9)
                assert np.array_equal(pr['partner'], j) and np.array_equal(pr['z'], z)
                inside = ((pr['run_point'] >= lo[:, None]) & (pr['run_point'] < hi[:, None])).all(axis=0)
                assert inside.all()                                                  # the target never sees a point outside
                seen_outside += int((~pr['inside']).sum())
    assert seen_outside > 0
    # a flat target on the box: every inside proposal with margin > 0 is taken, and no position ever leaves [lo, hi)
    r = mcmc.run_chain(lambda x: np.zeros(x.shape[1]), th, np.zeros(W), 40, lo, hi, seed=9)
    c = r['chain']
    assert c.shape == (40, n_dim, W)
    assert ((c >= lo[None, :, None]) & (c < hi[None, :, None])).all()
    assert sum(r['n_inside']) < 80 * h and 0 < sum(r['n_accepted']) <= sum(r['n_inside'])
    # a NaN position is outside
    bad = th.copy(); bad[1, 40] = np.nan
    pr = mcmc.propose(bad, 1, 0, lo, hi, seed=9)
    assert not pr['inside'][40 - h]
    # two walkers: each half has the one partner
    th2 = np.array([[0.25, 0.75]])
    for half in (0, 1):
        i, j, z = mcmc.stretch(2, half, 3, seed=1)
        assert i.tolist() == [half] and j.tolist() == [1 - half]
    r2 = mcmc.run_chain(gauss, th2, gauss(th2), 30, [0.0], [1.0], seed=1)
    assert r2['chain'].shape == (30, 1, 2) and 0 < r2['n_accept'].sum() < 60
    assert ((r2['chain'] >= 0.0) & (r2['chain'] < 1.0)).all()


def test_thinning_and_shape_errors():
    th = np.random.default_rng(2).standard_normal((2, 8))
    full = mcmc.run_chain(gauss, th, gauss(th), 12, [-9.0] * 2, [9.0] * 2, seed=4)
    thin = mcmc.run_chain(gauss, th, gauss(th), 12, [-9.0] * 2, [9.0] * 2, seed=4, thin=3)
    assert np.array_equal(thin['chain'], full['chain'][2::3]) and np.array_equal(thin['log_prob'], full['log_prob'][2::3])
    for W, n_dim, a in ((7, 2, 2.0), (2, 2, 2.0), (8, 0, 2.0), (40, 17, 2.0), (8, 2, 1.0), (8, 2, float('nan'))):
        with pytest.raises(ValueError):
            mcmc.check_shape(W, n_dim, a)
    with pytest.raises(ValueError):
        mcmc.propose(th, 0, 0, [0.0, 1.0], [1.0, 1.0])
    with pytest.raises(ValueError):
        mcmc.propose(th, 2, 0, [0.0, 0.0], [1.0, 1.0])


def test_continuation_is_bit_for_bit():
    n_dim, W = 4, 32
    th = np.random.default_rng(8).standard_normal((n_dim, W))
    lo, hi = [-3.0] * n_dim, [3.0] * n_dim
    whole = mcmc.run_chain(gauss, th, gauss(th), 11, lo, hi, seed=77)
    first = mcmc.run_chain(gauss, th, gauss(th), 4, lo, hi, seed=77)
    second = mcmc.run_chain(gauss, first['theta'], first['lp'], 7, lo, hi, seed=77, t0=first['t'], n_accept=first['n_accept'])
    assert second['t'] == whole['t'] == 11
    assert np.array_equal(np.concatenate([first['chain'], second['chain']]), whole['chain'])
    assert np.array_equal(np.concatenate([first['log_prob'], second['log_prob']]), whole['log_prob'])
    assert np.array_equal(second['n_accept'], whole['n_accept'])
    other = mcmc.run_chain(gauss, th, gauss(th), 11, lo, hi, seed=78)
    assert not np.array_equal(other['chain'], whole['chain'])


def call(obs='default', **kw):
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
    obs_dict = helpers.observations(p_SU['st_dt'], p_SU['end_dt']) if isinstance(obs, str) else obs
    args = dict(priors={'fc': (200.0, 380.0), 'T_g': (45.0, 85.0), 'm_Q': (0.01, 1.0)}, variables=['Q'], n_walkers=8, n_steps=1)
    args.update(kw)
    return sp.sample_posterior(met, p_struc, p_SU, p_LU, p_SC, p, dyn, obs_dict, **args)


def test_sample_posterior_argument_errors_need_no_gpu(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call was made before the arguments were checked")
    monkeypatch.setattr(engine, 'get_engine', no_device)
    box = {'fc': (200.0, 380.0), 'T_g': (45.0, 85.0), 'm_Q': (0.01, 1.0)}
    with pytest.raises(ValueError, match='even'):
        call(n_walkers=9)
    with pytest.raises(ValueError, match='2 n_dim'):
        call(n_walkers=4)
    with pytest.raises(ValueError, match='unknown parameter'):
        call(priors=dict(box, no_such=(0.0, 1.0)))
    with pytest.raises(ValueError, match='unknown parameter'):
        call(priors=dict(box, m_SS=(0.0, 1.0)))                      # an m of a variable that is not selected
    with pytest.raises(ValueError, match='unknown parameter'):
        call(priors=dict(box, A_catch=(40.0, 60.0)))                 # reach parameters are out of scope
    with pytest.raises(ValueError, match='lo < hi'):
        call(priors=dict(box, fc=(300.0, 300.0)))
    with pytest.raises(ValueError, match='lo < hi'):
        call(priors=dict(box, fc=(float('nan'), 300.0)))
    with pytest.raises(ValueError, match='error model'):
        call(priors={'fc': (200.0, 380.0)})                          # m_Q neither sampled nor fixed
    with pytest.raises(ValueError, match='outside the prior box'):
        call(start=np.full((3, 8), 500.0))
    with pytest.raises(ValueError, match='outside the prior box'):
        call(priors=dict(box, fc=(300.0, 380.0)))                    # the ball around the workbook's fc = 290
    with pytest.raises(ValueError, match='shape'):
        call(start=np.zeros((2, 8)))
    with pytest.raises(ValueError, match='obs_dict'):
        call(obs=None)
    few = helpers.observations('2004-01-01', '2004-12-31')
    few[1] = few[1].copy()
    few[1].loc[few[1].index[10:], 'Q'] = np.nan                      # 10 observations of Q: the reference drops the row
    with pytest.raises(ValueError, match='10 or fewer'):
        call(obs=few)
    with pytest.raises(ValueError, match='model rejects'):
        call(priors=dict(box, d_maxE_spr=(20.0, 120.0)))             # marshal.validate_ensemble: must lie in (30, 335)
    with pytest.raises(ValueError, match='stretch scale'):
        call(a=1.0)
