"""The device's stretch move (simplyp_mcmc_propose / _log_prob / _accept) against its NumPy statement (simplyp_amd/mcmc.py), and
sample_posterior end to end.

Partner, z, y and the box test are integer arithmetic or + * / in fp64 on both sides: compared bit for bit.  A decision depends on
margin = (n_dim - 1) ln z + lp_y - lp_i - ln u_a, which carries the rounding of two logarithms (a few 1e-16 relative on terms of
size <= 40): each test that compares decisions first asserts on the CPU that the mirror's smallest |margin| exceeds 1e-9.
log_prob against visualise_results.loglik of the downloaded table: 1e-12 relative (the same operations on the same numbers but
for the device's own log).  The public call's lp against an independent ensemble run at the same positions: 1e-12 relative (same
kernels, independent members; the goodness-of-fit sums may be chunked differently)."""

import numpy as np
import pytest
import torch

import helpers
import simplyp_amd as sp
from simplyp_amd import abi, engine, marshal, mcmc, visualise_results as vr

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1), (64, 3), (130, 5), (514, 16)]
NAME = 'tarland_2004_dynamic'
FLUX = ['Qr', 'Msus_kg/day', 'TDP_kg/day', 'PP_kg/day']
SENTINEL = -777.25


def dev(eng, a, dtype=torch.float64):
    return eng.to_device(np.ascontiguousarray(a), dtype)


def problem(W, n_dim, seed=0):
    """Positions inside a box that the stretch move leaves often, and targets that name rows, f_tdp and nothing."""
    rng = np.random.default_rng(1000 * W + n_dim + seed)
    lo = -1.0 - np.arange(n_dim) * 0.125
    hi = 1.5 + np.arange(n_dim) * 0.25
    theta = lo[:, None] + (hi - lo)[:, None] * rng.uniform(size=(n_dim, W))
    target = np.array([2, abi.MCMC_TARGET_F_TDP, abi.MCMC_TARGET_NONE] + list(range(5, 5 + n_dim)), dtype=np.int32)[:n_dim]
    return theta, lo, hi, target


@pytest.mark.parametrize('W,n_dim', SHAPES)
def test_propose_matches_the_mirror_bit_for_bit(engine0, W, n_dim):
    h = W // 2
    theta, lo, hi, target = problem(W, n_dim)
    th_d = dev(engine0, theta)
    outside = 0
    for half in (0, 1):
        for t in (0, 7, 2 ** 32 - 1):
            want = mcmc.propose(theta, half, t, lo, hi, a=2.5, seed=0xDEADBEEF12345678)
            prop = torch.full((n_dim, h), SENTINEL, dtype=torch.float64, device=engine0.tdev)
            inside = torch.full((h,), -5, dtype=torch.int32, device=engine0.tdev)
            mp = torch.full((marshal.NP_M, h), SENTINEL, dtype=torch.float64, device=engine0.tdev)
            ft = torch.full((h,), SENTINEL, dtype=torch.float64, device=engine0.tdev)
            info = engine0.mcmc_propose(th_d, half, t, lo, hi, target, prop, inside, mp, ft, a=2.5, seed=0xDEADBEEF12345678)
            assert np.array_equal(prop.cpu().numpy(), want['prop'])
            assert np.array_equal(inside.cpu().numpy(), want['inside'].astype(np.int32))
            assert info['n_inside'] == int(want['inside'].sum()) and info['n_accepted'] == 0 and info['n_nan'] == 0
            got_mp, got_ft = mp.cpu().numpy(), ft.cpu().numpy()
            named = set()
            for d in range(n_dim):
                if target[d] >= 0:
                    assert np.array_equal(got_mp[target[d]], want['run_point'][d]), d
                    named.add(int(target[d]))
                elif target[d] == abi.MCMC_TARGET_F_TDP:
                    assert np.array_equal(got_ft, want['run_point'][d])
            rest = [r for r in range(marshal.NP_M) if r not in named]
            assert (got_mp[rest] == SENTINEL).all()                        # rows that no dimension names are not touched
            if n_dim < 2:
                assert (got_ft == SENTINEL).all()
            # the run point: the proposal inside the box, the walker's own position outside
            i = half * h + np.arange(h)
            assert np.array_equal(want['run_point'], np.where(want['inside'], want['prop'], theta[:, i]))
            outside += int((~want['inside']).sum())
    assert np.array_equal(th_d.cpu().numpy(), theta)
    if W > 2:
        assert 0 < outside < 6 * h


def caller_lp(rng, lp_i, h):
    """ln p of the proposals as a caller might hand them over: around the current values, with -inf and NaN among them."""
    lp_y = lp_i + rng.normal(0.0, 1.5, h)
    if h >= 8:
        lp_y[rng.choice(h, h // 8, replace=False)] = -np.inf
        lp_y[rng.choice(h, h // 8, replace=False)] = np.nan
    return lp_y


@pytest.mark.parametrize('W,n_dim', SHAPES)
def test_accept_matches_the_mirror(engine0, W, n_dim):
    h = W // 2
    theta, lo, hi, _ = problem(W, n_dim)
    rng = np.random.default_rng(W + 17)
    lp = rng.normal(-20.0, 3.0, W)
    seed, t, a = 20240607, 41, 2.0
    # the mirror first: both halves of step t, and the margin condition
    m_theta, m_lp, m_acc = theta.copy(), lp.copy(), np.zeros(W, dtype=np.int64)
    steps = []
    for half in (0, 1):
        pr = mcmc.propose(m_theta, half, t, lo, hi, a, seed)
        lp_y = caller_lp(rng, m_lp[half * h:(half + 1) * h], h)
        acc, margin = mcmc.accept(m_theta, m_lp, m_acc, half, t, pr['prop'], pr['inside'], lp_y, a, seed)
        settled = pr['inside'] & np.isfinite(margin)
        assert not settled.any() or np.abs(margin[settled]).min() > 1e-9
        steps.append((pr, lp_y, acc))
    th_d, lp_d = dev(engine0, theta), dev(engine0, lp)
    nacc_d = torch.zeros((W,), dtype=torch.int32, device=engine0.tdev)
    row = torch.full((n_dim + 1, W), SENTINEL, dtype=torch.float64, device=engine0.tdev)
    target = np.full(n_dim, abi.MCMC_TARGET_NONE, dtype=np.int32)
    for half, (pr, lp_y, acc) in enumerate(steps):
        prop = torch.empty((n_dim, h), dtype=torch.float64, device=engine0.tdev)
        inside = torch.empty((h,), dtype=torch.int32, device=engine0.tdev)
        engine0.mcmc_propose(th_d, half, t, lo, hi, target, prop, inside, a=a, seed=seed)
        assert np.array_equal(prop.cpu().numpy(), pr['prop'])
        info = engine0.mcmc_accept(th_d, lp_d, nacc_d, half, t, prop, inside, dev(engine0, lp_y), chain_row=row, a=a, seed=seed)
        assert info['n_inside'] == int(pr['inside'].sum()) and info['n_accepted'] == int(acc.sum())
        assert info['n_nan'] == int(np.isnan(lp_y).sum())
        if half == 0:                                  # the other half's lanes of the chain row are still untouched
            assert (row.cpu().numpy()[:, h:] == SENTINEL).all()
    assert np.array_equal(th_d.cpu().numpy(), m_theta)
    assert np.array_equal(lp_d.cpu().numpy(), m_lp)
    assert np.array_equal(nacc_d.cpu().numpy(), m_acc)
    got_row = row.cpu().numpy()
    assert np.array_equal(got_row[:n_dim], m_theta) and np.array_equal(got_row[n_dim], m_lp)
    if W > 2:
        assert 0 < m_acc.sum() < W
    # without a chain row nothing else changes
    th2, lp2, n2 = dev(engine0, theta), dev(engine0, lp), torch.zeros((W,), dtype=torch.int32, device=engine0.tdev)
    pr, lp_y, acc = steps[0]
    engine0.mcmc_accept(th2, lp2, n2, 0, t, dev(engine0, pr['prop']), dev(engine0, pr['inside'], torch.int32), dev(engine0, lp_y),
                        a=a, seed=seed)
    assert np.array_equal(n2.cpu().numpy()[:h], acc.astype(np.int32)) and (n2.cpu().numpy()[h:] == 0).all()


def corr_gauss(x):
    """ln p of a 2-D Gaussian with unit variances and correlation 0.9, element by element."""
    return -0.5 * ((x[0] * x[0] - 1.8 * x[0] * x[1] + x[1] * x[1]) / 0.19)


def test_a_whole_chain_through_the_abi(engine0):
    W, n_dim, n_steps, seed = 512, 2, 30, 5
    h = W // 2
    lo, hi = np.array([-2.5, -3.0]), np.array([3.0, 2.5])
    theta = np.random.default_rng(3).uniform(-1.0, 1.0, (n_dim, W))
    lp = corr_gauss(theta)
    want = mcmc.run_chain(corr_gauss, theta, lp, n_steps, lo, hi, seed=seed, t0=100)
    assert want['min_abs_margin'] > 1e-9, want['min_abs_margin']
    assert sum(want['n_inside']) < 2 * n_steps * h                 # the box cuts proposals off
    th_d, lp_d = dev(engine0, theta), dev(engine0, lp)
    nacc_d = torch.zeros((W,), dtype=torch.int32, device=engine0.tdev)
    chain = torch.empty((n_steps, n_dim + 1, W), dtype=torch.float64, device=engine0.tdev)
    prop = torch.empty((n_dim, h), dtype=torch.float64, device=engine0.tdev)
    inside = torch.empty((h,), dtype=torch.int32, device=engine0.tdev)
    target = np.full(n_dim, abi.MCMC_TARGET_NONE, dtype=np.int32)
    n_in, n_acc = [], []
    for n in range(n_steps):
        for half in (0, 1):
            pinfo = engine0.mcmc_propose(th_d, half, 100 + n, lo, hi, target, prop, inside, seed=seed)
            lp_y = corr_gauss(prop.cpu().numpy())                  # the caller's own target, from the downloaded proposals
            ainfo = engine0.mcmc_accept(th_d, lp_d, nacc_d, half, 100 + n, prop, inside, dev(engine0, lp_y), chain_row=chain[n], seed=seed)
            n_in.append(pinfo['n_inside']); n_acc.append(ainfo['n_accepted'])
    got = chain.cpu().numpy()
    assert np.array_equal(got[:, :n_dim], want['chain']) and np.array_equal(got[:, n_dim], want['log_prob'])
    assert np.array_equal(nacc_d.cpu().numpy(), want['n_accept'])
    assert n_in == want['n_inside'] and n_acc == want['n_accepted']


@pytest.fixture(scope='module')
def gof_table(engine0):
    E = 64
    m = helpers.marshal_scenario(NAME, E=E, out_mask=marshal.mask_of_columns(FLUX))
    rng = np.random.default_rng(11)
    for pname, lo, hi in (('a_Q', 0.7, 1.4), ('T_g', 0.7, 1.4), ('fc', 0.85, 1.15)):
        m['member_params'][marshal.PM_NAMES.index(pname)] *= rng.uniform(lo, hi, E)
    out, status, _ = engine0.run(m['forcing'], m['doy'], m['member_params'], m['reach_params'], m['up_ptr'], m['up_idx'], m['opts'])
    obs = vr.observation_array(helpers.observations('2004-01-01', '2004-12-31'), [1], m['met'].index)
    gof, _ = engine0.gof(out, marshal.mask_of_columns(FLUX), obs, 0.7, m['reach_params'])
    assert int(status.cpu().numpy().max()) == 0
    return gof, status, gof.cpu().numpy()


def test_log_prob_equals_loglik_of_the_table(engine0, gof_table):
    gof, status, g = gof_table
    E = g.shape[-1]
    rng = np.random.default_rng(12)
    prop = np.stack([rng.uniform(200, 300, E), rng.uniform(0.05, 0.9, E), rng.uniform(0.1, 0.6, E)])
    prop_d = dev(engine0, prop)
    q, tdp = abi.GOF_VARS.index('Q'), abi.GOF_VARS.index('TDP')
    cases = [([(q, 0)], {q: 1}, {}),                                  # one variable, m sampled
             ([(q, 0)], {}, {q: 0.25}),                               # one variable, m fixed
             ([(q, 0), (tdp, 0)], {q: 1, tdp: 2}, {}),                # two variables, both sampled
             ([(tdp, 0), (q, 0)], {q: 1}, {tdp: 0.4})]                # two variables, one fixed
    for pairs, sampled, fixed in cases:
        m_dim = [sampled.get(v, -1) for v in range(6)]
        m_const = [fixed.get(v, float('nan')) for v in range(6)]
        lp = torch.full((E,), SENTINEL, dtype=torch.float64, device=engine0.tdev)
        info = engine0.mcmc_log_prob(gof, pairs, m_dim, m_const, prop_d, lp, status=status)
        want = sum(vr.loglik(g, prop[sampled[v]] if v in sampled else fixed[v])[v, r] for v, r in pairs)
        got = lp.cpu().numpy()
        assert np.isfinite(want).all()
        assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all(), np.abs(got / want - 1).max()
        assert info['n_inside'] == E and info['n_nan'] == 0 and info['n_accepted'] == 0


def test_log_prob_is_minus_infinity_where_the_point_does_not_count(engine0, gof_table):
    gof, status, g = gof_table
    E = g.shape[-1]
    q = abi.GOF_VARS.index('Q')
    prop = np.full((1, E), 0.3)
    prop[0, 5], prop[0, 6] = 0.0, -0.1                                   # m <= 0
    inside = np.ones(E, dtype=np.int32); inside[[0, 33]] = 0
    st = np.zeros(E, dtype=np.int32); st[7] = abi.STATUS_NONFINITE; st[8] = abi.STATUS_STEPCAP
    lp = torch.full((E,), SENTINEL, dtype=torch.float64, device=engine0.tdev)
    m_dim = [0 if v == q else -1 for v in range(6)]
    info = engine0.mcmc_log_prob(gof, [(q, 0)], m_dim, [float('nan')] * 6, dev(engine0, prop), lp,
                                 status=dev(engine0, st, torch.int32), inside=dev(engine0, inside, torch.int32))
    got = lp.cpu().numpy()
    bad = [0, 33, 5, 6, 7]
    assert (got[bad] == -np.inf).all()
    ok = np.setdiff1d(np.arange(E), bad)
    want = vr.loglik(g, 0.3)[q, 0]
    assert (np.abs(got[ok] - want[ok]) <= 1e-12 * np.abs(want[ok])).all()       # the step-cap bit does not disqualify
    assert info['n_inside'] == E - 2
    # a NaN sum (a poisoned table entry) gives -inf and is counted
    g2 = gof.clone()
    g2[abi.GOF_STATS.index('sum_relsq'), q, 0, 11] = float('nan')
    info = engine0.mcmc_log_prob(g2, [(q, 0)], [-1] * 6, [0.3] * 6, dev(engine0, prop), lp)
    got = lp.cpu().numpy()
    assert got[11] == -np.inf and info['n_nan'] == 1 and np.isfinite(np.delete(got, 11)).all()


# ---- the public call ----------------------------------------------------------------------------------------------------

W_PUB, STEPS_PUB, SEED_PUB = 64, 6, 11


def public(**kw):
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
    obs_dict = helpers.observations(p_SU['st_dt'], p_SU['end_dt'])
    priors = {nm: (0.7 * float(p[nm]), 1.3 * float(p[nm])) for nm in ('fc', 'T_g', 'a_Q')}
    priors['m_Q'] = (0.01, 1.0)
    args = dict(priors=priors, variables=['Q'], n_walkers=W_PUB, n_steps=STEPS_PUB, seed=SEED_PUB, record_proposals=True)
    args.update(kw)
    return sp.sample_posterior(met, p_struc, p_SU, p_LU, p_SC, p, dyn, obs_dict, **args), priors, obs_dict


@pytest.fixture(scope='module')
def res6(engine0):
    return public()


def test_public_lp_equals_an_independent_ensemble_run(engine0, res6):
    res, priors, obs_dict = res6
    assert res['names'] == ['fc', 'T_g', 'a_Q', 'm_Q']
    assert res['chain'].shape == (STEPS_PUB, 4, W_PUB) and res['log_prob'].shape == (STEPS_PUB, W_PUB)
    flat = res['chain'].transpose(1, 0, 2).reshape(4, -1)
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
    ens = sp.run_simply_p_ensemble(met, p_struc, p_SU, p_LU, p_SC, p, dyn, overrides={nm: flat[d] for d, nm in enumerate(res['names'][:3])},
                                   obs_dict=obs_dict, keep_daily=False)
    assert int(ens['status'].max()) == 0
    want = vr.loglik(ens['gof']['data'], flat[3])[abi.GOF_VARS.index('Q'), 0]
    got = res['log_prob'].reshape(-1)
    assert np.isfinite(got).all()
    assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all(), np.abs(got / want - 1).max()
    # every position is inside its box
    for d, nm in enumerate(res['names']):
        assert (res['chain'][:, d] >= priors[nm][0]).all() and (res['chain'][:, d] < priors[nm][1]).all()
    assert 0.0 < res['acceptance_fraction'].mean() < 1.0
    assert len(res['stats']['wall_ms']) == 2 * STEPS_PUB and min(res['stats']['run_kernel_ms']) > 0.0


def test_public_chain_is_the_mirrors_replay_of_the_recorded_proposals(engine0, res6):
    res, priors, _ = res6
    h = W_PUB // 2
    lo = np.array([priors[nm][0] for nm in res['names']]); hi = np.array([priors[nm][1] for nm in res['names']])
    calls = iter([(n, k) for n in range(STEPS_PUB) for k in (0, 1)])

    def recorded(points):
        n, k = next(calls)
        lp_y = res['proposal_log_prob'][n, k * h:(k + 1) * h]
        ran = np.isfinite(lp_y)                                    # where the model ran at the proposal, it is the recorded one
        assert np.array_equal(points[:, ran], res['proposals'][n, :, k * h:(k + 1) * h][:, ran])
        return lp_y

    st = res['start']
    rep = mcmc.run_chain(recorded, st['theta'], st['lp'], STEPS_PUB, lo, hi, seed=SEED_PUB, t0=st['t'])
    assert rep['min_abs_margin'] > 1e-9, rep['min_abs_margin']
    assert np.array_equal(rep['chain'], res['chain']) and np.array_equal(rep['log_prob'], res['log_prob'])
    assert np.array_equal(rep['n_accept'] / float(STEPS_PUB), res['acceptance_fraction'])
    assert rep['n_inside'] == res['stats']['n_inside'] and rep['n_accepted'] == res['stats']['n_accepted']


def test_public_continuation_seeds_and_hand_over(engine0, res6):
    res, _, obs_dict = res6
    first, _, _ = public(n_steps=3)
    assert np.array_equal(first['chain'], res['chain'][:3])                      # the same seed again: the same chain
    second, _, _ = public(n_steps=3, state=first['state'])
    assert np.array_equal(second['chain'], res['chain'][3:]) and np.array_equal(second['log_prob'], res['log_prob'][3:])
    assert np.array_equal(second['proposals'], res['proposals'][3:])
    assert np.array_equal(second['acceptance_fraction'], res['acceptance_fraction'])
    for k in ('theta', 'lp', 'n_accept'):
        assert np.array_equal(second['state'][k], res['state'][k])
    assert second['state']['t'] == res['state']['t'] == STEPS_PUB
    other, _, _ = public(n_steps=2, seed=SEED_PUB + 1)
    assert not np.array_equal(other['chain'], res['chain'][:2])
    # the last positions go straight into the ensemble call that draws the predictive bands
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
    assert sorted(res['overrides']) == ['T_g', 'a_Q', 'fc'] and list(res['error_m']) == ['Q_cumecs']
    assert np.array_equal(res['error_m']['Q_cumecs'], res['state']['theta'][3])
    ens = sp.run_simply_p_ensemble(met, p_struc, p_SU, p_LU, p_SC, p, dyn, overrides=res['overrides'], obs_dict=obs_dict,
                                   quantiles=[0.025, 0.5, 0.975], predictive_series=list(res['error_m']),
                                   predictive_m=res['error_m'], keep_daily=False)
    band = ens['predictive']['overall']['data']
    assert band.shape == (3, 1, 366, 1) and np.isfinite(band).all() and (band[0] <= band[2]).all()
    assert np.array_equal(ens['gof']['data'][abi.GOF_STATS.index('N obs'), 0, 0], np.full(W_PUB, 360.0))


def test_public_start_with_a_non_finite_log_posterior(engine0):
    with pytest.raises(ValueError, match='non-finite log posterior'):
        public(n_steps=1, variables=['Q'], error_m=None,
               priors={'fc': (200.0, 380.0), 'm_Q': (0.0, 1.0)}, n_walkers=4, start=np.array([[290.0] * 4, [0.3, 0.3, 0.0, 0.3]]))


# ---- argument errors of the ABI -----------------------------------------------------------------------------------------

def test_abi_argument_errors(engine0):
    W, n_dim, h = 8, 2, 4
    theta, lo, hi, target = problem(W, n_dim)
    f64 = dict(dtype=torch.float64, device=engine0.tdev)
    th_d = dev(engine0, theta)
    prop, inside = torch.full((n_dim, h), SENTINEL, **f64), torch.full((h,), -5, dtype=torch.int32, device=engine0.tdev)
    mp, ft = torch.full((marshal.NP_M, h), SENTINEL, **f64), torch.full((h,), SENTINEL, **f64)

    def propose(theta_d=th_d, half=0, lo_=lo, hi_=hi, tg=target, prop_=prop, a=2.0, mp_=mp):
        return engine0.mcmc_propose(theta_d, half, 0, lo_, hi_, tg, prop_, inside, mp_, ft, a=a)

    z = lambda *s: torch.zeros(s, **f64)
    nan = float('nan')
    bad = [dict(theta_d=z(1, 3), lo_=lo[:1], hi_=hi[:1], tg=target[:1]), dict(theta_d=z(2, 2)),                                        # odd W; W < 2 n_dim
           dict(theta_d=z(17, 40), lo_=np.zeros(17), hi_=np.ones(17), tg=np.full(17, -2)),      # n_dim past 16
           dict(half=2), dict(half=-1), dict(a=1.0), dict(a=nan),
           dict(lo_=np.array([0.0, 1.0]), hi_=np.array([1.0, 1.0])), dict(lo_=np.array([nan, 0.0])), dict(hi_=np.array([1.0, nan])),
           dict(tg=np.array([2, -3])), dict(tg=np.array([marshal.NP_M, 0])),
           dict(prop_=None), dict(mp_=None)]
    for kw in bad:
        with pytest.raises(engine.EngineError, match=r'simplyp_mcmc_propose failed \(-1\): simplyp_mcmc_propose'):
            propose(**kw)
    assert (prop == SENTINEL).all() and (inside == -5).all() and (mp == SENTINEL).all() and (ft == SENTINEL).all()
    info = propose()                                                                            # a valid call afterwards works
    assert np.array_equal(prop.cpu().numpy(), mcmc.propose(theta, 0, 0, lo, hi)['prop'])
    assert info['n_inside'] == int(inside.sum())

    lp, nacc, lpp = z(W), torch.zeros((W,), dtype=torch.int32, device=engine0.tdev), z(h)
    before = th_d.clone()

    def accept(theta_d=th_d, half=0, a=2.0, lpp_=lpp, nacc_=nacc):
        return engine0.mcmc_accept(theta_d, lp, nacc_, half, 0, prop, inside, lpp_, a=a)

    for kw in (dict(theta_d=z(1, 3)), dict(theta_d=z(3, 4)), dict(theta_d=z(17, 40)), dict(half=2), dict(a=0.5), dict(a=nan),
               dict(lpp_=None), dict(nacc_=None)):
        with pytest.raises(engine.EngineError, match=r'simplyp_mcmc_accept failed \(-1\): simplyp_mcmc_accept'):
            accept(**kw)
    assert torch.equal(th_d, before) and (nacc == 0).all() and (lp == 0).all()
    assert accept()['n_accepted'] == int(nacc.sum())

    gof = z(len(abi.GOF_STATS), 6, 1, h)
    out = torch.full((h,), SENTINEL, **f64)

    def log_prob(pairs=((0, 0),), m_dim=(0, -1, -1, -1, -1, -1), prop_=prop, out_=out):
        return engine0.mcmc_log_prob(gof, list(pairs), list(m_dim), [0.5] * 6, prop_, out_)

    for kw in (dict(pairs=((6, 0),)), dict(pairs=((0, 1),)), dict(pairs=((0, 0),) * 33), dict(m_dim=(2, -1, -1, -1, -1, -1)),
               dict(m_dim=(-2, -1, -1, -1, -1, -1)), dict(out_=None)):
        with pytest.raises(engine.EngineError, match=r'simplyp_mcmc_log_prob failed \(-1\): simplyp_mcmc_log_prob'):
            log_prob(**kw)
    with pytest.raises(engine.EngineError, match=r'simplyp_mcmc_log_prob failed \(-1\): simplyp_mcmc_log_prob'):
        engine0.mcmc_log_prob(z(len(abi.GOF_STATS), 6, 1, 17), [(0, 0)], [-1] * 6, [0.5] * 6, z(17, 17), None)    # n_dim 17 (and W < 2 n_dim)
    assert (out == SENTINEL).all()
    log_prob()
    assert (out != SENTINEL).all()
