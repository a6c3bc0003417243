"""The device's multi-start Nelder-Mead search (simplyp_nm_propose / simplyp_nm_update) against its NumPy statement
(simplyp_amd/neldermead.py), and find_map end to end.

Both sides are + - * / and comparisons in fp64 in the same order (the library is built without contraction): everything is compared
bit for bit, with no margin.  The public call's values against an independent ensemble run at the same points: 1e-12 relative, the
sampler test's bound for the same reason (same kernels, independent members; the goodness-of-fit sums may be chunked differently)."""

import numpy as np
import pytest
import torch

import helpers
import simplyp_amd as sp
from simplyp_amd import abi, engine, marshal, neldermead as nm, visualise_results as vr

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (64, 3), (130, 5), (257, 16)]        # a partial wave, a partial block, a second block; both ends of n_dim
NAME = 'tarland_2004_dynamic'
SENTINEL = -777.25
MAX_ITER = 4


def dev(eng, a, dtype=torch.float64):
    return eng.to_device(np.ascontiguousarray(a), dtype)


def variants(n_dim):
    """(phase, cursor, n_iter) a simplex can be in: stepping, evaluating its initial vertices (cursor 0, 4, ...) or its shrunk ones
    (cursor 1, 5, ...), done."""
    v = [(nm.STEP, 0, 1), (nm.STEP, 0, 2), (nm.STEP, 0, MAX_ITER - 1), (nm.DONE, 0, 3)]
    v += [(nm.EVAL, c, 0) for c in range(0, n_dim + 1, 4)]
    v += [(nm.EVAL, c, 2) for c in range(1, n_dim + 1, 4)] + [(nm.EVAL, c, MAX_ITER - 1) for c in range(1, n_dim + 1, 4)]
    return v


def problem(S, n_dim, shift):
    """Sorted simplexes inside a box their candidates often leave, every variant among the lanes (lane s: variant s + shift), some
    simplexes small enough to pass the termination test; targets that name rows, f_tdp and nothing."""
    rng = np.random.default_rng(1000 * S + n_dim)
    lo = -1.0 - np.arange(n_dim) * 0.125
    hi = 1.5 + np.arange(n_dim) * 0.25
    centre = rng.uniform(0.2, 0.8, (1, n_dim, S))
    sim = lo[None, :, None] + (hi - lo)[None, :, None] * (centre + rng.uniform(-0.12, 0.12, (n_dim + 1, n_dim, S)))
    fsim = np.sort(rng.normal(20.0, 3.0, (n_dim + 1, S)), axis=0)
    tiny = rng.uniform(size=S) < 0.25
    sim[1:, :, tiny] = sim[:1, :, tiny] + rng.uniform(-4e-5, 4e-5, (n_dim, n_dim, int(tiny.sum())))
    fsim[1:, tiny] = fsim[:1, tiny] + np.sort(rng.uniform(0.0, 4e-5, (n_dim, int(tiny.sum()))), axis=0)
    st = nm.new_state(sim)
    st['fsim'] = fsim
    var = variants(n_dim)
    for s in range(S):
        st['phase'][s], st['cursor'][s], st['n_iter'][s] = var[(s + shift) % len(var)]
    st['status'][st['phase'] == nm.DONE] = nm.CONVERGED
    st['counts'][:] = rng.integers(0, 5, st['counts'].shape)
    target = np.array([2, abi.MCMC_TARGET_F_TDP, abi.MCMC_TARGET_NONE] + list(range(5, 5 + n_dim)), dtype=np.int32)[:n_dim]
    return st, lo, hi, target


def caller_lp(rng, st, n_dim, S):
    """ln p of the run points as a caller might hand them over.  The reflection's value falls below the best vertex, among the
    vertices, between the two worst or beyond the worst, a quarter of the simplexes each, and the other three values anywhere
    across and beyond the simplex's own range: every branch of the decision tree is taken.  -inf and NaN are among them."""
    fb, fn1, fw = st['fsim'][0], st['fsim'][-2], st['fsim'][-1]
    span = fw - fb
    f = rng.uniform(fb - 0.5 * span, fw + 0.5 * span, (4, S))
    edges = np.stack([fb - 0.5 * span, fb, fn1, fw, fw + 0.5 * span])
    k = rng.integers(0, 4, S)
    f[0] = rng.uniform(edges[k, np.arange(S)], edges[k + 1, np.arange(S)])
    f[1] = np.where(rng.uniform(size=S) < 0.5, f[0] - 0.1 * span, f[1])          # an expansion that pays, half of the time
    f[:, rng.uniform(size=S) < 0.15] += 2.0 * span.max()         # nothing helps: a shrink
    lp = -f.reshape(-1)
    if S >= 8:
        lp[rng.choice(4 * S, S // 2, replace=False)] = -np.inf
        lp[rng.choice(4 * S, S // 2, replace=False)] = np.nan
    return lp


@pytest.mark.parametrize('S,n_dim', SHAPES)
def test_propose_and_update_match_the_mirror_bit_for_bit(engine0, S, n_dim):
    E = 4 * S
    n_var = len(variants(n_dim))
    seen = dict(outside=0, moves=np.zeros(5, dtype=np.int64), status=set(), eval_done=0)
    rng = np.random.default_rng(S + 17)
    for shift in range(n_var if S < n_var else 3):               # few lanes: every variant gets its turn
        st, lo, hi, target = problem(S, n_dim, shift)
        want = nm.propose(st, lo, hi)
        sim_d, fsim_d, ist_d = dev(engine0, st['sim']), dev(engine0, st['fsim']), dev(engine0, nm.pack_istate(st), torch.int32)
        prop = torch.full((n_dim, E), SENTINEL, dtype=torch.float64, device=engine0.tdev)
        inside = torch.full((E,), -5, dtype=torch.int32, device=engine0.tdev)
        mp = torch.full((marshal.NP_M, E), SENTINEL, dtype=torch.float64, device=engine0.tdev)
        ft = torch.full((E,), SENTINEL, dtype=torch.float64, device=engine0.tdev)
        info = engine0.nm_propose(sim_d, ist_d, lo, hi, target, prop, inside, mp, ft)
        assert np.array_equal(prop.cpu().numpy(), want['prop'])
        assert np.array_equal(inside.cpu().numpy(), want['inside'].astype(np.int32))
        c = nm.counters(st)
        assert info['n_inside'] == int(want['inside'].sum())
        assert {k: info[k] for k in c} == c
        got_mp, got_ft = mp.cpu().numpy(), ft.cpu().numpy()
        named = set()
        for d in range(n_dim):
            if target[d] >= 0:
                assert np.array_equal(got_mp[target[d]], want['run_point'][d]), d
                named.add(int(target[d]))
            elif target[d] == abi.MCMC_TARGET_F_TDP:
                assert np.array_equal(got_ft, want['run_point'][d])
        rest = [r for r in range(marshal.NP_M) if r not in named]
        assert (got_mp[rest] == SENTINEL).all()                    # rows that no dimension names are not touched
        if n_dim < 2:
            assert (got_ft == SENTINEL).all()
        # the run point: the slot's point where it wants a value inside the box, the first vertex everywhere else
        first = np.tile(st['sim'][0], (1, 4))
        assert np.array_equal(want['run_point'], np.where(want['inside'], want['prop'], first))
        assert ((want['run_point'] >= lo[:, None]) & (want['run_point'] < hi[:, None])).all()
        seen['outside'] += int((want['used'] & ~want['inside']).sum())
        assert np.array_equal(sim_d.cpu().numpy(), st['sim']) and np.array_equal(ist_d.cpu().numpy(), nm.pack_istate(st))

        # ---- the update, on the caller's ln p
        lp = caller_lp(rng, st, n_dim, S)
        mirror = nm.copy_state(st)
        hist = np.full((MAX_ITER + 1, S), SENTINEL)
        winfo = nm.update(mirror, want['prop'], want['inside'], lp, MAX_ITER, 1e-4, 1e-4, history=hist)
        hist_d = torch.full((MAX_ITER + 1, S), SENTINEL, dtype=torch.float64, device=engine0.tdev)
        info = engine0.nm_update(sim_d, fsim_d, ist_d, prop, inside, dev(engine0, lp), MAX_ITER, 1e-4, 1e-4, history=hist_d)
        assert np.array_equal(sim_d.cpu().numpy(), mirror['sim']) and np.array_equal(fsim_d.cpu().numpy(), mirror['fsim'])
        assert np.array_equal(ist_d.cpu().numpy(), nm.pack_istate(mirror))
        assert np.array_equal(hist_d.cpu().numpy(), hist)
        assert {k: info[k] for k in winfo} == winfo and info['n_inside'] == 0
        assert (mirror['fsim'][:-1, mirror['phase'] != nm.EVAL] <= mirror['fsim'][1:, mirror['phase'] != nm.EVAL]).all()
        seen['moves'] += (mirror['counts'] - st['counts']).sum(axis=1)
        seen['status'] |= set(mirror['status'][(st['phase'] != nm.DONE) & (mirror['phase'] == nm.DONE)].tolist())
        seen['eval_done'] += int(((st['phase'] == nm.EVAL) & (mirror['phase'] == nm.STEP)).sum())
        # without a history nothing else changes
        sim2, fsim2, ist2 = dev(engine0, st['sim']), dev(engine0, st['fsim']), dev(engine0, nm.pack_istate(st), torch.int32)
        engine0.nm_update(sim2, fsim2, ist2, prop, inside, dev(engine0, lp), MAX_ITER)
        assert torch.equal(sim2, sim_d) and torch.equal(fsim2, fsim_d) and torch.equal(ist2, ist_d)
    if S >= 64:
        assert seen['outside'] > 0 and (seen['moves'] > 0).all() and seen['eval_done'] > 0, seen
        assert seen['status'] == {nm.CONVERGED, nm.MAXITER, nm.NONFINITE_START}


def total(a):
    acc = a[0]
    for row in a[1:]:
        acc = acc + row
    return acc


def rosen(x):
    return total(100.0 * (x[1:] - x[:-1] ** 2) ** 2 + (1.0 - x[:-1]) ** 2)


def rough(x):
    return np.abs(x - 0.3).max(axis=0) * (1.5 + np.sin(40.0 * total(x))) + 0.05 * total(np.round(7.0 * x)) ** 2


@pytest.mark.parametrize('f,n_dim,S,max_iter', [(rough, 5, 130, 130), (rosen, 3, 70, 150)], ids=['rough', 'rosenbrock'])
def test_a_whole_optimisation_through_the_abi(engine0, f, n_dim, S, max_iter):
    """f is the caller's own: evaluated on the host at the downloaded run points."""
    lo, hi = -np.ones(n_dim), np.ones(n_dim)
    x0 = nm.uniform_starts(3, n_dim, S, 0.9 * lo, 0.9 * hi)
    if f is rough:
        x0[:, 0] = (0.9, -0.6, 0.5, 0.4, -0.3)
    want = nm.run(f, x0, lo, hi, max_iter=max_iter)
    assert {nm.CONVERGED, nm.MAXITER} == set(want['status'].tolist())           # one simplex of each final status at least
    if f is rough:
        assert want['counts']['shrink'].sum() >= 1 and want['counts']['shrink'][0] == 5
    st = nm.new_state(nm.initial_simplex(x0, lo, hi))
    sim_d, fsim_d, ist_d = dev(engine0, st['sim']), dev(engine0, st['fsim']), dev(engine0, nm.pack_istate(st), torch.int32)
    hist_d = torch.full((max_iter, S), float('nan'), dtype=torch.float64, device=engine0.tdev)
    prop = torch.empty((n_dim, 4 * S), dtype=torch.float64, device=engine0.tdev)
    inside = torch.empty((4 * S,), dtype=torch.int32, device=engine0.tdev)
    mp = torch.zeros((marshal.NP_M, 4 * S), dtype=torch.float64, device=engine0.tdev)
    target = np.arange(n_dim, dtype=np.int32)                    # the run points go to rows 0 .. n_dim - 1
    n_active, n_runs = S, 0
    while n_active and n_runs < want['n_runs'] + 1:
        pinfo = engine0.nm_propose(sim_d, ist_d, lo, hi, target, prop, inside, mp)
        assert pinfo['n_active'] == n_active
        points = mp[:n_dim].cpu().numpy()
        assert ((points >= lo[:, None]) & (points < hi[:, None])).all()
        n_active = engine0.nm_update(sim_d, fsim_d, ist_d, prop, inside, dev(engine0, -f(points)), max_iter, history=hist_d)['n_active']
        n_runs += 1
    assert n_active == 0 and n_runs == want['n_runs']
    assert np.array_equal(sim_d.cpu().numpy(), want['sim']) and np.array_equal(fsim_d.cpu().numpy(), want['fsim'])
    assert np.array_equal(ist_d.cpu().numpy(), nm.pack_istate(want['state']))
    assert np.array_equal(hist_d.cpu().numpy(), want['history'], equal_nan=True)


# ---- the public call ----------------------------------------------------------------------------------------------------

S_PUB, ITER_PUB, SEED_PUB = 16, 9, 11                   # max_iter 9: the initial simplex and 8 iterations


def public(**kw):
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
    obs_dict = helpers.observations(p_SU['st_dt'], p_SU['end_dt'])
    priors = {nm_: (0.7 * float(p[nm_]), 1.3 * float(p[nm_])) for nm_ in ('fc', 'T_g', 'a_Q')}
    priors['m_Q'] = (0.01, 1.0)
    args = dict(priors=priors, variables=['Q'], n_starts=S_PUB, max_iter=ITER_PUB, seed=SEED_PUB, record_evaluations=True)
    args.update(kw)
    return sp.find_map(met, p_struc, p_SU, p_LU, p_SC, p, dyn, obs_dict, **args), priors, obs_dict


@pytest.fixture(scope='module')
def res8(engine0):
    return public()


def test_public_values_equal_an_independent_ensemble_run(engine0, res8):
    res, priors, obs_dict = res8
    assert res['names'] == ['fc', 'T_g', 'a_Q', 'm_Q']
    assert res['x'].shape == (4, S_PUB) and res['fun'].shape == (S_PUB,) and res['history'].shape == (ITER_PUB, S_PUB)
    assert (res['n_iter'] == ITER_PUB).all() and (res['status'] == nm.MAXITER).all()
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
    ens = sp.run_simply_p_ensemble(met, p_struc, p_SU, p_LU, p_SC, p, dyn, overrides={n: res['x'][d] for d, n in enumerate(res['names'][:3])},
                                   obs_dict=obs_dict, keep_daily=False)
    assert int(ens['status'].max()) == 0
    want = -vr.loglik(ens['gof']['data'], res['x'][3])[abi.GOF_VARS.index('Q'), 0]
    assert np.isfinite(res['fun']).all()
    assert (np.abs(res['fun'] - want) <= 1e-12 * np.abs(want)).all(), np.abs(res['fun'] / want - 1).max()
    # the best value never rises, every vertex is inside its box, the best point is reported three ways
    assert (np.diff(res['history'], axis=0) <= 0).all() and np.array_equal(res['history'][-1], res['fun'])
    sim, fsim = res['final_simplex']
    for d, n in enumerate(res['names']):
        assert (sim[:, d] >= priors[n][0]).all() and (sim[:, d] < priors[n][1]).all()
    assert np.array_equal(sim[0], res['x']) and np.array_equal(fsim[0], res['fun']) and (fsim[:-1] <= fsim[1:]).all()
    b = res['best']
    assert res['fun'][b] == res['fun'].min() and res['map'] == {n: res['x'][d, b] for d, n in enumerate(res['names'])}
    assert sorted(res['overrides']) == ['T_g', 'a_Q', 'fc'] and list(res['error_m']) == ['Q_cumecs']
    assert res['overrides']['fc'].shape == (1,) and res['error_m']['Q_cumecs'][0] == res['x'][3, b]
    n_runs = len(res['stats']['wall_ms'])
    assert res['evaluations'].shape == (n_runs, 4, 4 * S_PUB) and min(res['stats']['run_kernel_ms']) > 0.0
    assert res['stats']['n_active'][0] == S_PUB and sum(int(v.sum()) for v in res['moves'].values()) == S_PUB * (ITER_PUB - 1)
    # simplex 0 started at the workbook's values, the others at the documented uniforms
    x0 = res['start']['sim'][0]
    lo = np.array([priors[n][0] for n in res['names']]); hi = np.array([priors[n][1] for n in res['names']])
    assert np.array_equal(x0[:3, 0], [float(p[n]) for n in res['names'][:3]]) and x0[3, 0] == 0.5 * (0.01 + 1.0)
    assert np.array_equal(x0[:, 1:], nm.uniform_starts(SEED_PUB, 4, S_PUB, lo, hi)[:, 1:])
    # the best point goes straight into the ensemble call
    one = sp.run_simply_p_ensemble(met, p_struc, p_SU, p_LU, p_SC, p, dyn, overrides=res['overrides'], obs_dict=obs_dict, keep_daily=False)
    lp = vr.loglik(one['gof']['data'], res['error_m']['Q_cumecs'])[abi.GOF_VARS.index('Q'), 0]
    assert abs(-lp[0] - res['fun'][b]) <= 1e-12 * abs(res['fun'][b])


def test_public_path_is_the_mirrors_replay_of_the_recorded_values(engine0, res8):
    res, priors, _ = res8
    lo = np.array([priors[n][0] for n in res['names']]); hi = np.array([priors[n][1] for n in res['names']])
    runs = iter(range(len(res['evaluations'])))

    def recorded(points):
        k = next(runs)
        lp = res['evaluation_log_prob'][k]
        ran = np.isfinite(lp)                                      # where the model ran at the slot's point, it is the recorded one
        assert np.array_equal(points[:, ran], res['evaluations'][k][:, ran])
        return -lp

    rep = nm.run(recorded, None, lo, hi, max_iter=ITER_PUB, state=res['start'])
    assert rep['n_runs'] == len(res['evaluations'])
    assert np.array_equal(rep['sim'], res['final_simplex'][0]) and np.array_equal(rep['fsim'], res['final_simplex'][1])
    assert np.array_equal(rep['n_iter'], res['n_iter']) and np.array_equal(rep['status'], res['status'])
    assert np.array_equal(rep['history'], res['history'], equal_nan=True)
    for m in nm.MOVES:
        assert np.array_equal(rep['counts'][m], res['moves'][m])


def test_public_continuation_and_hand_over_to_the_sampler(engine0, res8):
    res, priors, obs_dict = res8
    first, _, _ = public(max_iter=5)
    assert (first['n_iter'] == 5).all() and np.array_equal(first['history'], res['history'][:5])
    second, _, _ = public(state=first['state'])
    for k in ('x', 'fun', 'n_iter', 'status', 'history'):
        assert np.array_equal(second[k], res[k]), k
    assert np.array_equal(second['final_simplex'][0], res['final_simplex'][0])
    assert np.array_equal(second['final_simplex'][1], res['final_simplex'][1])
    assert np.array_equal(np.concatenate([first['evaluations'], second['evaluations']]), res['evaluations'])
    for k in res['state']:
        assert np.array_equal(second['state'][k], res['state'][k], equal_nan=(k == 'history')), k
    # the best point, as a ball, starts a chain
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
    start = sp.start_ball(res['x'][:, res['best']], priors, 8, seed=3)
    chain = sp.sample_posterior(met, p_struc, p_SU, p_LU, p_SC, p, dyn, obs_dict, priors, variables=['Q'], n_walkers=8, n_steps=1,
                                start=start, seed=3)
    assert np.array_equal(chain['start']['theta'], start) and np.isfinite(chain['log_prob']).all()


def test_public_errors(engine0):
    with pytest.raises(ValueError, match='start of simplex 2 has a vertex with a non-finite log posterior'):
        public(priors={'fc': (200.0, 380.0), 'm_Q': (0.0, 1.0)}, n_starts=4, init_guess=np.array([[290.0] * 4, [0.3, 0.3, 0.0, 0.3]]))
    with pytest.raises(ValueError, match=r'init_guess must have shape \[n_dim, n_starts\]'):
        public(init_guess=np.zeros((4, 3)))
    with pytest.raises(ValueError, match='initial guess of simplex 1 lies outside the box'):
        public(priors={'fc': (200.0, 380.0), 'm_Q': (0.01, 1.0)}, n_starts=2, init_guess=np.array([[290.0, 380.0], [0.3, 0.3]]))
    with pytest.raises(ValueError, match='4 n_starts >= n_dim'):
        public(n_starts=0)
    with pytest.raises(ValueError, match="out_slot_order'\\] must stay 0"):
        public(solver=dict(out_slot_order=1))
    with pytest.raises(ValueError, match='needs obs_dict'):
        met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
        sp.find_map(met, p_struc, p_SU, p_LU, p_SC, p, dyn, None, {'fc': (200.0, 380.0)}, error_m={'Q': 0.3})


# ---- argument errors of the ABI -----------------------------------------------------------------------------------------

def test_abi_argument_errors(engine0):
    S, n_dim = 6, 2
    st, lo, hi, target = problem(S, n_dim, 0)
    f64 = dict(dtype=torch.float64, device=engine0.tdev)
    i32 = dict(dtype=torch.int32, device=engine0.tdev)
    sim_d, fsim_d, ist_d = dev(engine0, st['sim']), dev(engine0, st['fsim']), dev(engine0, nm.pack_istate(st), torch.int32)
    prop, inside = torch.full((n_dim, 4 * S), SENTINEL, **f64), torch.full((4 * S,), -5, **i32)
    mp, ft = torch.full((marshal.NP_M, 4 * S), SENTINEL, **f64), torch.full((4 * S,), SENTINEL, **f64)

    def propose(sim_=sim_d, ist_=ist_d, lo_=lo, hi_=hi, tg=target, prop_=prop, mp_=mp, ft_=ft):
        return engine0.nm_propose(sim_, ist_, lo_, hi_, tg, prop_, inside, mp_, ft_)

    z = lambda *s: torch.zeros(s, **f64)
    nan = float('nan')
    bad = [dict(sim_=z(18, 17, 4), lo_=np.zeros(17), hi_=np.ones(17), tg=np.full(17, -2)),                  # n_dim past 16
           dict(sim_=z(3, 2, 0)),                                                                            # S = 0
           dict(lo_=np.array([0.0, 1.0]), hi_=np.array([1.0, 1.0])), dict(lo_=np.array([nan, 0.0])), dict(hi_=np.array([1.0, nan])),
           dict(tg=np.array([2, -3])), dict(tg=np.array([marshal.NP_M, 0])), dict(tg=np.array([4, 4])),
           dict(prop_=None), dict(ist_=None), dict(mp_=None), dict(ft_=None)]
    for kw in bad:
        with pytest.raises(engine.EngineError, match=r'simplyp_nm_propose failed \(-1\): simplyp_nm_propose'):
            propose(**kw)
    assert (prop == SENTINEL).all() and (inside == -5).all() and (mp == SENTINEL).all() and (ft == SENTINEL).all()
    info = propose()                                                                                         # a valid call afterwards works
    assert np.array_equal(prop.cpu().numpy(), nm.propose(st, lo, hi)['prop']) and info['n_inside'] == int(inside.sum())

    lp = z(4 * S)
    before = (sim_d.clone(), fsim_d.clone(), ist_d.clone())

    def update(sim_=sim_d, fsim_=fsim_d, ist_=ist_d, lp_=lp, max_iter=5, xatol=1e-4, fatol=1e-4, hist=None):
        return engine0.nm_update(sim_, fsim_, ist_, prop, inside, lp_, max_iter, xatol, fatol, history=hist)

    for kw in (dict(sim_=z(18, 17, 4)), dict(sim_=z(3, 2, 0)), dict(max_iter=0), dict(xatol=-1.0), dict(fatol=nan), dict(xatol=nan),
               dict(lp_=None), dict(fsim_=None), dict(ist_=None)):
        with pytest.raises(engine.EngineError, match=r'simplyp_nm_update failed \(-1\): simplyp_nm_update'):
            update(**kw)
    with pytest.raises(ValueError, match='sim must be'):
        update(sim_=z(2, 2, 4))
    assert torch.equal(sim_d, before[0]) and torch.equal(fsim_d, before[1]) and torch.equal(ist_d, before[2])
    mirror = nm.copy_state(st)
    want = nm.update(mirror, prop.cpu().numpy(), inside.cpu().numpy(), np.zeros(4 * S), 5)
    got = update()
    assert {k: got[k] for k in want} == want and np.array_equal(sim_d.cpu().numpy(), mirror['sim'])
