"""Forcing uncertainty on the device: the generated table against its NumPy statement (simplyp_amd/forcing.py), the run that
reads it against the run handed the same table explicitly, the invariances a counter-based draw promises, the CPU oracle on the
mirror's table, the refusals, and the particle filter with input noise.

E = 70 (no multiple of 64), Tarland 2004 (D = 366: across the 256-day forcing tile), 2 forcing rows and 3 (snow module)."""

import numpy as np
import pytest

import helpers
import simplyp_amd as sp
from simplyp_amd import engine, forcing, marshal

pytestmark = pytest.mark.gpu

NAME = 'tarland_2004_dynamic'
E, D, SEED = 70, 366, 20041
SIGMA = (0.3, 0.1, 0.5)
# the stream's integers are exact, so z differs from the mirror's by the roundings of log, sqrt and cospi only: 2^-45
# (tests/test_gpu_predictive.py).  T_air' = (T + offset) + sigma z: sigma 2^-45 absolute.
# P', PET' = v * exp(sigma z - sigma^2 / 2): the argument (|.| <= 19.2) is off by sigma 2^-45 <= 2^-44 and by its two roundings
# (<= 2^-47); sp_exp adds its own ~1 ulp (tests/test_gpu_elementary.py): 2^-43 relative covers them.
Z_TOL, REL_TOL = 2.0 ** -45, 2.0 ** -43


def problem(name=NAME, snow=False, n=E, solver=None, mask=marshal.MASK_REACH5):
    m = helpers.marshal_scenario(name, E=n, out_mask=mask, solver=solver, snow=snow)
    m['member_params'][marshal.PM_NAMES.index('fc')] *= np.random.default_rng(7).uniform(0.9, 1.1, n)
    return m


def spec(snow, groups='day', shift=True, sigma=SIGMA):
    rng = np.random.default_rng(3)
    s = {'P': {'sigma': sigma[0], 'groups': groups}, 'PET': {'sigma': sigma[1], 'groups': groups}}
    if shift:
        s['P']['scale'], s['PET']['scale'] = rng.uniform(0.8, 1.2, E), 1.05
    if snow:
        s['T_air'] = {'sigma': sigma[2], 'groups': groups}
        if shift:
            s['T_air']['offset'] = rng.uniform(-1.0, 3.0, E)
    return s


def run(eng, m, **kw):
    rhs = eng.torch.zeros((m['member_params'].shape[1],), dtype=eng.torch.int32, device=eng.tdev)
    out, status, stats = eng.run(m['forcing'], m['doy'], m['member_params'], m['reach_params'], m['up_ptr'], m['up_idx'], m['opts'],
                                 member_rhs=rhs, **kw)
    return out.cpu().numpy(), status.cpu().numpy(), rhs.cpu().numpy(), stats


def same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the table against the mirror ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('snow', [False, True], ids=['rows2', 'rows3'])
@pytest.mark.parametrize('groups', ['day', 'month_array', 'one_group'])
def test_table_matches_the_mirror(engine0, snow, groups):
    """sigma = (0.3, 0.1, 0.5), scales and offset given.  T_air within sigma_T 2^-45 absolute, P and PET within 2^-43 relative (the
    derivation stands above); dry days exact.  Measured worst cases on MI355X, far inside the derived bounds, which stay: P and
    PET 4.2e-16 relative (bound 1.1e-13), T_air 3.6e-15 absolute (bound 1.4e-14)."""
    m = problem(snow=snow)
    index = m['met'].index
    g = {'day': 'day', 'month_array': np.asarray(index.year * 12 + index.month - 1), 'one_group': np.full(D, 5)}[groups]
    fe = forcing.resolve(spec(snow, g), index, E, snow, SEED)
    _, status, _, stats = run(engine0, m, forcing_error=fe, keep_forcing_table=True)
    got, want = stats['forcing_table'].cpu().numpy(), forcing.table(m['forcing'], fe, E=E)
    assert got.shape == want.shape == (E, 3 if snow else 2, D) and status.max() == 0
    dry = m['forcing'][0, 0] == 0
    assert dry.any() and (got[:, 0, dry] == 0).all() and (got[:, 0, ~dry] > 0).all()
    for r in (0, 1):
        err = helpers.max_rel_err(got[:, r], want[:, r], floor=1e-300)
        print('row %d max rel err %.3e (bound %.3e)' % (r, err, REL_TOL))
        assert err <= REL_TOL, (r, err)
    if snow:
        err = np.abs(got[:, 2] - want[:, 2]).max()
        print('T_air max abs err %.3e (bound %.3e)' % (err, SIGMA[2] * Z_TOL))
        assert err <= SIGMA[2] * Z_TOL, err
    if groups == 'one_group':            # one multiplier per member: the ratio to the scaled base is constant over the wet days
        ratio = got[:, 0, ~dry] / (m['forcing'][0, 0, ~dry][None, :] * fe['shift'][0][:, None])
        assert (np.abs(ratio / ratio[:, :1] - 1.0) < 4e-16).all() and len(np.unique(ratio[:, 0])) == E


@pytest.mark.parametrize('snow', [False, True], ids=['rows2', 'rows3'])
def test_rows_without_sigma_are_exact(engine0, snow):
    """sigma = 0: base * scale (base + offset) alone, bit for bit; no shift either: the base itself."""
    m = problem(snow=snow)
    fe = forcing.resolve(spec(snow, sigma=(0.3, 0.0, 0.0)), m['met'].index, E, snow, SEED)
    _, _, _, stats = run(engine0, m, forcing_error=fe, keep_forcing_table=True)
    got, want = stats['forcing_table'].cpu().numpy(), forcing.table(m['forcing'], fe, E=E)
    assert same(np.ascontiguousarray(got[:, 1:]), np.ascontiguousarray(want[:, 1:]))
    fe = forcing.resolve(spec(snow, shift=False, sigma=(0.3, 0.0, 0.0)), m['met'].index, E, snow, SEED)
    _, _, _, stats = run(engine0, m, forcing_error=fe, keep_forcing_table=True)
    got = stats['forcing_table'].cpu().numpy()
    assert all(same(np.ascontiguousarray(got[e, 1:]), np.ascontiguousarray(m['forcing'][0, 1:])) for e in range(E))


# ---- the run reads exactly that table --------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', [NAME, 'chain4_val_2004'])
@pytest.mark.parametrize('balance', [0, 1])
@pytest.mark.parametrize('lanes', [1, 4])
def test_run_uses_exactly_the_generated_table(engine0, name, balance, lanes):
    m = problem(name, solver=dict(balance=balance, lanes_per_member=lanes))
    fe = forcing.resolve(spec(False), m['met'].index, E, False, SEED)
    out, status, rhs, stats = run(engine0, m, forcing_error=fe, keep_forcing_table=True)
    assert stats['balanced'] == balance and stats['lanes_per_member'] == lanes and stats['queued'] == (name != NAME)
    m2 = dict(m, forcing=stats['forcing_table'])
    out2, status2, rhs2, stats2 = run(engine0, m2, forcing_of_member=np.arange(E, dtype=np.int32))
    assert stats2['balanced'] == balance and stats2['queued'] == stats['queued']
    assert same(out, out2) and same(status, status2) and same(rhs, rhs2) and status.max() == 0 and rhs.min() > 0
    plain, _, _, _ = run(engine0, m)
    assert not same(out, plain)


# ---- invariances -----------------------------------------------------------------------------------------------------------

def public(fe='default', snow=True, **kw):
    inputs = helpers.scenario_inputs(NAME)
    fc = float(inputs[5]['fc']) * np.random.default_rng(7).uniform(0.9, 1.1, E)
    if fe == 'default':
        fe = spec(snow)
    return inputs, dict(overrides={'fc': fc}, forcing_error=fe, forcing_seed=SEED, snow_in_kernel=snow, **kw)


@pytest.fixture(scope='module')
def whole():
    inputs, kw = public()
    return sp.run_simply_p_ensemble(*inputs, **kw)


def test_windows_laid_end_to_end_are_the_one_call(whole):
    inputs, kw = public()
    index = inputs[0].index
    parts = list(sp.run_simply_p_ensemble_windows(*inputs, window=[index[0], index[100], index[257]], **kw))
    assert [p['window'][2:] for p in parts] == [(0, 100), (100, 257), (257, D)]
    assert same(np.concatenate([p['data'] for p in parts], axis=1), whole['data']) and int(whole['status'].max()) == 0


def test_two_device_blocks_are_the_one_call(whole):
    inputs, kw = public(devices=[0, 0])
    res = sp.run_simply_p_ensemble(*inputs, **kw)
    assert res['stats']['bounds'] == [[0, 35], [35, 70]] and same(res['data'], whole['data'])


def test_a_member_block_draws_what_the_whole_ensemble_draws(engine0):
    m = problem(snow=True)
    fe = forcing.resolve(spec(True), m['met'].index, E, True, SEED)
    out, _, rhs, stats = run(engine0, m, forcing_error=fe, keep_forcing_table=True)
    blk = dict(m, member_params=np.ascontiguousarray(m['member_params'][:, 13:]), reach_params=np.ascontiguousarray(m['reach_params'][:, :, 13:]))
    out_b, _, rhs_b, stats_b = run(engine0, blk, forcing_error=forcing.member_block(fe, 13, E), keep_forcing_table=True)
    assert same(stats_b['forcing_table'].cpu().numpy(), np.ascontiguousarray(stats['forcing_table'].cpu().numpy()[13:]))
    assert same(out_b, np.ascontiguousarray(out[..., 13:])) and same(rhs_b, rhs[13:])


def test_no_sigma_and_no_shift_is_the_call_without_forcing_error():
    inputs, kw = public(fe={'P': {'sigma': 0.0}, 'PET': {'groups': 'month'}, 'T_air': {}})
    got = sp.run_simply_p_ensemble(*inputs, **kw)
    inputs, kw = public(fe=None)
    want = sp.run_simply_p_ensemble(*inputs, **kw)
    assert same(got['data'], want['data']) and same(got['status'], want['status'])


# ---- against the oracle ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('solver,tol', [(dict(integrator='rk4', substeps=32), 1e-10), (None, helpers.TOL_WORKING)])
def test_kernel_on_the_generated_table_matches_the_oracle_on_the_mirrors(engine0, oracle_lib, solver, tol):
    """The CPU oracle given the mirror's table as 8 forcing sets, at test_kernel_matches_oracle's tolerance for the solver."""
    n = 8
    m = problem(snow=True, n=n, solver=solver, mask=marshal.MASK_ALL)
    s = spec(True)
    s['P']['scale'], s['T_air']['offset'] = s['P']['scale'][:n], s['T_air']['offset'][:n]
    fe = forcing.resolve(s, m['met'].index, n, True, SEED)
    got, status, _, stats = run(engine0, m, forcing_error=fe)
    ref, rstatus, rstats = oracle_lib.run(forcing.table(m['forcing'], fe, E=n), m['doy'], m['member_params'], m['reach_params'],
                                          m['up_ptr'], m['up_idx'], m['opts'], forcing_of_member=np.arange(n, dtype=np.int32))
    assert status.max() == 0 and rstatus.max() == 0
    for ci, c in enumerate(marshal.OUT_COLUMNS):
        err = helpers.max_rel_err(got[ci], ref[ci], floor=1e-12)
        assert err < tol, (c, err)
    assert abs(stats['rhs_evals'] - rstats['rhs_evals']) <= 0.005 * rstats['rhs_evals']


# ---- refusals --------------------------------------------------------------------------------------------------------------

def _edit(o, **kw):
    for k, v in kw.items():
        if k.startswith('sigma'):
            o.forcing_sigma[int(k[-1])] = v
        elif k == 'no_group':
            o.forcing_group_of_day[v] = None
        else:
            setattr(o, k, v)


@pytest.mark.parametrize('snow,edit,match', [
    (False, dict(forcing_table=None), 'forcing_error needs forcing_table'),
    (False, dict(sigma0=-0.1), r'forcing_sigma\[0\] \(P\) must be finite and in \[0, 2\]'),
    (False, dict(sigma1=2.5), r'forcing_sigma\[1\] \(PET\) must be finite and in \[0, 2\]'),
    (True, dict(sigma2=float('nan')), r'forcing_sigma\[2\] \(T_air\) must be finite and in \[0, 2\]'),
    (False, dict(sigma0=float('inf')), r'forcing_sigma\[0\] \(P\) must be finite and in \[0, 2\]'),
    (False, dict(sigma2=0.5), r'forcing_sigma\[2\] > 0 perturbs T_air'),
    (False, dict(forcing_shift_rows=3), 'a T_air offset'),
    (False, dict(no_group=0), r'needs forcing_group_of_day\[0\]'),
    (True, dict(no_group=2), r'needs forcing_group_of_day\[2\]')])
def test_refusals_launch_nothing(engine0, snow, edit, match):
    m = problem(snow=snow)
    fe = forcing.resolve(spec(snow), m['met'].index, E, snow, SEED)
    o, keep = engine0._forcing_opts(m['opts'], fe, E, D, 3 if snow else 2)
    if 'sigma2' in edit and not snow:            # a group array is there: only the missing snow module can refuse it
        keep.append(engine0.to_device(fe['groups'][0], engine0.torch.int32))
        o.forcing_group_of_day[2] = keep[-1].data_ptr()
    keep[0].fill_(-777.0)
    _edit(o, **edit)
    out = engine0.torch.full((5, D, 1, E), -777.0, dtype=engine0.torch.float64, device=engine0.tdev)
    with pytest.raises(engine.EngineError, match=match):
        engine0.run(m['forcing'], m['doy'], m['member_params'], m['reach_params'], m['up_ptr'], m['up_idx'], o, out=out)
    engine0.torch.cuda.synchronize()
    assert bool((keep[0] == -777.0).all()) and bool((out == -777.0).all())


def test_a_table_that_does_not_fit_is_refused_with_its_size(engine0, monkeypatch):
    cuda = engine0.torch.cuda
    monkeypatch.setattr(cuda, 'mem_get_info', lambda *a, **k: (1 << 10, 1 << 38))
    monkeypatch.setattr(cuda, 'memory_reserved', lambda *a, **k: 0)
    monkeypatch.setattr(cuda, 'memory_allocated', lambda *a, **k: 0)
    m = problem()
    fe = forcing.resolve(spec(False), m['met'].index, E, False, SEED)
    with pytest.raises(ValueError, match=r'takes %d bytes' % (E * 2 * D * 8)):
        run(engine0, m, forcing_error=fe)


# ---- the particle filter ---------------------------------------------------------------------------------------------------

N_DAYS, WINDOW = 60, 30


def filt(days=slice(0, N_DAYS), **kw):
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
    obs_dict = helpers.observations(p_SU['st_dt'], p_SU['end_dt'])
    priors = {nm: (0.7 * float(p[nm]), 1.3 * float(p[nm])) for nm in ('fc', 'T_g', 'a_Q')}
    priors['m_Q'] = (0.01, 1.0)
    args = dict(priors=priors, variables=['Q'], n_particles=E, window=WINDOW, seed=SEED, record=True)
    args.update(kw)
    return sp.assimilate(met.iloc[days], p_struc, p_SU, p_LU, p_SC, p, dyn, obs_dict, **args)


def same_filter(a, b):
    return all(same(np.asarray(a[k]), np.asarray(b[k])) for k in ('theta', 'log_weights', 'ess', 'log_evidence')) and \
        same(a['state']['data'], b['state']['data'])


def test_assimilate_without_sigma_is_todays_filter():
    assert same_filter(filt(forcing_error={'P': {'sigma': 0.0}, 'PET': {'sigma': 0.0}}), filt())


@pytest.fixture(scope='module')
def noisy():
    return filt(forcing_error={'P': {'sigma': 0.3}})


def test_assimilate_windows_run_on_the_table_of_seed_particle_and_calendar_day(noisy):
    met = helpers.scenario_inputs(NAME)[0]
    base = marshal.forcing_arrays(met)[0]
    assert len(noisy['windows']) == 2 and noisy['resampled'].any()
    for w, (_, _, lo, hi) in enumerate(noisy['windows']):
        fe = forcing.resolve({'P': {'sigma': 0.3}}, met.index[lo:hi], E, False, SEED)
        want = forcing.table(base[:, :, lo:hi], fe, E=E)
        got = noisy['forcing_table'][w]
        assert helpers.max_rel_err(got[:, 0], want[:, 0], floor=1e-300) <= REL_TOL and same(got[:, 1], np.ascontiguousarray(want[:, 1]))
        # the window's run: an explicit ensemble call with the particles' parameters, their state, and the same draws
        met_w, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
        th = noisy['theta_before'][w]
        ens = sp.run_simply_p_ensemble(met_w.iloc[lo:hi], p_struc, p_SU, p_LU, p_SC, p, dyn,
                                       overrides={nm: th[d] for d, nm in enumerate(noisy['names'][:3])}, outputs=marshal.FLUX_COLUMNS,
                                       initial_state=noisy['state_in'][w], return_state=True, forcing_error={'P': {'sigma': 0.3}},
                                       forcing_seed=SEED)
        assert same(ens['state']['data'], noisy['state_out'][w])
    # siblings of one ancestor entered the second window with one state and left it with different ones
    anc = noisy['ancestors'][0]
    twins = [np.nonzero(anc == a)[0] for a in np.unique(anc) if (anc == a).sum() > 1]
    assert twins and not same(noisy['forcing_table'][1][twins[0][0]], noisy['forcing_table'][1][twins[0][1]])


def test_assimilate_continues_bit_for_bit(noisy):
    first = filt(days=slice(0, WINDOW), forcing_error={'P': {'sigma': 0.3}})
    second = filt(days=slice(WINDOW, N_DAYS), forcing_error={'P': {'sigma': 0.3}}, state=first['state'])
    assert same_filter(second, dict(noisy, ess=noisy['ess'][1:], log_evidence=noisy['log_evidence'][1:]))
