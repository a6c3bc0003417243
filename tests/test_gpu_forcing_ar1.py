"""Autocorrelated forcing errors and seasonal change factors on the device: the AR(1) generator's table and noise state against
the NumPy statement (simplyp_amd/forcing.py), its rows without rho against the independent kernel, the tile edges device against
device (windows, member blocks, device blocks, in place), the run that reads the table, the CPU oracle on the mirror's table, the
shift groups through both kernels, the C-level refusals, and the particle filter that owns a noise state.

E = 70 (no multiple of 64, nor of the 4 waves of a block), Tarland 2004 (D = 366: five full 64-day tiles and a 46-day tail)."""

import numpy as np
import pytest

import helpers
import simplyp_amd as sp
from simplyp_amd import abi, engine, forcing, marshal

pytestmark = pytest.mark.gpu

NAME = 'tarland_2004_dynamic'
E, D, SEED = 70, 366, 20041
SIGMA = (0.3, 0.1, 0.5)
RHO = (0.8, 0.5, 0.95)


def z_tol_ar(rho):
    """tests/test_gpu_forcing.py derives Z_TOL = 2^-45 for one draw.  The recurrence z = rho z_prev + c eps contracts the error
    of z_prev by rho at each step and adds c 2^-45 from the draw and its own three roundings on values <= sqrt(2) 8.58
    (<= 0.15 2^-45): the geometric series sums to (c + 0.15) 2^-45 / (1 - rho)."""
    return (np.sqrt(1.0 - rho * rho) + 0.15) * 2.0 ** -45 / (1.0 - rho)


def rel_tol(sigma, rho):
    """P', PET' = v exp(sigma z - sigma^2 / 2): the argument is off by sigma Z_TOL_AR, exp and the roundings by 2^-44 at most."""
    return 2.0 * max(sigma * z_tol_ar(rho), 2.0 ** -44)


def problem(name=NAME, snow=False, n=E, solver=None, mask=marshal.MASK_REACH5):
    m = helpers.marshal_scenario(name, E=n, out_mask=mask, solver=solver, snow=snow)
    m['member_params'][marshal.PM_NAMES.index('fc')] *= np.random.default_rng(7).uniform(0.9, 1.1, n)
    return m


def spec(snow, groups='day', rho=RHO, shift=True, sigma=SIGMA):
    rng = np.random.default_rng(3)
    s = {'P': {'sigma': sigma[0], 'groups': groups, 'rho': rho[0]}, 'PET': {'sigma': sigma[1], 'groups': groups, 'rho': rho[1]}}
    if shift:
        s['P']['scale'], s['PET']['scale'] = rng.uniform(0.8, 1.2, E), 1.05
    if snow:
        s['T_air'] = {'sigma': sigma[2], 'groups': groups, 'rho': rho[2]}
        if shift:
            s['T_air']['offset'] = rng.uniform(-1.0, 3.0, E)
    return s


def run(eng, m, days=None, **kw):
    f, doy = (m['forcing'], m['doy']) if days is None else (np.ascontiguousarray(m['forcing'][:, :, days]), np.ascontiguousarray(m['doy'][days]))
    rhs = eng.torch.zeros((m['member_params'].shape[1],), dtype=eng.torch.int32, device=eng.tdev)
    out, status, stats = eng.run(f, doy, m['member_params'], m['reach_params'], m['up_ptr'], m['up_idx'], m['opts'], member_rhs=rhs, **kw)
    return out.cpu().numpy(), status.cpu().numpy(), rhs.cpu().numpy(), stats


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def host(t):
    return t.cpu().numpy()


# ---- the table and the noise state against the mirror ------------------------------------------------------------------------

@pytest.mark.parametrize('snow', [False, True], ids=['rows2', 'rows3'])
@pytest.mark.parametrize('groups', ['day', 'month_array', 'one_group'])
def test_table_matches_the_mirror(engine0, snow, groups):
    """sigma = (0.3, 0.1, 0.5), rho = (0.8, 0.5, 0.95), scales and offset given.  Derived bounds, which are what is asserted:
    T_air within sigma_T Z_TOL_AR(0.95) = 1.3e-13 absolute, P within 2 max(sigma Z_TOL_AR, 2^-44) = 1.1e-13 relative, PET 1.1e-13
    relative; dry days exact.  Measured worst cases on MI355X, far inside the derived bounds, which stay: P and PET 4.9e-16
    relative, T_air 3.6e-15 absolute, the z rows of the noise state 5.6e-16 absolute (bounds 1.1e-13, 5.8e-14, 2.6e-13)."""
    m = problem(snow=snow)
    index = m['met'].index
    g = {'day': 'day', 'month_array': np.asarray(index.year * 12 + index.month - 1), 'one_group': np.full(D, 5)}[groups]
    fe = forcing.resolve(spec(snow, g), index, E, snow, SEED)
    _, status, _, stats = run(engine0, m, forcing_error=fe, keep_forcing_table=True, forcing_noise_out=True)
    got, (want, want_nz) = host(stats['forcing_table']), forcing.table(m['forcing'], fe, E=E, return_noise=True)
    assert got.shape == want.shape == (E, 3 if snow else 2, D) and status.max() == 0
    dry = m['forcing'][0, 0] == 0
    assert dry.any() and (got[:, 0, dry] == 0).all() and (got[:, 0, ~dry] > 0).all()
    for r in (0, 1):
        err, tol = helpers.max_rel_err(got[:, r], want[:, r], floor=1e-300), rel_tol(SIGMA[r], RHO[r])
        print('row %d max rel err %.3e (bound %.3e)' % (r, err, tol))
        assert err <= tol, (r, err)
    if snow:
        err, tol = np.abs(got[:, 2] - want[:, 2]).max(), SIGMA[2] * z_tol_ar(RHO[2])
        print('T_air max abs err %.3e (bound %.3e)' % (err, tol))
        assert err <= tol, err
    nz = host(stats['forcing_noise'])
    rows = 3 if snow else 2
    assert nz.shape == (6, E) and same(nz[3:], want_nz[3:]) and (nz[3:3 + rows] == float(fe['groups'][0][-1])).all()
    for r in range(rows):
        err = np.abs(nz[r] - want_nz[r]).max()
        print('z row %d max abs err %.3e (bound %.3e)' % (r, err, z_tol_ar(RHO[r])))
        assert err <= z_tol_ar(RHO[r]), (r, err)
    if not snow:
        assert (nz[2] == 0.0).all() and (nz[5] == -1.0).all()


def test_noise_state_of_rows_without_rho_and_the_rest_bit_for_bit(engine0):
    """rho = (0.8, 0, 0): rows 1 and 2 are the independent kernel's (the rho = 0 call, same seed) bit for bit, and their noise
    state is exactly 0.0 / -1.0."""
    m = problem(snow=True)
    fe = forcing.resolve(spec(True, 'month', rho=(0.8, 0.0, 0.0)), m['met'].index, E, True, SEED)
    fe0 = forcing.resolve(spec(True, 'month', rho=(0.0, 0.0, 0.0)), m['met'].index, E, True, SEED)
    _, _, _, stats = run(engine0, m, forcing_error=fe, keep_forcing_table=True, forcing_noise_out=True)
    _, _, _, stats0 = run(engine0, m, forcing_error=fe0, keep_forcing_table=True)
    got, ind = host(stats['forcing_table']), host(stats0['forcing_table'])
    assert same(got[:, 1:], ind[:, 1:]) and not same(got[:, 0], ind[:, 0]) and 'forcing_noise' not in stats0
    nz, want = host(stats['forcing_noise']), forcing.table(m['forcing'], fe, E=E, return_noise=True)[1]
    assert (nz[1:3] == 0.0).all() and (nz[4:] == -1.0).all() and same(nz[3:], want[3:])
    assert np.abs(nz[0] - want[0]).max() <= z_tol_ar(0.8) and len(np.unique(nz[0])) == E
    with pytest.raises(ValueError, match='need forcing_error with some rho > 0'):
        run(engine0, m, forcing_error=fe0, forcing_noise_out=True)
    with pytest.raises(ValueError, match='need forcing_error with some rho > 0'):
        run(engine0, m, forcing_noise_out=True)


# ---- tile edges, bit for bit, device against device ------------------------------------------------------------------------------

def public(groups='day', snow=True, **kw):
    inputs = helpers.scenario_inputs(NAME)
    fc = float(inputs[5]['fc']) * np.random.default_rng(7).uniform(0.9, 1.1, E)
    return inputs, dict(overrides={'fc': fc}, forcing_error=spec(snow, groups), forcing_seed=SEED, snow_in_kernel=snow, **kw)


_WHOLE = {}


def whole(groups):
    if groups not in _WHOLE:
        inputs, kw = public(groups)
        _WHOLE[groups] = sp.run_simply_p_ensemble(*inputs, return_state=True, **kw)
    return _WHOLE[groups]


@pytest.mark.parametrize('groups,cuts', [('day', (100, 257)), ('month', (100, 257)), ('day', (10,))], ids=['day', 'month', 'ten_days'])
def test_windows_laid_end_to_end_are_the_one_call(groups, cuts):
    """Cuts at days 100 and 257: mid-month, inside a 64-day tile of the whole, a 46-day tail; and a first window of 10 days."""
    one = whole(groups)
    inputs, kw = public(groups)
    index = inputs[0].index
    parts = list(sp.run_simply_p_ensemble_windows(*inputs, window=[index[0]] + [index[c] for c in cuts], **kw))
    assert [p['window'][2:] for p in parts] == list(zip((0,) + cuts, cuts + (D,)))
    assert same(np.concatenate([p['data'] for p in parts], axis=1), one['data']) and int(one['status'].max()) == 0
    assert one['state']['forcing_noise'].shape == (6, E) and same(host(parts[-1]['state']['forcing_noise']), one['state']['forcing_noise'])
    assert same(host(parts[-1]['state']['data']), one['state']['data'])


def test_two_device_blocks_are_the_one_call():
    one = whole('day')
    inputs, kw = public('day', devices=[0, 0])
    res = sp.run_simply_p_ensemble(*inputs, return_state=True, **kw)
    assert res['stats']['bounds'] == [[0, 35], [35, 70]] and same(res['data'], one['data'])
    assert same(res['state']['forcing_noise'], one['state']['forcing_noise'])
    # the per-block list continues a run
    inputs, kw = public('day', devices=[0, 0])
    met = inputs[0]
    first = sp.run_simply_p_ensemble(met.iloc[:100], *inputs[1:], return_state='device', **kw)
    assert [tuple(t.shape) for t in first['state']['forcing_noise']] == [(6, 35), (6, 35)]
    inputs, kw = public('day', devices=[0, 0])
    second = sp.run_simply_p_ensemble(inputs[0].iloc[100:], *inputs[1:], initial_state=first['state'], **kw)
    assert same(second['data'], one['data'][:, 100:])


def test_without_rho_the_state_gains_no_key():
    inputs, kw = public('day')
    kw['forcing_error'] = {'P': {'sigma': 0.3}}
    res = sp.run_simply_p_ensemble(*inputs, return_state=True, **kw)
    assert 'forcing_noise' not in res['state']


def test_a_member_block_with_its_noise_columns_and_in_place(engine0):
    m = problem(snow=True)
    fe = forcing.resolve(spec(True), m['met'].index, E, True, SEED)
    a, b = slice(0, 100), slice(100, D)
    _, _, _, st1 = run(engine0, m, days=a, forcing_error=forcing.day_window(fe, 0, 100), forcing_noise_out=True)
    nz = st1['forcing_noise']
    fe_b = forcing.day_window(fe, 100, D)
    out, _, rhs, st2 = run(engine0, m, days=b, forcing_error=fe_b, forcing_noise_in=nz, forcing_noise_out=True, keep_forcing_table=True)
    assert st2['forcing_noise'].data_ptr() != nz.data_ptr()
    blk = dict(m, member_params=np.ascontiguousarray(m['member_params'][:, 13:]), reach_params=np.ascontiguousarray(m['reach_params'][:, :, 13:]))
    out_b, _, rhs_b, st_b = run(engine0, blk, days=b, forcing_error=forcing.member_block(fe_b, 13, E), keep_forcing_table=True,
                                forcing_noise_in=np.ascontiguousarray(host(nz)[:, 13:]), forcing_noise_out=True)
    assert same(host(st_b['forcing_table']), host(st2['forcing_table'])[13:]) and same(host(st_b['forcing_noise']), host(st2['forcing_noise'])[:, 13:])
    assert same(out_b, out[..., 13:]) and same(rhs_b, rhs[13:])
    # in place: the one buffer as input and output
    buf = nz.clone()
    out_i, _, _, st_i = run(engine0, m, days=b, forcing_error=fe_b, forcing_noise_in=buf, forcing_noise_out=buf, keep_forcing_table=True)
    assert st_i['forcing_noise'] is buf and same(host(buf), host(st2['forcing_noise'])) and not same(host(buf), host(nz))
    assert same(host(st_i['forcing_table']), host(st2['forcing_table'])) and same(out_i, out)
    # and the two pieces are the one call
    _, _, _, st = run(engine0, m, forcing_error=fe, keep_forcing_table=True, forcing_noise_out=True)
    assert same(host(st['forcing_table'])[:, :, 100:], host(st2['forcing_table'])) and same(host(st['forcing_noise']), host(st2['forcing_noise']))


# ---- the run reads exactly that table ----------------------------------------------------------------------------------------

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


# ---- against the oracle ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('solver,tol', [(dict(integrator='rk4', substeps=32), 1e-10), (None, helpers.TOL_WORKING)])
def test_kernel_on_the_generated_table_matches_the_oracle_on_the_mirrors(engine0, oracle_lib, solver, tol):
    """The CPU oracle given the mirror's AR(1) table as 8 forcing sets, at test_kernel_matches_oracle's tolerance for the solver."""
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


# ---- seasonal change factors -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('ar1', [False, True], ids=['independent_kernel', 'ar1_kernel'])
def test_month_of_year_scale_is_base_times_scale_of_the_month(engine0, ar1):
    m = problem(snow=True)
    index = m['met'].index
    rng = np.random.default_rng(11)
    s12, o12 = rng.uniform(0.7, 1.3, (12, E)), rng.uniform(-1.0, 2.0, 12)
    s = {'P': {'scale': s12, 'scale_groups': 'month_of_year'}, 'T_air': {'offset': o12, 'offset_groups': np.asarray(index.month) - 1}}
    if ar1:
        s['PET'] = {'sigma': 0.1, 'rho': 0.5}
    fe = forcing.resolve(s, index, E, True, SEED)
    _, status, _, stats = run(engine0, m, forcing_error=fe, keep_forcing_table=True)
    got, mon = host(stats['forcing_table']), np.asarray(index.month) - 1
    assert status.max() == 0 and same(got[:, 0], m['forcing'][0, 0][None, :] * s12[mon].T)
    assert same(got[:, 2], np.broadcast_to(m['forcing'][0, 2] + o12[mon], (E, D)))
    if ar1:
        want = forcing.table(m['forcing'], fe, E=E)
        assert helpers.max_rel_err(got[:, 1], want[:, 1], floor=1e-300) <= rel_tol(0.1, 0.5)
    else:
        assert same(got[:, 1], np.broadcast_to(m['forcing'][0, 1], (E, D)))


@pytest.mark.parametrize('rho', [0.0, 0.8], ids=['independent_kernel', 'ar1_kernel'])
def test_one_shift_group_is_the_ungrouped_call(engine0, rho):
    m = problem(snow=False)
    sc = np.random.default_rng(5).uniform(0.8, 1.2, E)
    tables = []
    for grouped in (False, True):
        row = {'sigma': 0.3, 'rho': rho, 'scale': sc[None, :] if grouped else sc}
        if grouped:
            row['scale_groups'] = np.zeros(D, dtype=int)
        fe = forcing.resolve({'P': row}, m['met'].index, E, False, SEED)
        out, _, _, stats = run(engine0, m, forcing_error=fe, keep_forcing_table=True)
        tables.append((host(stats['forcing_table']), out))
    assert same(tables[0][0], tables[1][0]) and same(tables[0][1], tables[1][1])


# ---- refusals ----------------------------------------------------------------------------------------------------------------

def _edit(o, keep, eng, **kw):
    for k, v in kw.items():
        if k.startswith('rho') or k.startswith('sigma'):
            getattr(o, 'forcing_' + k[:-1])[int(k[-1])] = v
        elif k == 'all_rho':
            for r in range(3):
                o.forcing_rho[r] = v
        elif k == 'shift_group_array':
            keep.append(eng.to_device(np.zeros(D, dtype=np.int32), eng.torch.int32))
            o.forcing_shift_group_of_day = keep[-1].data_ptr()
        else:
            setattr(o, k, v)


@pytest.mark.parametrize('snow,edit,match', [
    (False, dict(rho0=-0.1), r'forcing_rho\[0\] \(P\) must be finite and in \[0, 0.999\]'),
    (False, dict(rho1=0.9995), r'forcing_rho\[1\] \(PET\) must be finite and in \[0, 0.999\]'),
    (True, dict(rho2=float('nan')), r'forcing_rho\[2\] \(T_air\) must be finite and in \[0, 0.999\]'),
    (False, dict(rho0=float('inf')), r'forcing_rho\[0\] \(P\) must be finite and in \[0, 0.999\]'),
    (False, dict(sigma0=0.0), r'forcing_rho\[0\] \(P\) > 0 needs forcing_sigma\[0\] > 0'),
    (False, dict(all_rho=0.0), 'need some forcing_rho > 0'),
    (False, dict(forcing_shift_groups=-1), r'forcing_shift_groups must be 0 or in \[1, 4096\]'),
    (False, dict(forcing_shift_groups=4097, shift_group_array=1), r'forcing_shift_groups must be 0 or in \[1, 4096\]'),
    (False, dict(forcing_shift_groups=1), 'needs forcing_shift_group_of_day and forcing_shift'),
    (False, dict(forcing_shift_groups=1, shift_group_array=1, forcing_shift=None, forcing_shift_rows=0),
     'needs forcing_shift_group_of_day and forcing_shift'),
    (False, dict(shift_group_array=1), 'forcing_shift_group_of_day needs forcing_shift_groups >= 1'),
    (False, dict(forcing_error=0), 'need forcing_error = 1'),
    (False, dict(forcing_error=0, all_rho=0.0), 'need forcing_error = 1'),
    (False, dict(forcing_error=0, all_rho=0.0, forcing_noise_out=None, forcing_shift_groups=12), 'need forcing_error = 1')])
def test_refusals_launch_nothing(engine0, snow, edit, match):
    """Every new host-side refusal: the output, the table and the noise-out buffer stay at their fill value."""
    m = problem(snow=snow)
    fe = forcing.resolve(spec(snow), m['met'].index, E, snow, SEED)
    o, keep = engine0._forcing_opts(m['opts'], fe, E, D, 3 if snow else 2, None, True)
    table, noise_out = keep[0], keep[4]
    table.fill_(-777.0)
    noise_out.fill_(-777.0)
    _edit(o, keep, engine0, **edit)
    out = engine0.torch.full((5, D, 1, E), -777.0, dtype=engine0.torch.float64, device=engine0.tdev)
    with pytest.raises(engine.EngineError, match=match):
        engine0.run(m['forcing'], m['doy'], m['member_params'], m['reach_params'], m['up_ptr'], m['up_idx'], o, out=out)
    engine0.torch.cuda.synchronize()
    assert bool((table == -777.0).all()) and bool((out == -777.0).all()) and bool((noise_out == -777.0).all())


# ---- the particle filter -----------------------------------------------------------------------------------------------------

N_DAYS, WINDOW = 60, 30
FE = {'P': {'sigma': 0.2, 'rho': 0.7}}


def filt(days=slice(0, N_DAYS), **kw):
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
    obs_dict = helpers.observations(p_SU['st_dt'], p_SU['end_dt'])
    priors = {nm: (0.7 * float(p[nm]), 1.3 * float(p[nm])) for nm in ('fc', 'T_g', 'a_Q')}
    priors['m_Q'] = (0.01, 1.0)
    args = dict(priors=priors, variables=['Q'], n_particles=E, window=WINDOW, seed=SEED, record=True, forcing_error=FE)
    args.update(kw)
    return sp.assimilate(met.iloc[days], p_struc, p_SU, p_LU, p_SC, p, dyn, obs_dict, **args)


def test_assimilate_owns_gathers_and_continues_the_noise_state():
    both = filt()
    assert len(both['windows']) == 2 and both['resampled'].all() and both['state']['forcing_noise'].shape == (6, E)
    assert both['forcing_noise_in'][0] is None and both['forcing_noise_out'][0].shape == (6, E)
    # after a resampled window the noise state is the run's gathered by the ancestors
    anc = both['ancestors'][0]
    assert len(np.unique(anc)) < E and same(both['forcing_noise_in'][1], both['forcing_noise_out'][0][:, anc])
    assert same(both['state']['forcing_noise'], both['forcing_noise_out'][1][:, both['ancestors'][1]])
    # the second window's table is the mirror's continued from that state
    met = helpers.scenario_inputs(NAME)[0]
    base = marshal.forcing_arrays(met)[0]
    fe = forcing.resolve(FE, met.index[WINDOW:N_DAYS], E, False, SEED)
    want, want_nz = forcing.table(base[:, :, WINDOW:N_DAYS], fe, E=E, noise=both['forcing_noise_in'][1], return_noise=True)
    got = both['forcing_table'][1]
    assert helpers.max_rel_err(got[:, 0], want[:, 0], floor=1e-300) <= rel_tol(0.2, 0.7) and same(got[:, 1], want[:, 1])
    assert np.abs(both['forcing_noise_out'][1][0] - want_nz[0]).max() <= z_tol_ar(0.7) and same(both['forcing_noise_out'][1][3:], want_nz[3:])
    # a filter continued from the state is the one filter, bit for bit
    first = filt(days=slice(0, WINDOW))
    assert same(first['state']['forcing_noise'], both['forcing_noise_in'][1])
    second = filt(days=slice(WINDOW, N_DAYS), state=first['state'])
    for k in ('theta', 'log_weights'):
        assert same(np.asarray(second[k]), np.asarray(both[k])), k
    assert same(second['ess'], both['ess'][1:]) and same(second['log_evidence'], both['log_evidence'][1:])
    assert same(second['state']['data'], both['state']['data']) and same(second['state']['forcing_noise'], both['state']['forcing_noise'])
    assert second['state']['forcing_noise'].shape == (6, E) and same(second['forcing_table'][0], both['forcing_table'][1])
