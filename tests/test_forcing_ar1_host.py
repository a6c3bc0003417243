"""Autocorrelated forcing errors and seasonal change factors on the host: the NumPy statement of the AR(1) recurrence and its noise
state (simplyp_amd/forcing.py), the invariances it promises (rho = 0 is the independent model; windows and member blocks handed
the state are the whole), its stationarity, the shift groups, and the refusals before any device call."""

import numpy as np
import pandas as pd
import pytest

import helpers
import simplyp_amd as sp
from simplyp_amd import abi, engine, forcing

NAME = 'tarland_2004_dynamic'
E, D = 70, 366
INDEX = pd.date_range('2004-01-01', periods=D)
SEED = 20041
RHO = (0.8, 0.5, 0.95)
CUTS = ((0, 100), (100, 257), (257, D))


@pytest.fixture
def no_device(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(engine, 'get_engine', touched)
    monkeypatch.setattr(engine, 'pinned_empty', touched)


@pytest.fixture(scope='module')
def base():
    """Tarland 2004, [1, 3, D]: Precipitation, PET, T_air."""
    m = helpers.marshal_scenario(NAME, snow=True)
    assert m['forcing'].shape == (1, 3, D)
    return m['forcing']


def full_spec(groups='day', rho=RHO):
    rng = np.random.default_rng(3)
    s = {'P': {'sigma': 0.3, 'groups': groups, 'scale': rng.uniform(0.8, 1.2, E)},
         'PET': {'sigma': 0.1, 'groups': groups, 'scale': 1.05},
         'T_air': {'sigma': 0.5, 'groups': groups, 'offset': rng.uniform(-1, 3, E)}}
    if rho is not None:
        for name, v in zip(abi.FORCING_ROWS, rho):
            s[name]['rho'] = v
    return s


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- rho = 0 is the independent model ----------------------------------------------------------------------------------------

def test_rho_zero_is_todays_table_byte_for_byte(base):
    today = forcing.table(base, forcing.resolve(full_spec(rho=None), INDEX, E, True, SEED), E=E)
    fe = forcing.resolve(full_spec(rho=(0.0, 0.0, 0.0)), INDEX, E, True, SEED)
    assert list(fe['rho']) == [0.0] * 3 and not forcing.any_rho(fe)
    got, noise = forcing.table(base, fe, E=E, return_noise=True)
    assert same(got, today) and (noise[:3] == 0.0).all() and (noise[3:] == -1.0).all()
    fe = forcing.resolve(full_spec(rho=(0.8, 0.0, 0.0)), INDEX, E, True, SEED)
    got, noise = forcing.table(base, fe, E=E, return_noise=True)
    assert forcing.any_rho(fe) and same(got[:, 1:], today[:, 1:]) and not same(got[:, 0], today[:, 0])
    # the noise state names its rows; a row without rho is 0.0 / -1.0, the autocorrelated one ends on the last day's id
    assert abi.FORCING_NOISE_ROWS == ['z_P', 'z_PET', 'z_T_air', 'group_P', 'group_PET', 'group_T_air'] and noise.shape == (6, E)
    assert (noise[1:3] == 0.0).all() and (noise[4:] == -1.0).all() and (noise[3] == float(INDEX[-1].toordinal())).all()
    assert len(np.unique(noise[0])) == E
    # the first day of a stationary start is the independent draw itself
    assert same(got[:, 0, 0], today[:, 0, 0])


def test_the_recurrence_as_written(base):
    """Member 5, row 0, by hand: products rounded one by one, then the sum."""
    fe = forcing.resolve({'P': {'sigma': 0.3, 'rho': 0.8}}, INDEX, E, True, SEED)
    z, z_last, g_last = forcing.ar1_normals(fe, 0, E)
    eps = forcing.normals(fe, 0, E)[5]
    c = float(np.sqrt(1.0 - 0.8 * 0.8))
    want = [eps[0]]
    for d in range(1, D):
        want.append((0.8 * want[-1]) + (c * eps[d]))
    assert same(z[5], np.array(want)) and z_last[5] == want[-1] and g_last == INDEX[-1].toordinal()


# ---- windows and member blocks -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('groups', ['day', 'month', 'array'])
def test_windows_handed_the_state_are_the_whole(base, groups):
    """Cuts at days 100 and 257 fall mid-month: with 'month' groups the next window continues z without a step."""
    g = np.asarray(INDEX.month) // 2 + 100 if groups == 'array' else groups
    fe = forcing.resolve(full_spec(g), INDEX, E, True, SEED)
    whole, end = forcing.table(base, fe, E=E, return_noise=True)
    noise, parts = None, []
    for lo, hi in CUTS:
        part, noise = forcing.table(base[:, :, lo:hi], forcing.day_window(fe, lo, hi), E=E, noise=noise, return_noise=True)
        # and so is the window the public layer resolves from the window's dates
        cut = forcing.cut_group_arrays(full_spec(g), D, lo, hi)
        again = forcing.table(base[:, :, lo:hi], forcing.resolve(cut, INDEX[lo:hi], E, True, SEED), E=E,
                              noise=None if not parts else before)
        assert same(again, part)
        parts.append(part)
        before = noise
    assert same(np.concatenate(parts, axis=2), whole) and same(noise, end)
    # without the state the second window starts anew: it is NOT the slice
    alone = forcing.table(base[:, :, 100:257], forcing.day_window(fe, 100, 257), E=E)
    assert not same(alone, whole[:, :, 100:257])


def test_a_member_block_with_its_noise_columns_is_the_slice_of_the_whole(base):
    fe = forcing.resolve(full_spec(), INDEX, E, True, SEED)
    first, noise = forcing.table(base[:, :, :100], forcing.day_window(fe, 0, 100), E=E, return_noise=True)
    whole, end = forcing.table(base[:, :, 100:], forcing.day_window(fe, 100, D), E=E, noise=noise, return_noise=True)
    blk = forcing.member_block(forcing.day_window(fe, 100, D), 13, E)
    got, end_b = forcing.table(base[:, :, 100:], blk, E=E - 13, noise=noise[:, 13:], return_noise=True)
    assert blk['member0'] == 13 and same(got, whole[13:]) and same(end_b, end[:, 13:])


def test_a_group_id_that_comes_back_is_a_new_step_with_its_old_eps(base):
    g = np.repeat([7, 9, 7], [100, 100, D - 200])
    fe = forcing.resolve({'P': {'sigma': 0.3, 'rho': 0.8, 'groups': g}}, INDEX, E, True, SEED)
    z, _, _ = forcing.ar1_normals(fe, 0, E)
    eps = forcing.normals(fe, 0, E)
    c = float(np.sqrt(1.0 - 0.8 * 0.8))
    z1 = (0.8 * eps[:, 0]) + (c * eps[:, 100])
    assert same(eps[:, 0], eps[:, 200]) and same(z[:, 99], eps[:, 0]) and same(z[:, 150], z1)
    assert same(z[:, D - 1], (0.8 * z1) + (c * eps[:, 0]))


# ---- stationarity ------------------------------------------------------------------------------------------------------------

def test_z_is_stationary_with_lag_one_correlation_rho():
    """seed 20041, E = 70, D = 366, daily groups, rho = (0.8, 0.5, 0.95): the pooled lag-one correlation of z within 4 standard
    errors sqrt((1 - rho^2) / n_pairs) of rho, its variance within 4 standard errors of 1 (the s.e. of the variance of an AR(1)
    sample of n values: sqrt(2 (1 + rho^2) / ((1 - rho^2) n))).  NumPy on these very inputs: the correlations are off by -0.06,
    +0.62 and -0.82 standard errors, the variances are 1.005, 0.994 and 0.952."""
    fe = forcing.resolve({'P': {'sigma': 0.3, 'rho': RHO[0]}, 'PET': {'sigma': 0.1, 'rho': RHO[1]}, 'T_air': {'sigma': 0.5, 'rho': RHO[2]}},
                         INDEX, E, True, SEED)
    for r, rho in enumerate(RHO):
        z = forcing.ar1_normals(fe, r, E)[0]
        a, b = z[:, :-1].ravel(), z[:, 1:].ravel()
        corr = (a * b).mean() / z.var()
        se = np.sqrt((1.0 - rho * rho) / a.size)
        var_se = np.sqrt(2.0 * (1.0 + rho * rho) / ((1.0 - rho * rho) * z.size))
        print('row %d: corr %.4f (rho %.2f, %+.2f se), var %.4f (%+.2f se)' % (r, corr, rho, (corr - rho) / se, z.var(), (z.var() - 1.0) / var_se))
        assert abs(corr - rho) < 4.0 * se, (r, corr, se)
        assert abs(z.var() - 1.0) < 4.0 * var_se, (r, z.var(), var_se)


# ---- seasonal change factors -------------------------------------------------------------------------------------------------

def test_month_of_year_shift_groups(base):
    rng = np.random.default_rng(11)
    s12, o12 = rng.uniform(0.7, 1.3, (12, E)), rng.uniform(-1, 2, 12)
    fe = forcing.resolve({'P': {'scale': s12, 'scale_groups': 'month_of_year'}, 'PET': {'scale': rng.uniform(0.9, 1.1, E)},
                          'T_air': {'offset': o12, 'offset_groups': 'month_of_year'}}, INDEX, E, True, SEED)
    assert fe['shift'].shape == (3, 12, E) and fe['shift_groups'].dtype == np.int32
    assert list(fe['shift_groups']) == [m - 1 for m in INDEX.month] and sorted(set(fe['shift_groups'])) == list(range(12))
    assert (fe['shift'][1] == fe['shift'][1][0]).all()                        # the per-member row: the same for every group
    assert (fe['shift'][2] == o12[:, None]).all()                             # [12] broadcast over members
    got = forcing.table(base, fe, E=E)
    mon = np.asarray(INDEX.month) - 1
    assert same(got[:, 0], base[0, 0][None, :] * s12[mon].T) and same(got[:, 2], np.broadcast_to(base[0, 2] + o12[mon], (E, D)))
    assert same(got[:, 1], base[0, 1][None, :] * fe['shift'][1][0][:, None])
    # windows and member blocks cut the shift groups with the days and the members
    w = forcing.day_window(fe, 100, 257)
    assert same(forcing.table(base[:, :, 100:257], w, E=E), got[:, :, 100:257])
    assert same(forcing.table(base, forcing.member_block(fe, 13, E), E=E - 13), got[13:])
    cut = forcing.cut_group_arrays({'P': {'scale': s12, 'scale_groups': mon}}, D, 100, 257)
    assert list(cut['P']['scale_groups']) == list(mon[100:257])


def test_one_shift_group_is_the_ungrouped_scale(base):
    sc = np.random.default_rng(5).uniform(0.8, 1.2, E)
    plain = forcing.resolve({'P': {'sigma': 0.3, 'rho': 0.8, 'scale': sc}}, INDEX, E, True, SEED)
    one = forcing.resolve({'P': {'sigma': 0.3, 'rho': 0.8, 'scale': sc[None, :], 'scale_groups': np.zeros(D, dtype=int)}}, INDEX, E, True, SEED)
    assert plain['shift'].shape == (2, E) and plain['shift_groups'] is None and one['shift'].shape == (2, 1, E)
    assert same(forcing.table(base, one, E=E), forcing.table(base, plain, E=E))


# ---- refusals ----------------------------------------------------------------------------------------------------------------

MONTHS = np.asarray(INDEX.month) - 1
BAD = [({'P': {'sigma': 0.3, 'rho': -0.1}}, False, r"rho'\] must be finite and in \[0, 0.999\]"),
       ({'P': {'sigma': 0.3, 'rho': 0.9995}}, False, r"rho'\] must be finite and in \[0, 0.999\]"),
       ({'PET': {'sigma': 0.3, 'rho': np.nan}}, False, r"rho'\] must be finite and in \[0, 0.999\]"),
       ({'P': {'sigma': 0.3, 'rho': 'high'}}, False, r"rho'\] must be a number"),
       ({'P': {'rho': 0.5}}, False, r"rho'\] > 0 needs 'sigma' > 0"),
       ({'P': {'scale': np.ones((12, E))}}, False, "more than one dimension needs 'scale_groups'"),
       ({'P': {'scale': np.ones((12, E)), 'scale_groups': MONTHS + 1}}, False, r'shift group ids must lie in \[0, G = 12\)'),
       ({'P': {'scale': np.ones(12), 'scale_groups': -MONTHS}}, False, r'shift group ids must lie in \[0, G = 12\)'),
       ({'P': {'scale': np.ones(12), 'scale_groups': MONTHS}, 'PET': {'scale': np.ones(12), 'scale_groups': MONTHS[::-1].copy()}}, False,
        'share one array of shift groups'),
       ({'P': {'scale': np.ones(12), 'scale_groups': MONTHS}, 'T_air': {'offset': np.ones(13), 'offset_groups': MONTHS}}, True,
        'share one array of shift groups'),
       ({'P': {'scale': np.ones(4097), 'scale_groups': MONTHS}}, False, r'G must lie in \[1, 4096\]'),
       ({'P': {'scale': np.ones(11), 'scale_groups': 'month_of_year'}}, False, 'G = 12'),
       ({'P': {'scale': np.ones((12, E + 1)), 'scale_groups': 'month_of_year'}}, False, r'must have shape \[G\] or \[G, E = 70\]'),
       ({'P': {'scale': np.ones(12), 'scale_groups': 'season'}}, False, "'month_of_year' or an int array"),
       ({'P': {'scale': np.ones(12), 'scale_groups': MONTHS[:-1]}}, False, "'month_of_year' or an int array"),
       ({'P': {'scale_groups': 'month_of_year'}}, False, 'one entry per shift group'),
       ({'P': {'scale': np.ones(12), 'offset_groups': 'month_of_year'}}, False, 'keys among'),
       ({'T_air': {'offset': np.ones(12), 'scale_groups': 'month_of_year'}}, True, 'keys among')]


@pytest.mark.parametrize('spec,snow,match', BAD)
def test_resolve_refuses(spec, snow, match):
    with pytest.raises(ValueError, match=match):
        forcing.resolve(spec, INDEX, E, snow)


@pytest.mark.parametrize('spec,snow,match', [BAD[0], BAD[4], BAD[5], BAD[6], BAD[8], BAD[10], BAD[16]])
def test_public_calls_refuse_before_any_device_call(no_device, spec, snow, match):
    inputs = helpers.scenario_inputs(NAME)
    with pytest.raises(ValueError, match=match):
        sp.run_simply_p_ensemble(*inputs, n_members=E, forcing_error=spec, snow_in_kernel=snow)
    with pytest.raises(ValueError, match=match):                 # when the generator is created
        sp.run_simply_p_ensemble_windows(*helpers.scenario_inputs(NAME), window=100, n_members=E, forcing_error=spec,
                                         snow_in_kernel=snow).__next__()
    obs = helpers.observations(inputs[2]['st_dt'], inputs[2]['end_dt'])
    with pytest.raises(ValueError, match=match):
        sp.assimilate(*helpers.scenario_inputs(NAME), obs, priors={'fc': (200.0, 380.0), 'm_Q': (0.01, 1.0)}, n_particles=E,
                      forcing_error=spec)


def test_check_resolved_and_the_noise_state_shape(base):
    fe = forcing.resolve(full_spec(), INDEX, E, True, SEED)
    with pytest.raises(ValueError, match='rho needs one finite entry'):
        forcing.check_resolved(dict(fe, rho=np.array([0.8, 1.0, 0.0])), E, D, 3)
    with pytest.raises(ValueError, match='rho > 0 needs sigma > 0'):
        forcing.check_resolved(dict(fe, sigma=np.array([0.0, 0.1, 0.5])), E, D, 3)
    with pytest.raises(ValueError, match=r'noise state must have shape \[6, E = 70\]'):
        forcing.table(base, fe, E=E, noise=np.zeros((6, E - 1)))
    grouped = forcing.resolve({'P': {'scale': np.ones(12), 'scale_groups': 'month_of_year'}}, INDEX, E, True, SEED)
    with pytest.raises(ValueError, match=r'one id in \[0, G = 12\) per day'):
        forcing.check_resolved(dict(grouped, shift_groups=grouped['shift_groups'] + 1), E, D, 3)
    with pytest.raises(ValueError, match='shift with shift_groups must have shape'):
        forcing.check_resolved(dict(grouped, shift=grouped['shift'][:, 0]), E, D, 3)
    forcing.check_resolved({k: v for k, v in fe.items() if k not in ('rho', 'shift_groups')}, E, D, 3)     # the earlier resolved form


def test_opts_carry_the_new_fields_and_default_to_off():
    o = abi.make_opts()
    assert list(o.forcing_rho) == [0.0] * 3 and not o.forcing_noise_in and not o.forcing_noise_out
    assert not o.forcing_shift_group_of_day and o.forcing_shift_groups == 0 and o.forcing_reserved2 == 0
    names = [f for f, _ in abi.Opts._fields_]
    assert names[names.index('forcing_table') + 1:] == ['forcing_rho', 'forcing_noise_in', 'forcing_noise_out',
                                                        'forcing_shift_group_of_day', 'forcing_shift_groups', 'forcing_reserved2']
    c = o.copy()
    c.forcing_rho[0] = 0.8
    assert o.forcing_rho[0] == 0.0 and c.forcing_rho[0] == 0.8
