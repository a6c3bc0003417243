"""``run_simply_p_ensemble`` with every product asked for at once, against the calls that ask for one product alone.

The other public tests exercise one option at a time; what the options share inside one block pass -- the participant mask, the
integer weights, ``member_of_slot``, the band adapter -- shows only when they meet.  70 members (two 64-lane waves, so that slot
order can differ from member order) over all of 2004, one of them non-finite, three left out of the bands.  Equality throughout:
``np.array_equal`` with NaN positions equal; ``info`` dictionaries, ``stats`` and timings are left out."""

import numpy as np
import pytest

import helpers
import simplyp_amd as sp
from simplyp_amd import abi, marshal

pytestmark = pytest.mark.gpu

NAME = 'tarland_2004_dynamic'
E = 70
NAN_MEMBER = 41
Q = [0.025, 0.5, 0.975]
MEMBERS = np.ones(E, dtype=bool)
MEMBERS[[3, 40, 66]] = False
BANDS = dict(quantiles=Q, quantile_members=MEMBERS)
PRODUCTS = dict(
    gof=dict(obs=True, spearman=True),
    quantiles=dict(BANDS),
    time_quantiles=dict(BANDS, time_quantiles=[0.05, 0.5, 1.0], time_quantile_series=['Q_cumecs', 'Qr'], time_quantile_periods='annual'),
    predictive=dict(BANDS, predictive_series=['Q_cumecs', 'TDP_mgl'], predictive_m={'Q_cumecs': 0.1}),
    scores=dict(obs=True, score=True, quantile_members=MEMBERS, predictive_series=['Q_cumecs', 'TDP_mgl'], predictive_m={'Q_cumecs': 0.1}),
    pareto=dict(obs=True, pareto=[('NSE', 'Q'), ('Bias (%)', 'Q')], quantile_members=MEMBERS),
    state=dict(return_state=True))
WEIGHTED = ('quantiles', 'time_quantiles', 'predictive', 'scores')         # the products the weights enter
ALWAYS = ('status', 'data', 'columns', 'reaches')


def overrides():
    """As tests/test_gpu_pareto_public.py::overrides, one member made non-finite through T_g."""
    base = helpers.marshal_scenario(NAME, E=1)['member_params'][:, 0]
    rng = np.random.default_rng(E)
    over = {nm: base[marshal.PM_NAMES.index(nm)] * rng.uniform(lo, hi, E)
            for nm, lo, hi in (('a_Q', 0.6, 1.6), ('T_g', 0.7, 1.4), ('E_M', 0.5, 2.0), ('fc', 0.85, 1.15))}
    over['T_g'][NAN_MEMBER] = np.nan                                 # marshal.validate_ensemble does not look at T_g
    return over


def call(name=NAME, obs=False, flags=None, over=None, **kw):
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(name)
    if flags is not None:
        p_struc['In_final_flux?'] = flags
    if obs:
        kw['obs_dict'] = helpers.observations(p_SU['st_dt'], p_SU['end_dt'])
    return sp.run_simply_p_ensemble(met, p_struc, p_SU, p_LU, p_SC, p, dyn, overrides=overrides() if over is None else over,
                                    outputs=list(marshal.REACH5_COLUMNS), **kw)


def merged(*options, **more):
    kw = {}
    for o in options:
        kw.update(o)
    kw.update(more)
    return kw


def same(got, want, path):
    """Every array under every key equal, NaN positions included; 'info' dictionaries (kernel times, counters) are not compared.
    The run's 'stats' is a key of the result itself and never handed in here; a 'stats' further down is a list of names."""
    if isinstance(want, dict):
        assert isinstance(got, dict) and set(got) == set(want), (path, sorted(got), sorted(want))
        for k in want:
            if k != 'info':
                same(got[k], want[k], path + (k,))
    elif isinstance(want, (list, tuple)) and any(isinstance(x, (dict, np.ndarray)) for x in want):
        assert len(got) == len(want), path
        for i, (g, w) in enumerate(zip(got, want)):
            same(g, w, path + (i,))
    elif isinstance(want, np.ndarray):
        assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape, (path, got.dtype, want.dtype)
        assert np.array_equal(got, want, equal_nan=want.dtype.kind == 'f'), path
    else:
        assert type(got) is type(want) and (got == want or (want != want and got != got)), (path, got, want)


def compare(all_at_once, alone, keys=tuple(PRODUCTS)):
    for key in keys:
        same(all_at_once[key], alone[key][key], (key,))
        for k in ALWAYS:
            same(all_at_once[k], alone[key][k], (key, k))


@pytest.fixture(scope='module')
def alone(engine0):
    """One call per product, asking for that product and what it requires."""
    return {key: call(**kw) for key, kw in PRODUCTS.items()}


@pytest.fixture(scope='module')
def together(engine0):
    return call(**merged(*PRODUCTS.values()))


def test_the_setup_is_what_it_says(together):
    status = together['status']
    assert status[NAN_MEMBER] & abi.STATUS_NONFINITE and (np.delete(status, NAN_MEMBER) & abi.STATUS_NONFINITE == 0).all()
    assert together['columns'] == marshal.REACH5_COLUMNS and together['data'].shape == (5, 366, 1, E)
    assert together['quantiles']['n_members'] == E - 4 and together['pareto']['n_members'] <= E - 4
    assert together['scores']['series'] == ['Q_cumecs', 'TDP_mgl'] and together['scores']['n_members'] == E - 4
    assert together['time_quantiles']['data'].shape == (3, 2, 1, 1, E) and np.isnan(together['time_quantiles']['data'][2, ..., NAN_MEMBER]).all()
    assert together['predictive']['overall'] is not None and np.isfinite(together['quantiles']['data']).all()


def test_all_products_at_once_equal_each_alone(together, alone):
    compare(together, alone)


def test_all_products_at_once_under_log_weights(together, alone):
    lw = np.random.default_rng(7).normal(size=E)
    got = call(**merged(*PRODUCTS.values(), quantile_log_weights=lw))
    weighted = {key: call(**merged(PRODUCTS[key], quantile_log_weights=lw)) for key in WEIGHTED}
    compare(got, weighted, WEIGHTED)
    compare(got, alone, [k for k in PRODUCTS if k not in WEIGHTED])            # the weights do not enter these
    pred = got['predictive']
    bands = [got['quantiles'], got['time_quantiles']['quantiles'], pred, pred['param_only'], pred['overall']]
    assert all(b['rule'] == 'inverted_cdf' for b in bands)
    totals = {int(b['weight_total']) for b in bands} | {int(got['scores']['weight_total'])}
    assert len(totals) == 1 and totals.pop() > 0
    assert not np.array_equal(got['quantiles']['data'], together['quantiles']['data'], equal_nan=True)


def test_slot_order_changes_the_table_only(together):
    """``out_slot_order=1``: every product comes back in member order and equal, the table alone in slot order.  Left out of the
    comparison: the scores' ``abs_err`` and what is computed from it (``crps``, ``mean_crps``) -- that sum over the members is
    taken in slot order and differs from the member-order run's in the last bit (at most 8e-16 relative, 1 in 4 rows; the
    parent of this test's commit does the same)."""
    got = call(**merged(*PRODUCTS.values(), solver=dict(balance=1, out_slot_order=1)))
    mos = got['stats']['member_of_slot'].cpu().numpy()
    assert sorted(mos.tolist()) == list(range(E)) and not np.array_equal(mos, np.arange(E))
    summed = ('abs_err', 'crps', 'mean_crps')
    less = lambda sc: dict(sc, **{part: {k: v for k, v in sc[part].items() if k not in summed} for part in ('param_only', 'overall')})
    for key in list(PRODUCTS) + ['status', 'columns', 'reaches']:
        same(less(got[key]) if key == 'scores' else got[key], less(together[key]) if key == 'scores' else together[key], (key,))
    back = np.empty_like(got['data'])
    back[..., mos] = got['data']                                     # slot j holds member mos[j]
    assert np.array_equal(back, together['data'], equal_nan=True)


def test_two_contexts_on_one_device_equal_one(engine0):
    """A reach network split over ``devices=[0, 0]``: the per-member products joined along the member axis."""
    rng = np.random.default_rng(2)
    over = dict(fc=290 * rng.uniform(0.9, 1.1, E), f_TDP=rng.uniform(0.5, 0.9, E))
    kw = dict(name='confluence3_nc_2004', flags=[1, 0, 1], over=over, obs=True, time_quantiles=[0.05, 0.5, 1.0], waterbody=True,
              return_state=True)
    one, two = call(**kw), call(devices=[0, 0], **kw)
    bounds = two['stats']['bounds']
    assert len(bounds) == 2 and bounds[0][0] == 0 and bounds[0][1] == bounds[1][0] and bounds[1][1] == E
    assert one['waterbody']['reaches'] == [1, 3] and one['state']['data'].shape[-1] == E
    for key in ('gof', 'time_quantiles', 'waterbody', 'state', 'status', 'data', 'columns', 'reaches'):
        same(two[key], one[key], (key,))
