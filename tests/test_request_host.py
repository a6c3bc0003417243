"""The host-only rules the public calls share (simplyp_amd/request.py), each against the inputs its former copies saw, and the
one rule for the reference's in-place edits (marshal.reference_edits): a call refused after its prologue leaves the caller's
frames as a completed call does.  No device: ``engine.get_engine`` and ``engine.pinned_empty`` are patched to fail."""

import numpy as np
import pandas as pd
import pytest

import helpers
import simplyp_amd as sp
from simplyp_amd import abi, engine, marshal, request

NAME = 'tarland_2004_dynamic'
AMONG = "the reference's columns and the df_R names"


def refused(match, fn, *args, **kw):
    with pytest.raises(ValueError, match=match):
        fn(*args, **kw)


# ---- probabilities ------------------------------------------------------------------------------------------------------

def test_probabilities():
    assert request.probabilities('quantiles', [0.025, 0.5, 1.0]) == [0.025, 0.5, 1.0]
    assert request.probabilities('quantiles', 0.5) == [0.5]                      # a scalar is one probability
    assert request.probabilities('quantiles', np.linspace(0, 1, 16)) == list(np.linspace(0, 1, 16))
    for bad in ([], np.linspace(0, 1, 17), [-0.1], [0.5, 1.0 + 1e-12], [np.nan]):
        refused('time_quantiles must be 1 to 16 probabilities in \\[0, 1\\]', request.probabilities, 'time_quantiles', bad)


# ---- series -------------------------------------------------------------------------------------------------------------

def test_series_ids_and_the_columns_they_add():
    names, ids, needs = request.series_ids('predictive_series', ['TDP_mgl', 'Qr', 'D_snow'], AMONG)
    assert names == ['TDP_mgl', 'Qr', 'D_snow']
    assert needs == ['Qr', 'Msus_kg/day', 'TDP_kg/day', 'PP_kg/day', 'D_snow']      # a df_R series needs the four fluxes, a column itself
    assert ids == [abi.TQ_DERIVED + abi.TQ_DERIVED_SERIES.index('TDP_mgl'), marshal.ALL_COLUMNS.index('Qr'),
                   marshal.ALL_COLUMNS.index('D_snow')]
    assert request.series_ids('predictive_series', 'Q_cumecs', AMONG)[:2] == (['Q_cumecs'], [abi.TQ_DERIVED])    # a bare string
    assert request.series_ids('time_quantile_series', ['Q_cumecs', 'Vg'], AMONG)[2] == ['Qr', 'Msus_kg/day', 'TDP_kg/day', 'PP_kg/day', 'Vg']
    assert request.series_ids('time_quantile_series', ['Vg', 'Vr'], AMONG)[2] == ['Vg', 'Vr']


def test_series_ids_refuse():
    with pytest.raises(ValueError) as exc:
        request.series_ids('time_quantile_series', ['Q_cumecs', 'Q_litres', 'Qr', 'nope'], AMONG)
    assert str(exc.value) == "time_quantile_series must be 1 to 32 names among %s (unknown: ['Q_litres', 'nope'])" % AMONG
    refused('1 to 32', request.series_ids, 'predictive_series', [], AMONG)
    refused('1 to 32', request.series_ids, 'predictive_series', ['Qr'] * 33, AMONG)
    assert len(request.series_ids('predictive_series', ['Qr'] * 32, AMONG)[1]) == 32
    # a caller that allows fewer columns: the rest of the table's are unknown to it
    refused("unknown: \\['Vr'\\]", request.series_ids, 'forecast_series', ['Qr', 'Vr'], 'a and b', marshal.FLUX_COLUMNS)


# ---- periods ------------------------------------------------------------------------------------------------------------

def test_annual_periods_over_two_calendar_years():
    index = pd.date_range('2003-12-30', '2004-01-02')
    years, pod = request.annual_periods(index)
    assert list(years) == [2003, 2004] and pod.dtype == np.int32 and list(pod) == [0, 0, 1, 1]
    for got in (request.reduce_periods('annual', index), request.reduce_periods('annual', index, total=True)):
        assert list(got[0]) == [2003, 2004] and list(got[1]) == [0, 0, 1, 1]


def test_reduce_periods():
    index = pd.date_range('2004-01-01', periods=5)
    periods, pod = request.reduce_periods([0, 0, 2, 2, 1], index)
    assert list(periods) == [0, 1, 2] and pod.dtype == np.int32 and list(pod) == [0, 0, 2, 2, 1] and pod.flags.c_contiguous
    periods, pod = request.reduce_periods('total', index, total=True)
    assert list(periods) == [0] and list(pod) == [0] * 5 and pod.dtype == np.int32
    refused("reduce must be None, 'annual' or an array", request.reduce_periods, 'total', index)
    refused("reduce must be 'annual', 'total' or an array", request.reduce_periods, 'monthly', index, total=True)
    refused('one non-negative period index per day', request.reduce_periods, [0, 0, 1], index)
    refused('one non-negative period index per day', request.reduce_periods, [0, 0, -1, 1, 1], index)


def test_skipping_periods():
    assert request.skipping_periods('time_quantile_periods', None) == (None, None)
    assert request.skipping_periods('time_quantile_periods', 'annual') == (None, None)
    labels, pod = request.skipping_periods('time_quantile_periods', np.array([-1, 0, 0, -1, 2, -1]))
    assert list(labels) == [0, 1, 2] and pod.dtype == np.int32 and list(pod) == [-1, 0, 0, -1, 2, -1]
    labels, pod = request.skipping_periods('time_quantile_periods', np.array([-1, -1]))       # a run without a season
    assert list(labels) == [0] and list(pod) == [-1, -1]
    refused('must not decrease', request.skipping_periods, 'time_quantile_periods', np.array([0, 1, -1, 0]))
    for bad in ('monthly', np.array([0.0, 1.0]), np.array([[0, 1]]), np.array([0, -2])):
        refused("time_quantile_periods must be None, 'annual' or an int array", request.skipping_periods, 'time_quantile_periods', bad)


# ---- observed series, error-model rows ----------------------------------------------------------------------------------

def test_observed_series_with_and_without_a_restriction():
    index = pd.date_range('2004-01-01', periods=4)
    frame = pd.DataFrame({'Q': [1.0, np.nan, 3.0, np.nan], 'TDP': [np.nan, 0.02, np.nan, np.nan], 'PP': [np.nan] * 4}, index=index)
    obs_dict = {1: frame, 7: frame * 2}                                         # reach 7 is no output reach
    obs = sp.visualise_results.observation_array(obs_dict, [1], index)          # [n_reaches, 6, D]
    names, ids, sc_obs = request.observed_series(obs_dict, [1], obs)
    assert names == ['Q_cumecs', 'TDP_mgl']                                      # PP has a column and no value
    assert ids == [abi.TQ_DERIVED + abi.TQ_DERIVED_SERIES.index(c) for c in names]
    assert sc_obs.shape == (2, 4, 1) and sc_obs.flags.c_contiguous
    assert np.array_equal(sc_obs[0, :, 0], frame['Q'].to_numpy(), equal_nan=True)
    assert np.array_equal(sc_obs[1, :, 0], frame['TDP'].to_numpy(), equal_nan=True)
    names, ids, sc_obs = request.observed_series(obs_dict, [1], obs, among=['TDP_mgl', 'Qr', 'SS_mgl'])     # predictive_series
    assert names == ['TDP_mgl'] and ids == [abi.TQ_DERIVED + abi.TQ_DERIVED_SERIES.index('TDP_mgl')] and sc_obs.shape == (1, 4, 1)
    assert request.observed_series(obs_dict, [1], obs, among=['SS_mgl']) == ([], None, None)
    assert request.observed_series({7: frame}, [1], obs) == ([], None, None)


def test_error_model_rows():
    names = ['Q_cumecs', 'TDP_mgl']
    assert np.array_equal(request.error_model_rows(0.1, names, 3), np.full((2, 3), 0.1))
    assert np.array_equal(request.error_model_rows([0.1, 0.2, 0.0], names, 3), np.array([[0.1, 0.2, 0.0]] * 2))
    rows = request.error_model_rows({'TDP_mgl': [0.1, 0.2, 0.3]}, names, 3)     # a name the dict lacks gets 0
    assert np.array_equal(rows, np.array([[0.0, 0.0, 0.0], [0.1, 0.2, 0.3]])) and rows.flags.c_contiguous and rows.dtype == np.float64


@pytest.mark.parametrize('m', [-0.1, np.nan, np.inf, [0.1, 0.2, -1e-300], [0.1, 0.2], {'Q_cumecs': np.nan},
                               {'TDP_mgl': [0.1, np.inf, 0.1]}, 'much'])
def test_error_model_rows_refuse(m):
    """The refused forms of tests/test_predictive_host.py."""
    refused('predictive_m', request.error_model_rows, m, ['Q_cumecs', 'TDP_mgl'], 3)


# ---- the reference's in-place edits ---------------------------------------------------------------------------------------

@pytest.fixture
def no_device(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(engine, 'get_engine', touched)
    monkeypatch.setattr(engine, 'pinned_empty', touched)


def completed():
    """(p_LU, p_SC) as a completed call leaves them."""
    _, _, p_SU, p_LU, p_SC, p, _ = helpers.scenario_inputs(NAME)
    marshal.prologue(p_SU, p_LU, p_SC, p)
    marshal.epilogue_mutations(p_SU, p_LU, p_SC, p)
    return p_LU, p_SC


def ensemble_call(inputs):
    sp.run_simply_p_ensemble(*inputs, n_members=3, quantiles=[0.5], predictive_series=['Q_cumecs'], predictive_m=-0.1)


def sobol_call(inputs):
    sp.sobol_indices(*inputs, priors={'fc': (200.0, 380.0), 'd_maxE_spr': (20.0, 120.0)}, n_base=8)     # (30, 335) is allowed


def few_observations(inputs):
    """Observations in which Q has 10 values: the reference drops such a row (visualise_results.py:430)."""
    few = helpers.observations(inputs[2]['st_dt'], inputs[2]['end_dt'])
    few[1] = few[1].copy()
    few[1].loc[few[1].index[10:], 'Q'] = np.nan
    return few


def mcmc_call(inputs):
    sp.sample_posterior(*inputs, few_observations(inputs), priors={'fc': (200.0, 380.0), 'm_Q': (0.01, 1.0)}, n_walkers=4, n_steps=1)


def filter_call(inputs):
    sp.assimilate(*inputs, few_observations(inputs), priors={'fc': (200.0, 380.0), 'm_Q': (0.01, 1.0)}, n_particles=64)


@pytest.mark.parametrize('call,match', [(ensemble_call, 'predictive_m must be finite'), (sobol_call, 'model rejects'),
                                        (mcmc_call, '10 or fewer'), (filter_call, '10 or fewer')],
                         ids=['run_simply_p_ensemble', 'sobol_indices', 'sample_posterior', 'assimilate'])
def test_a_call_refused_after_its_prologue_leaves_what_a_completed_call_leaves(no_device, call, match):
    inputs = helpers.scenario_inputs(NAME)
    with pytest.raises(ValueError, match=match):
        call(inputs)
    want_LU, want_SC = completed()
    assert inputs[3].equals(want_LU) and inputs[4].equals(want_SC)
    assert not inputs[3].loc[['EPC0_0', 'Plab0'], ['A', 'S']].isna().any().any()          # the rows the prologue blanks are filled


@pytest.mark.parametrize('call', [ensemble_call, sobol_call, mcmc_call, filter_call, lambda inputs: sp.run_simply_p(*inputs)],
                         ids=['run_simply_p_ensemble', 'sobol_indices', 'sample_posterior', 'assimilate', 'run_simply_p'])
def test_a_prologue_that_raises_propagates(no_device, call):
    """Land-use shares that do not add to 1: the reference's own ValueError comes through, and no epilogue runs after it (the
    rows the prologue blanked stay blank)."""
    inputs = helpers.scenario_inputs(NAME)
    p_SC, p = inputs[4], inputs[5]
    p_SC.loc['f_S', marshal.sc_list(p)[0]] += 0.25
    with pytest.raises(ValueError, match='Land use proportions do not add to 1'):
        call(inputs)
    assert inputs[3].loc[['EPC0_0', 'Plab0', 'TDPs0']].isna().all().all()
