"""Host side of the per-member quantiles over time (simplyp_time_quantiles): the exported symbol, the header's
constant and the fields of its info struct, the host interpolation between the two order statistics the device returns
(per-period day counts), and the refusals of run_simply_p_ensemble, which come before any device is touched.  No GPU needed.

The interpolation is compared with np.quantile(x, q, axis=0, method='linear') BIT FOR BIT: interpolate_quantiles forms
h = q (n - 1), gamma = h - floor(h) and the lerp exactly as numpy does, from the same two sorted elements."""

import numpy as np
import pytest

import simplyp_amd as sp
from simplyp_amd import abi, engine

from c_header import c_values


def brackets(x, q):
    """What the device returns for one period, made with np.sort: x [n, ...] -> lower, upper [K, ...]."""
    s = np.sort(x, axis=0)
    n = x.shape[0]
    h = np.asarray(q, dtype=np.float64) * np.float64(n - 1)
    k_lo = np.floor(h).astype(np.int64)
    k_hi = np.minimum(k_lo + 1, n - 1)
    return s[k_lo], s[k_hi]


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def test_library_exports_the_entry():
    engine.build()
    assert 'simplyp_time_quantiles' in engine.ABI_SYMBOLS
    assert hasattr(engine.lib(), 'simplyp_time_quantiles')
    assert c_values(['SIMPLYP_TQ_DERIVED'])['SIMPLYP_TQ_DERIVED'] == abi.TQ_DERIVED
    assert [f for f, _ in abi.TqInfo._fields_] == ['kernel_ms', 'bytes_read', 'n_sweeps', 'n_periods']
    assert abi.TQ_DERIVED == 64 and abi.TQ_DERIVED_SERIES == ['Q_cumecs', 'SS_mgl', 'TDP_mgl', 'PP_mgl', 'TP_mgl', 'SRP_mgl']


Q16 = np.concatenate([[0.0, 0.05, 0.5, 0.95, 1.0], np.random.default_rng(16).uniform(0, 1, 11)])


@pytest.mark.parametrize('n', [1, 2, 3, 10, 365, 366])
def test_interpolation_equals_numpy_bit_for_bit(n):
    rng = np.random.default_rng(n)
    x = np.exp(rng.normal(size=(n, 2, 1, 3, 7)))                            # [days, n_series, -, R, E]
    lower, upper = brackets(x, Q16)                                         # [K, n_series, 1, R, E]: one period
    got = engine.interpolate_time_quantiles(lower, upper, Q16, [n])
    want = np.quantile(x, Q16, axis=0, method='linear')
    assert got.shape == want.shape == (16, 2, 1, 3, 7)
    assert same_bits(got, want)


def test_interpolation_with_periods_of_different_lengths():
    rng = np.random.default_rng(7)
    lengths = [365, 366, 1, 90, 2]
    xs = [rng.normal(size=(n, 3, 2, 5)) * 10.0 ** rng.integers(-3, 4, size=(1, 3, 1, 1)) for n in lengths]
    lo, up = zip(*(brackets(x, Q16) for x in xs))                           # each [K, n_series, R, E]
    lower, upper = np.stack(lo, axis=2), np.stack(up, axis=2)               # [K, n_series, P, R, E]
    got = engine.interpolate_time_quantiles(lower, upper, Q16, lengths)
    for p, x in enumerate(xs):
        assert same_bits(got[:, :, p], np.quantile(x, Q16, axis=0, method='linear')), p


def test_period_without_days_gives_nan():
    rng = np.random.default_rng(9)
    x = rng.normal(size=(10, 1, 2, 4))
    lo, up = brackets(x, [0.1, 0.9])
    nan = np.full_like(lo, np.nan)
    got = engine.interpolate_time_quantiles(np.stack([lo, nan, lo], axis=2), np.stack([up, nan, up], axis=2), [0.1, 0.9], [10, 0, 10])
    assert np.isnan(got[:, :, 1]).all()
    want = np.quantile(x, [0.1, 0.9], axis=0, method='linear')
    assert same_bits(got[:, :, 0], want) and same_bits(got[:, :, 2], want)
    with pytest.raises(ValueError):
        engine.interpolate_time_quantiles(np.stack([lo, lo], axis=2), np.stack([up, up], axis=2), [0.1, 0.9], [10, 0, 10])


@pytest.fixture
def no_device(monkeypatch):
    def touched(*a, **k):
        raise AssertionError("the call touched the device layer")
    monkeypatch.setattr(engine, 'get_engine', touched)
    monkeypatch.setattr(engine, 'pinned_empty', touched)


def refused(match, **kw):
    with pytest.raises(ValueError, match=match):
        sp.run_simply_p_ensemble(None, None, None, None, None, None, None, **kw)


def test_time_quantiles_with_reduce_is_refused(no_device):
    refused('cannot be combined with reduce', time_quantiles=[0.5], reduce='annual')
    refused('cannot be combined with reduce', time_quantiles=[0.5], reduce=np.zeros(10, dtype=np.int32))


def test_bad_probabilities_are_refused(no_device):
    for q in ([-1e-9], [1.0 + 1e-9], [0.5, np.nan], [0.5] * 17, []):
        refused('1 to 16 probabilities', time_quantiles=q)


def test_unknown_series_is_refused(no_device):
    refused('Q_cumec', time_quantiles=[0.5], time_quantile_series=['Qr', 'Q_cumec'])
    refused('unknown', time_quantiles=[0.5], time_quantile_series=[])
    refused('unknown', time_quantiles=[0.5], outputs=['Qr', 'no_such_column'])       # the default: every column of outputs


def test_decreasing_periods_are_refused(no_device):
    refused('must not decrease', time_quantiles=[0.5], time_quantile_periods=np.array([0, 0, 1, -1, 0]))
    refused('period indices', time_quantiles=[0.5], time_quantile_periods=np.array([0, -2, 1]))
    refused('period indices', time_quantiles=[0.5], time_quantile_periods=np.array([0.0, 1.0]))
    refused('period indices', time_quantiles=[0.5], time_quantile_periods='monthly')


def test_series_or_periods_without_time_quantiles_are_refused(no_device):
    refused('without time_quantiles', time_quantile_series=['Qr'])
    refused('without time_quantiles', time_quantile_periods='annual')
    refused('without time_quantiles', time_quantile_periods=np.zeros(5, dtype=np.int32))
