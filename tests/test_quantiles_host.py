"""Host side of the ensemble percentile bands (simplyp_quantiles): the exported symbol, the fields of its info struct,
the host interpolation between the two order statistics the device returns, the coverage count, and the refusal of a
multi-device split.  No GPU needed.

Tolerance of the interpolation against numpy: 4 * eps * max(|lo|, |hi|) absolute -- three roundings (the difference, the
product, the sum), each of a quantity of magnitude at most 2 max(|lo|, |hi|).  Nothing here is measured."""

import numpy as np
import pandas as pd
import pytest

import simplyp_amd as sp
from simplyp_amd import abi, engine, visualise_results as vr

EPS = np.finfo(np.float64).eps


def brackets(x, q):
    """What the device returns, made with np.sort: x [..., n] -> lower, upper [K, ...]."""
    s = np.sort(x, axis=-1)
    n = x.shape[-1]
    h = np.asarray(q, dtype=np.float64) * np.float64(n - 1)
    k_lo = np.floor(h).astype(np.int64)
    k_hi = np.minimum(k_lo + 1, n - 1)
    return np.stack([s[..., k] for k in k_lo]), np.stack([s[..., k] for k in k_hi])


def within_bound(got, want, lower, upper):
    tol = 4 * EPS * np.maximum(np.abs(lower), np.abs(upper))
    return bool((np.abs(got - want) <= tol).all())


def test_library_exports_the_entry():
    engine.build()
    assert 'simplyp_quantiles' in engine.ABI_SYMBOLS
    assert hasattr(engine.lib(), 'simplyp_quantiles')
    assert [f for f, _ in abi.QuantileInfo._fields_] == ['kernel_ms', 'bytes_table', 'n_used', 'n_passes']


@pytest.mark.parametrize('n', [1, 2, 3, 64, 100, 4097])
def test_interpolation_equals_numpy(n):
    rng = np.random.default_rng(n)
    q = np.concatenate([[0.0, 0.025, 0.5, 0.975, 1.0], rng.uniform(0, 1, 11)])
    for x in (rng.normal(size=(3, 17, n)) * 10.0 ** rng.integers(-8, 9, size=(3, 17, 1)),       # mixed signs and scales
              rng.choice([-2.5, 0.0, 1.0, 1.0 + EPS, 7e9], size=(3, 17, n)),                  # heavy ties
              np.abs(rng.normal(size=(3, 17, n))) + 5.0):                                      # a positive, narrow band
        lower, upper = brackets(x, q)
        got = engine.interpolate_quantiles(lower, upper, q, n)
        want = np.quantile(x, q, axis=-1)
        assert got.shape == want.shape == (len(q), 3, 17)
        assert within_bound(got, want, lower, upper)


def test_interpolation_equals_the_notebooks_describe():
    """The reference's own call (MCMC.ipynb cell 11): frame of days x members, .T.describe(percentiles=...)."""
    rng = np.random.default_rng(11)
    q = [0.025, 0.5, 0.975]
    days, members = 40, 101
    frame = pd.DataFrame(np.exp(rng.normal(size=(days, members))), index=pd.date_range('2004-01-01', periods=days))
    want = frame.T.describe(percentiles=q).T[['2.5%', '50%', '97.5%']].to_numpy().T
    lower, upper = brackets(frame.to_numpy(), q)
    got = engine.interpolate_quantiles(lower, upper, q, members)
    assert within_bound(got, want, lower, upper)


def test_no_member_gives_nan():
    got = engine.interpolate_quantiles(np.full((2, 5), np.nan), np.full((2, 5), np.nan), [0.1, 0.9], 0)
    assert got.shape == (2, 5) and np.isnan(got).all()


def test_band_coverage_with_gaps():
    lo = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    hi = np.array([2.0, 2.0, 2.0, 2.0, 2.0, 2.0])
    obs = np.array([1.5, np.nan, 2.0, 0.9, np.nan, 1.0])          # 4 observations: inside, on the upper end, below, on the lower end
    assert vr.band_coverage(lo, hi, obs) == 3 / 4
    # without gaps it is the notebook's sum / len
    obs2 = np.array([1.5, 3.0, 2.0, 0.9, 1.2, 1.0])
    assert vr.band_coverage(lo, hi, obs2) == ((obs2 >= lo) & (obs2 <= hi)).sum() / float(len(obs2)) == 4 / 6
    # leading axes broadcast; a series without observations gives NaN
    both = vr.band_coverage(lo, hi, np.stack([obs, np.full(6, np.nan)]))
    assert both.shape == (2,) and both[0] == 0.75 and np.isnan(both[1])


def test_devices_with_quantiles_is_refused_before_any_device_is_touched(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the call touched the device layer")
    monkeypatch.setattr(engine, 'get_engine', no_device)
    monkeypatch.setattr(engine, 'pinned_empty', no_device)
    with pytest.raises(ValueError, match='not a function of the member blocks'):
        sp.run_simply_p_ensemble(None, None, None, None, None, None, None, devices=[0, 0], quantiles=[0.5])
