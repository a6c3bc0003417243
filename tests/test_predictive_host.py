"""The random stream behind the predictive bands, on the CPU (simplyp_amd/predictive.py, the NumPy mirror of
csrc/simplyp_predictive.hip.h): Philox4x32-10 against known answers, the moments of the normals the stream's rule gives, the
error model's order of operations, and the argument checks of the public call that need no device.

Bounds of the moment tests: five standard errors of each statistic for n independent standard normals -- mean 1/sqrt(n),
variance sqrt(2/n), a tail share p sqrt(p (1 - p)/n), a correlation 1/sqrt(n)."""

import numpy as np
import pytest

import helpers
import simplyp_amd as sp
from simplyp_amd import abi, predictive


def words(*xs):
    return tuple(np.uint32(x) for x in xs)


@pytest.mark.parametrize('counter,key,want', [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(counter, key, want):
    got = predictive.philox4x32_10(counter, key)
    assert tuple(int(x) for x in got) == want
    # the same through arrays: every element is its own counter
    c = [np.full(5, x, dtype=np.uint32) for x in counter]
    got = predictive.philox4x32_10(c, key)
    assert all(g.dtype == np.uint32 and g.shape == (5,) and (g == w).all() for g, w in zip(got, want))


def test_uniforms_are_exact_and_open():
    """u = (h + 0.5) 2^-52 with h < 2^52: 2^53 u is an odd integer (nothing was rounded), and 0 < u < 1."""
    u1, u2 = predictive.uniforms(5, np.arange(4096), 3, 1, 64)
    for u in (u1, u2):
        t = u * 2.0 ** 53
        assert (t == np.floor(t)).all() and (t % 2 == 1).all()
        assert (u > 0).all() and (u < 1).all()
    # the rule's extremes: all-zero and all-one words
    zero, ones = np.zeros(1, np.uint32), np.full(1, 0xffffffff, np.uint32)
    assert predictive._uniform(zero, zero)[0] == 2.0 ** -53
    assert predictive._uniform(ones, ones)[0] == 1.0 - 2.0 ** -53
    assert np.sqrt(-2.0 * np.log(2.0 ** -53)) <= 8.58


def test_key_is_the_seed_split_in_two():
    m, d = np.arange(7), 11
    x = predictive.philox4x32_10((m, d, 2, 64), (5, 7))
    u1, u2 = predictive.uniforms((7 << 32) | 5, m, d, 2, 64)
    assert (u1 == predictive._uniform(x[0], x[1])).all() and (u2 == predictive._uniform(x[2], x[3])).all()
    assert not (predictive.uniforms(5, m, d, 2, 64)[0] == u1).any()


@pytest.mark.parametrize('seed', [0, 1, 20260101])
def test_moments_of_the_normals(seed):
    z = predictive.standard_normal(seed, np.arange(1024)[:, None], np.arange(1024)[None, :], 0, abi.TQ_DERIVED)
    n = z.size
    assert n == 1 << 20 and np.isfinite(z).all() and np.abs(z).max() <= 8.58
    assert abs(z.mean()) < 5 / np.sqrt(n)
    assert abs(z.var() - 1) < 5 * np.sqrt(2 / n)
    assert abs((np.abs(z) > 1.96).mean() - 0.05) < 5 * np.sqrt(.05 * .95 / n)
    assert abs(np.corrcoef(z[1:].ravel(), z[:-1].ravel())[0, 1]) < 5 / np.sqrt(n)          # along the members
    assert abs(np.corrcoef(z[:, 1:].ravel(), z[:, :-1].ravel())[0, 1]) < 5 / np.sqrt(n)    # along the days


def test_every_index_and_the_seed_enter():
    base = dict(seed=9, member=np.arange(64), day=100, reach=1, series=5)
    z = predictive.standard_normal(**base)
    for k, v in (('seed', 10), ('seed', 9 + (1 << 32)), ('day', 101), ('reach', 2), ('series', 6), ('series', abi.TQ_DERIVED + 5)):
        assert not (predictive.standard_normal(**dict(base, **{k: v})) == z).any(), k
    assert (predictive.standard_normal(**dict(base, member=np.arange(64)[::-1]))[::-1] == z).all()


def test_cospi_reduces_its_argument_exactly():
    t = np.array([0.5, 1.0, 1.5, 0.25, 2.0 ** -52, 2.0 - 2.0 ** -52])
    want = np.array([0.0, -1.0, 0.0, np.sqrt(0.5), 1.0, 1.0])
    got = predictive._cospi(t)
    assert (got[:3] == want[:3]).all() and np.abs(got - want).max() <= 2.0 ** -52
    u = np.random.default_rng(0).uniform(0, 2, 100000)
    assert np.abs(predictive._cospi(u) - np.cos(np.pi * u)).max() < 2e-15


def test_perturb_is_two_multiplies_and_an_add():
    rng = np.random.default_rng(1)
    v, m, z = rng.lognormal(size=1000), rng.uniform(0, 0.5, 1000), rng.normal(size=1000)
    got = predictive.perturb(v, m, z)
    assert (got == v + (m * v) * z).all()
    assert (predictive.perturb(v, 0.0, z) == v).all()
    sp_ = predictive.perturb(np.array([np.nan, 0.0, -2.0, np.inf, np.inf]), 0.5, np.array([1.0, 1.0, 1.0, 1.0, -1.0]))
    assert np.isnan(sp_[0]) and sp_[1] == 0.0 and sp_[2] == -3.0 and sp_[3] == np.inf and np.isnan(sp_[4])


# ---- the public call's argument checks: none of them needs a device ---------------------------------------------------------

def refused(match, **kw):
    with pytest.raises(ValueError, match=match):
        sp.run_simply_p_ensemble(None, None, None, None, None, None, None, **kw)


def test_public_call_refuses_before_touching_anything():
    q = [0.025, 0.5, 0.975]
    refused('needs quantiles', predictive_series=['Q_cumecs'])
    refused('without predictive_series', predictive_m=0.1, quantiles=q)
    refused('reduce', predictive_series=['Q_cumecs'], quantiles=q, reduce='annual')
    refused('devices', predictive_series=['Q_cumecs'], quantiles=q, devices=[0, 1])
    refused('unknown', predictive_series=['Q_cumecs', 'Q_litres'], quantiles=q)
    refused('1 to 32', predictive_series=[], quantiles=q)
    refused('1 to 32', predictive_series=['Qr'] * 33, quantiles=q)
    refused('does not', predictive_series=['Q_cumecs'], predictive_m={'TDP_mgl': 0.1}, quantiles=q)
    refused('predictive_seed', predictive_series=['Q_cumecs'], quantiles=q, predictive_seed=-1)
    refused('predictive_seed', predictive_series=['Q_cumecs'], quantiles=q, predictive_seed=1 << 64)
    refused('predictive_day0', predictive_series=['Q_cumecs'], quantiles=q, predictive_day0=-1)


@pytest.mark.parametrize('m', [-0.1, np.nan, np.inf, [0.1, 0.2, -1e-300], [0.1, 0.2], {'Q_cumecs': np.nan},
                               {'TDP_mgl': [0.1, np.inf, 0.1]}, 'much'])
def test_public_call_refuses_a_bad_error_model(m):
    """predictive_m is checked on the host, once the ensemble's size is known and before anything is allocated."""
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs('tarland_2004_dynamic')
    with pytest.raises(ValueError, match='predictive_m'):
        sp.run_simply_p_ensemble(met, p_struc, p_SU, p_LU, p_SC, p, dyn, n_members=3, quantiles=[0.5],
                                 predictive_series=['Q_cumecs', 'TDP_mgl'], predictive_m=m)
