"""simplyp_amd/residuals.py -- the NumPy statement of the lag-one sums and of the AR(1) heteroscedastic log-likelihood -- against
a brute-force double loop, against the dense multivariate normal it factorises, and against the independent likelihood at
phi = 0; and what the calibration calls refuse before they touch a device."""

import math

import numpy as np
import pytest
import scipy.stats

import simplyp_amd as sp
from simplyp_amd import abi, calibrate, residuals
from oracle import gof as ogof

NAN = float('nan')


def brute_lag_sums(obs, sim):
    """The link rule, row by row."""
    n_link, A, B, C = 0, [], [], []
    for t in range(1, len(obs)):
        if any(x != x for x in (obs[t], sim[t], obs[t - 1], sim[t - 1])):
            continue
        r1, r0 = obs[t] / sim[t] - 1.0, obs[t - 1] / sim[t - 1] - 1.0
        n_link += 1
        A.append(r1 * r1); B.append(r0 * r0); C.append(r1 * r0)
    return float(n_link), math.fsum(A), math.fsum(B), math.fsum(C)


def patterned(rng, D, observed, sim_nan=()):
    sim = rng.uniform(0.5, 3.0, D)
    obs = np.full(D, NAN)
    observed = np.asarray(observed)
    obs[observed] = sim[observed] * rng.uniform(0.6, 1.5, len(observed))
    sim[list(sim_nan)] = NAN
    return obs, sim


PATTERNS = {
    'gaps and an isolated day': (30, [2, 3, 4, 8, 11, 12, 13, 14, 20, 25, 26], ()),
    'a segment at row 0': (20, [0, 1, 2, 3, 9, 10], ()),
    'a segment ending at row D - 1': (20, [4, 5, 15, 16, 17, 18, 19], ()),
    'every day': (25, list(range(25)), ()),
    'a NaN simulated value inside a segment': (30, list(range(5, 21)), (12,)),
    'NaN simulated values at both ends and side by side': (16, list(range(16)), (0, 7, 8, 15)),
    'no link at all': (12, [1, 3, 5, 7, 9, 11], ()),
}


@pytest.mark.parametrize('name', list(PATTERNS))
def test_lag_sums_equal_a_double_loop(name):
    D, observed, sim_nan = PATTERNS[name]
    rng = np.random.default_rng(len(name))
    obs, sim = patterned(rng, D, observed, sim_nan)
    want = brute_lag_sums(obs, sim)
    got = residuals.lag_sums(obs, sim)
    assert got[0] == want[0], name
    for g, w in zip(got[1:], want[1:]):
        assert abs(g - w) <= 4 * want[0] * 2.0 ** -53 * max(abs(w), 1.0), (name, g, w)
    if name == 'no link at all':
        assert got == (0.0, 0.0, 0.0, 0.0) and np.isnan(residuals.phi_hat(got[2], got[3]))
    if name == 'a NaN simulated value inside a segment':           # 16 observed days in a row, one lost: two links go with it
        assert got[0] == 15 - 2


def test_lag_sums_keep_the_member_axis_and_break_links_per_member():
    rng = np.random.default_rng(5)
    D, E = 40, 7
    obs = np.full(D, NAN)
    days = np.r_[0:9, 12:30, 33]
    obs[days] = rng.uniform(0.5, 2.0, len(days))
    sim = rng.uniform(0.5, 3.0, (D, E))
    sim[4, 2] = sim[12, 3] = sim[20, 3] = sim[21, 3] = NAN
    got = residuals.lag_sums(obs, sim)
    assert all(g.shape == (E,) for g in got)
    for e in range(E):
        want = brute_lag_sums(obs, sim[:, e])
        assert got[0][e] == want[0]
        assert np.allclose([g[e] for g in got[1:]], want[1:], rtol=1e-13, atol=0.0)
    assert got[0][0] == 8 + 17 and got[0][2] == got[0][0] - 2 and got[0][3] == got[0][0] - 1 - 3
    assert np.allclose(residuals.phi_hat(got[2], got[3]), got[3] / got[2])


@pytest.mark.parametrize('phi', [-0.9, 0.3, 0.7, 0.99])
def test_loglik_ar1_is_the_dense_multivariate_normal(phi):
    """40 days with gaps, an isolated day and segments at both ends: the covariance is phi^|a - b| m sim_a m sim_b inside a run of
    consecutive observed days and 0 across runs.  Tolerance: cond(cov) n 2^-52 relative -- what the dense factorisation can lose."""
    rng = np.random.default_rng(40)
    D, m = 40, 0.2
    observed = np.r_[0:6, 9:10, 13:25, 27:29, 33:40]
    obs, sim = patterned(rng, D, observed)
    sim[17] = NAN                                                    # a missing simulated value splits a run
    paired = np.flatnonzero(~np.isnan(obs) & ~np.isnan(sim))
    n = len(paired)
    cov = np.zeros((n, n))
    for a in range(n):
        for b in range(n):
            lo, hi = sorted((paired[a], paired[b]))
            if all(d in paired for d in range(lo, hi + 1)):
                cov[a, b] = phi ** (hi - lo) * (m * sim[paired[a]]) * (m * sim[paired[b]])
    want = scipy.stats.multivariate_normal(mean=sim[paired], cov=cov).logpdf(obs[paired])
    r = obs[paired] / sim[paired] - 1.0
    n_link, A, B, C = residuals.lag_sums(obs, sim)
    got = residuals.loglik_ar1(float(n), np.log(sim[paired]).sum(), (r * r).sum(), n_link, A, B, C, m, phi)
    tol = np.linalg.cond(cov) * n * 2.0 ** -52
    print('phi = %g: n = %d, n_link = %d, cond = %.3e, relative difference %.3e (tolerance %.3e)'
          % (phi, n, n_link, np.linalg.cond(cov), abs(got / want - 1.0), tol))
    assert n_link == 5 + 3 + 6 + 1 + 6 and abs(got - want) <= tol * abs(want)


def test_loglik_ar1_at_phi_zero_is_the_independent_likelihood_bit_for_bit():
    rng = np.random.default_rng(8)
    K = 500
    n = rng.integers(11, 5000, K).astype(np.float64)
    row = np.zeros((8, K))
    row[0], row[6], row[7] = n, rng.normal(0.0, 3.0, K) * n, rng.uniform(0.001, 2.0, K) * n
    n_link = np.floor(n * rng.uniform(0.0, 1.0, K))
    A, B, C = rng.uniform(0.0, 1.0, (3, K)) * row[7]
    C *= rng.choice([-1.0, 1.0], K)
    m = rng.uniform(0.01, 2.0, K)
    want = ogof.loglik(row, m)
    for phi in (0.0, -0.0, np.zeros(K)):
        got = residuals.loglik_ar1(row[0], row[6], row[7], n_link, A, B, C, m, phi)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert not np.array_equal(residuals.loglik_ar1(row[0], row[6], row[7], n_link, A, B, C, m, 0.5), want)


def test_the_maximum_over_phi_lies_at_about_phi_hat():
    """C / B maximises the conditional likelihood: the full one (with the stationary first days) peaks next to it on a long record."""
    rng = np.random.default_rng(3)
    D, phi0, m = 4000, 0.6, 0.3
    eta = np.empty(D)
    eta[0] = rng.normal()
    for t in range(1, D):
        eta[t] = phi0 * eta[t - 1] + math.sqrt(1 - phi0 * phi0) * rng.normal()
    sim = rng.uniform(0.5, 3.0, D)
    obs = sim * (1.0 + m * eta)
    r = obs / sim - 1.0
    n_link, A, B, C = residuals.lag_sums(obs, sim)
    ph = residuals.phi_hat(B, C)
    grid = np.linspace(-0.95, 0.95, 381)
    ll = residuals.loglik_ar1(float(D), np.log(sim).sum(), (r * r).sum(), n_link, A, B, C, m, grid)
    assert n_link == D - 1 and abs(ph - phi0) < 0.05 and abs(grid[np.argmax(ll)] - ph) < 0.02


# ---- the extension header and its binding -----------------------------------------------------------------------------------

def test_the_extension_header_declares_the_two_entries_and_the_library_exports_them():
    import ctypes as C
    import os
    import re
    import subprocess
    import tempfile
    from simplyp_amd import engine
    path = os.path.join(engine.INCLUDE, 'simplyp_residuals.h')
    with open(path) as fh:
        text = fh.read()
    assert set(re.findall(r'\b(simplyp_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', ' ', text, flags=re.S))) =={'simplyp_gof_lag', 'simplyp_mcmc_log_prob_ar1'}
    assert engine.RESIDUALS_SYMBOLS == ['simplyp_gof_lag', 'simplyp_mcmc_log_prob_ar1']
    assert not set(engine.RESIDUALS_SYMBOLS) & set(engine.ABI_SYMBOLS)
    vp, i32 = C.c_void_p, C.c_int32
    proto = {name: (restype, argtypes) for name, restype, argtypes in engine.RESIDUALS_PROTOTYPES}
    assert proto['simplyp_gof_lag'] == (C.c_int, [vp, C.POINTER(abi.Dims), C.c_uint32, vp, i32] + [vp] * 6 + [C.POINTER(abi.GofInfo)])
    assert proto['simplyp_mcmc_log_prob_ar1'] == (C.c_int, [vp, i32, i32, i32] + [vp] * 6 + [i32] + [vp] * 6 + [C.POINTER(abi.McmcInfo)])
    engine.build()
    L = engine.lib()
    for name, (restype, argtypes) in proto.items():
        assert getattr(L, name).restype is restype and list(getattr(L, name).argtypes) == argtypes, name
    # the header stands on its own in C, and its rows are abi.LAG_STATS in order
    rows = ['SIMPLYP_LAGSTAT_N_LINK', 'SIMPLYP_LAGSTAT_SQ_HEAD', 'SIMPLYP_LAGSTAT_SQ_TAIL', 'SIMPLYP_LAGSTAT_CROSS', 'SIMPLYP_N_LAG_STATS']
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, 'rows.c'), os.path.join(tmp, 'rows')
        with open(src, 'w') as fh:
            fh.write('#include <stdio.h>\n#include "%s"\nint main(void) { printf("%s\\n", %s); return 0; }\n'
                     % (path, ' '.join(['%d'] * len(rows)), ', '.join(rows)))
        subprocess.check_call(['gcc', '-Wall', '-Werror', '-o', exe, src])
        assert subprocess.check_output([exe], text=True).split() == ['0', '1', '2', '3', '4']
    assert [r[len('SIMPLYP_LAGSTAT_'):].lower() for r in rows[:4]] == abi.LAG_STATS


# ---- what the public calls refuse on the host -------------------------------------------------------------------------------

def plan(priors, variables=('Q',), error_m=None, error_phi=None):
    return calibrate._plan(priors, variables, error_m, lambda n_dim: None, error_phi)


def test_plan_wires_phi_like_m():
    out = plan({'fc': (200.0, 380.0), 'm_Q': (0.01, 1.0), 'phi_Q': (-0.5, 0.9), 'm_TDP': (0.01, 1.0)}, ('Q', 'TDP'), error_phi={'TDP': 0.25})
    names, variables, lo, hi, target, m_dim, m_const, phi = out
    q, tdp = abi.GOF_VARS.index('Q'), abi.GOF_VARS.index('TDP')
    assert names == ['fc', 'm_Q', 'phi_Q', 'm_TDP'] and list(target[1:]) == [abi.MCMC_TARGET_NONE] * 3
    assert (lo[2], hi[2]) == (-0.5, 0.9)
    phi_dim, phi_const, with_phi = phi
    assert phi_dim[q] == 2 and phi_dim[tdp] == -1 and phi_const[tdp] == 0.25 and with_phi == ['Q', 'TDP']
    assert [phi_const[v] for v in range(6) if v != tdp] == [0.0] * 5
    # without any phi the plan says so, and the rest is what it was
    assert plan({'fc': (200.0, 380.0), 'm_Q': (0.01, 1.0)})[-1] is None
    assert plan({'fc': (200.0, 380.0)}, error_m={'Q': 0.2}, error_phi={})[-1] is None
    assert plan({'fc': (200.0, 380.0)}, error_m={'Q': 0.2}, error_phi={'Q': 0.0})[-1] == ([-1] * 6, [0.0] * 6, ['Q'])


@pytest.mark.parametrize('kw, text', [
    (dict(priors={'m_Q': (0.01, 1.0), 'phi_Q': (-1.0, 0.5)}), r'box of phi_Q must lie inside \(-1, 1\)'),
    (dict(priors={'m_Q': (0.01, 1.0), 'phi_Q': (0.0, 1.0)}), r'box of phi_Q must lie inside \(-1, 1\)'),
    (dict(priors={'m_Q': (0.01, 1.0), 'phi_Q': (NAN, 0.5)}), r'box of phi_Q must lie inside \(-1, 1\)'),
    (dict(priors={'m_Q': (0.01, 1.0), 'phi_Q': (0.0, 0.5)}, error_phi={'Q': 0.6}), 'phi_Q is sampled and fixed through error_phi at once'),
    (dict(priors={'m_Q': (0.01, 1.0), 'phi_TDP': (0.0, 0.5)}), "phi_TDP: variable 'TDP' is not selected"),
    (dict(priors={'m_Q': (0.01, 1.0)}, error_phi={'TDP': 0.3}), 'error_phi names variables that are not selected'),
    (dict(priors={'m_Q': (0.01, 1.0)}, error_phi={'Q': 1.0}), r"error_phi\['Q'\] = 1.0 is not inside \(-1, 1\)"),
    (dict(priors={'m_Q': (0.01, 1.0)}, error_phi={'Q': NAN}), r'is not inside \(-1, 1\)'),
    (dict(priors={'m_Q': (0.01, 1.0), 'phi_X': (0.0, 0.5)}), "unknown parameter 'phi_X'"),
])
def test_plan_refusals(kw, text):
    with pytest.raises(ValueError, match=text):
        plan(**kw)


@pytest.mark.parametrize('call', ['sample_posterior', 'find_map'])
def test_the_public_calls_refuse_before_any_device_call(call):
    """The plan comes before the inputs are even looked at: placeholders do for them."""
    fn = getattr(sp, call)
    kw = dict(n_walkers=8) if call == 'sample_posterior' else dict(n_starts=2)
    with pytest.raises(ValueError, match='must lie inside'):
        fn(None, None, None, None, None, None, None, {1: 'observations'}, {'m_Q': (0.01, 1.0), 'phi_Q': (-0.5, 1.0)}, **kw)
    with pytest.raises(ValueError, match='sampled and fixed'):
        fn(None, None, None, None, None, None, None, {1: 'observations'}, {'m_Q': (0.01, 1.0), 'phi_Q': (-0.5, 0.5)},
           error_phi={'Q': 0.1}, **kw)
    with pytest.raises(ValueError, match='not selected'):
        fn(None, None, None, None, None, None, None, {1: 'observations'}, {'m_Q': (0.01, 1.0)}, error_phi={'SS': 0.1}, **kw)


def test_assimilate_takes_no_phi():
    for kw in (dict(priors={'m_Q': (0.01, 1.0), 'phi_Q': (-0.5, 0.5)}), dict(priors={'m_Q': (0.01, 1.0)}, error_phi={'Q': 0.3})):
        with pytest.raises(ValueError, match='assimilate takes no lag-one coefficient'):
            sp.assimilate(None, None, None, None, None, None, None, {1: 'observations'}, n_particles=8, **kw)


def test_residual_lag_needs_observations():
    with pytest.raises(ValueError, match='residual_lag needs obs_dict'):
        sp.run_simply_p_ensemble(None, None, None, None, None, None, None, residual_lag=True)
