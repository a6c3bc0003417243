"""The NumPy statement of the Sobol' estimator (simplyp_amd/sobol.py) against scipy and against itself, and the host checks of the
public call.  No GPU."""

import numpy as np
import pytest
import scipy.stats
from scipy.stats._sensitivity_analysis import saltelli_2010

import helpers
import simplyp_amd as sp
from simplyp_amd import abi, engine, sobol

NAME = 'tarland_2004_dynamic'
LO, HI = np.full(3, -np.pi), np.full(3, np.pi)
ANALYTIC_S1 = np.array([0.3139, 0.4424, 0.0])
ANALYTIC_ST = np.array([0.5576, 0.4424, 0.2437])
SEED = 1                    # the design and bootstrap key the analytic test fixes


def ishigami(x, offset=100.0):
    """Ishigami with a = 7, b = 0.1, shifted so that the centring matters."""
    return np.sin(x[0]) + 7.0 * np.sin(x[1]) ** 2 + 0.1 * x[2] ** 4 * np.sin(x[0]) + offset


def blocks(f, N, d):
    return f[:N], f[N:2 * N], f[2 * N:].reshape(d, N)


def index_bounds(terms, n, var, d):
    """The summation bound of every index, N 2^-53 sum |term| / (n var), times 4 for the operations of the ratio: [2, d]."""
    N = terms.shape[0]
    g, t = np.abs(terms[:, 2:2 + d]).sum(axis=0), 0.5 * np.abs(terms[:, 2 + d:]).sum(axis=0)
    return 4.0 * N * 2.0 ** -53 * np.stack([g, t]) / (n * var)


@pytest.mark.parametrize('N', [4096, 7])
def test_point_estimate_is_scipys(N):
    f = ishigami(sobol.design(N, LO, HI, seed=SEED))
    fa, fb, fab = blocks(f, N, 3)
    if N & (N - 1) == 0:
        ref = scipy.stats.sobol_indices(func={'f_A': fa[None], 'f_B': fb[None], 'f_AB': fab[:, None, :]}, n=N)
        s1, st = ref.first_order.ravel(), ref.total_order.ravel()
    else:
        # the public call refuses an n that is no power of two; this is what it does after that check (sobol_indices, _sensitivity_analysis.py)
        mean = np.mean([fa, fb])
        s1, st = (v.ravel() for v in saltelli_2010((fa - mean)[None], (fb - mean)[None], (fab - mean)[:, None, :]))
    got = sobol.sobol_indices(f[None], N, 3)
    terms, _ = sobol.row_terms(f[None], N, 3, np.ones(N, dtype=bool))
    bound = index_bounds(terms[0], N, got['var'][0, 0], 3)
    err = np.abs(got['indices'][:, :, 0, 0] - np.stack([s1, st]))
    print('N = %d: max error %.3e, smallest bound %.3e' % (N, err.max(), bound.min()))
    assert bound.max() < 2e-12 and (err <= bound).all(), (err, bound)
    assert got['n_used'][0] == N and got['indices'].shape == (2, 3, 1, 1)


def test_counts_form_is_the_gather_form():
    N, d, n_boot = 257, 3, 8
    f = ishigami(sobol.design(N, LO, HI, seed=5))
    fa, fb, fab = blocks(f, N, d)
    mean = np.mean([fa, fb])
    a, b, ab = fa - mean, fb - mean, fab - mean
    got = sobol.sobol_indices(f[None], N, d, n_boot=n_boot, seed=9)
    assert (got['counts'].sum(axis=1) == N).all() and (got['counts'][0] == 1).all() and (got['n_used'] == N).all()
    idx = sobol.boot_indices(9, n_boot, N)
    assert idx.shape == (n_boot, N) and idx.min() >= 0 and idx.max() < N
    terms, _ = sobol.row_terms(f[None], N, d, np.ones(N, dtype=bool))
    for k in range(n_boot):
        ra, rb, rab = a[idx[k]], b[idx[k]], ab[:, idx[k]]
        var = np.var([ra, rb])
        s1 = np.mean(rb * (rab - ra), axis=-1) / var
        st = 0.5 * np.mean((ra - rab) ** 2, axis=-1) / var
        c = got['counts'][1 + k]
        bound = index_bounds(terms[0] * c[:, None], N, var, d)
        err = np.abs(got['indices'][:, :, 0, 1 + k] - np.stack([s1, st]))
        assert (err <= bound).all(), (k, err, bound)
    assert len({tuple(c) for c in got['counts']}) == 1 + n_boot


def test_design_blocks_box_and_unit_samples():
    N, d = 11, 4
    lo, hi = np.array([0.0, -3.0, 10.0, 1e-3]), np.array([1.0, 5.0, 10.5, 2e-3])
    u = sobol.unit_points(3, N, d)
    assert u.shape == (2, d, N) and (u > 0).all() and (u < 1).all() and len(np.unique(u)) == u.size
    x = sobol.design(N, lo, hi, seed=3)
    assert x.shape == (d, N * (d + 2)) and (x >= lo[:, None]).all() and (x <= hi[:, None]).all()
    A, B = x[:, :N], x[:, N:2 * N]
    assert np.array_equal(A, lo[:, None] + (hi - lo)[:, None] * u[0]) and np.array_equal(B, lo[:, None] + (hi - lo)[:, None] * u[1])
    for i in range(d):
        AB = x[:, (2 + i) * N:(3 + i) * N]
        rest = [k for k in range(d) if k != i]
        assert np.array_equal(AB[i], B[i]) and np.array_equal(AB[rest], A[rest]) and not np.array_equal(AB[i], A[i])
    assert not np.array_equal(x, sobol.design(N, lo, hi, seed=4))
    own = np.random.default_rng(0).random((2, d, N))
    xo = sobol.design(N, lo, hi, seed=3, unit=own)
    assert np.array_equal(xo[:, :N], lo[:, None] + (hi - lo)[:, None] * own[0]) and np.array_equal(xo[2, 4 * N:5 * N], xo[2, N:2 * N])
    for bad in (own[:, :, :-1], np.where(own > 0.9, 1.0, own), -own):
        with pytest.raises(ValueError, match='unit_samples'):
            sobol.design(N, lo, hi, unit=bad)


def test_invalid_samples_are_compacted_away():
    N, d = 40, 3
    f = ishigami(sobol.design(N, LO, HI, seed=2))
    status = np.zeros(N * (d + 2), dtype=np.int32)
    status[0 * N + 5] = abi.STATUS_NONFINITE                       # an A member, a B member, an AB member: three samples
    status[1 * N + 17] = abi.STATUS_NONFINITE | abi.STATUS_STEPCAP
    status[3 * N + 39] = abi.STATUS_NONFINITE
    status[2 * N + 8] = abi.STATUS_STEPCAP                         # a step cap alone does not invalidate
    dirty = f.copy()
    dirty[[5, N + 17, 3 * N + 39]] = np.nan
    valid = sobol.valid_samples(status, N, d)
    assert valid.sum() == N - 3 and not valid[[5, 17, 39]].any()
    got = sobol.sobol_indices(dirty[None], N, d, status=status)
    compact = f.reshape(d + 2, N)[:, valid].ravel()
    want = sobol.sobol_indices(compact[None], N - 3, d)
    assert got['n_used'][0] == N - 3 and np.isfinite(got['sums']).all()
    assert np.array_equal(got['sums'], want['sums']) and np.array_equal(got['indices'], want['indices'])
    boot = sobol.sobol_indices(dirty[None], N, d, status=status, n_boot=5, seed=1)
    assert np.array_equal(boot['n_used'], (boot['counts'] * valid).sum(axis=1)) and np.isfinite(boot['indices']).all()


def test_a_constant_row_gives_nan():
    N, d = 16, 2
    got = sobol.sobol_indices(np.full((1, N * (d + 2)), 3.5), N, d, n_boot=2)
    assert np.isnan(got['indices']).all() and (got['var'] == 0).all()


def test_public_errors_come_before_any_device_call(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(engine, 'get_engine', no_device)

    def call(priors={'fc': (200.0, 380.0), 'T_g': (45.0, 85.0)}, **kw):
        met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
        args = dict(n_base=8, columns=['Qr'], n_boot=4)
        args.update(kw)
        return sp.sobol_indices(met, p_struc, p_SU, p_LU, p_SC, p, dyn, priors=priors, **args)

    with pytest.raises(ValueError, match="unknown parameter 'm_Q'"):
        call(priors={'fc': (200.0, 380.0), 'm_Q': (0.1, 0.5)})
    with pytest.raises(ValueError, match='at least one entry'):
        call(priors={})
    with pytest.raises(ValueError, match="prior of 'T_g' needs lo < hi"):
        call(priors={'fc': (200.0, 380.0), 'T_g': (85.0, 85.0)})
    for n_base in (1, 32769):
        with pytest.raises(ValueError, match='n_base must be in'):
            call(n_base=n_base)
    for conf in (0.0, 1.0, float('nan')):
        with pytest.raises(ValueError, match='conf must lie in'):
            call(conf=conf)
    with pytest.raises(ValueError, match='unit_samples must have shape'):
        call(unit_samples=np.zeros((2, 2, 7)))
    with pytest.raises(ValueError, match=r'unit_samples must lie in \[0, 1\)'):
        call(unit_samples=np.ones((2, 2, 8)))
    with pytest.raises(ValueError, match="'f_TDP' without obs_dict"):
        call(priors={'fc': (200.0, 380.0), 'f_TDP': (0.3, 0.7)})
    with pytest.raises(ValueError, match='columns must be distinct names'):
        call(columns=['Qr', 'no such column'])
    with pytest.raises(ValueError, match='reduce must be'):
        call(reduce='monthly')
    with pytest.raises(ValueError, match='n_boot must be in'):
        call(n_boot=-1)
    with pytest.raises(ValueError, match='the prior box holds points the model rejects'):
        call(priors={'d_maxE_spr': (20.0, 120.0)})
    with pytest.raises(AssertionError, match='the device was reached'):            # a good call goes on to the device
        call()


def test_ishigami_analytic_values_lie_inside_the_99_percent_interval():
    N, n_boot = 4096, 200
    f = ishigami(sobol.design(N, LO, HI, seed=SEED))
    got = sobol.sobol_indices(f[None], N, 3, n_boot=n_boot, seed=SEED)
    ci = sobol.percentile_interval(got['indices'], 0.99)[:, :, :, 0]              # [2 ends, 2 planes, 3]
    want = np.stack([ANALYTIC_S1, ANALYTIC_ST])
    assert (ci[0] <= want).all() and (want <= ci[1]).all(), (ci, want)
    assert (ci[1] - ci[0]).max() < 0.15                                           # and the interval says something
