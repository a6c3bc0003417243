"""The NumPy statement of the multi-start Nelder-Mead search (simplyp_amd/neldermead.py) against scipy, and its schedule.

One simplex of the mirror takes scipy's path bit for bit: the same arithmetic in the same order, the same decisions.  The target is
+inf outside the box on both sides (scipy is given no bounds).  Ties in f are outside the contract -- scipy's argsort of more than
16 values is not stable -- so every comparison first asserts that the smallest gap the mirror sorted is > 0."""

import numpy as np
import pytest

from simplyp_amd import neldermead as nm, predictive


def total(a):
    """The sum over the first axis, row after row: the same roundings for a single point [n] and for many [n, M]."""
    acc = a[0]
    for row in a[1:]:
        acc = acc + row
    return acc


def rosen(x):
    x = np.asarray(x, dtype=np.float64)
    return total(100.0 * (x[1:] - x[:-1] ** 2) ** 2 + (1.0 - x[:-1]) ** 2)


def quad5(x):
    x = np.asarray(x, dtype=np.float64)
    c = np.array([0.3, -0.2, 0.1, 0.4, -0.5]).reshape((5,) + (1,) * (x.ndim - 1))
    s = np.array([1.0, 4.0, 0.5, 9.0, 2.0]).reshape(c.shape)
    return total(s * (x - c) ** 2) + 0.3 * (x[0] - 0.3) * (x[1] + 0.2)


def parabola(x):
    x = np.asarray(x, dtype=np.float64)
    return 3.0 * (x[0] - 0.7) ** 2 + 1.25


def rough(x):
    """Not smooth anywhere: the simplex has to shrink."""
    x = np.asarray(x, dtype=np.float64)
    return np.abs(x - 0.3).max(axis=0) * (1.5 + np.sin(40.0 * total(x))) + 0.05 * total(np.round(7.0 * x)) ** 2


ROUGH_X0 = (0.9, -0.6, 0.5, 0.4, -0.3)
FREE = 1e6
CASES = {
    'rosen2_free': (rosen, (-1.2, 1.0), -FREE, FREE, 400),
    'rosen2_box': (rosen, (-1.2, 1.0), (-1.5, -0.5), (0.75, 1.08), 400),              # the minimum (1, 1) lies outside: the box is hit
    'quad5': (quad5, (1.0, 1.0, -1.0, 0.5, 0.25), -FREE, FREE, 1000),
    'rosen16': (rosen, tuple(0.5 + 0.05 * k * (-1) ** k for k in range(16)), -FREE, FREE, 3200),
    'parabola1': (parabola, (2.0,), -FREE, FREE, 200),
    'rough5': (rough, ROUGH_X0, -1.0, 1.0, 300),
}


def box_of(lo, hi, n):
    return np.broadcast_to(np.asarray(lo, dtype=np.float64), (n,)).copy(), np.broadcast_to(np.asarray(hi, dtype=np.float64), (n,)).copy()


def scipy_run(f, x0, lo, hi, max_iter):
    optimize = pytest.importorskip('scipy.optimize')
    hits = [0]

    def target(x):
        if not ((x >= lo) & (x < hi)).all():
            hits[0] += 1
            return np.inf
        return float(f(x))

    res = optimize.minimize(target, np.array(x0, dtype=np.float64), method='Nelder-Mead',
                            options=dict(maxiter=max_iter, xatol=1e-4, fatol=1e-4))
    return res, hits[0]


@pytest.mark.parametrize('case', list(CASES))
def test_one_simplex_takes_scipys_path_bit_for_bit(case):
    f, x0, lo, hi, max_iter = CASES[case]
    n = len(x0)
    lo, hi = box_of(lo, hi, n)
    got = nm.run(f, np.array(x0, dtype=np.float64)[:, None], lo, hi, max_iter=max_iter)
    assert got['min_gap'] > 0.0, got['min_gap']                       # no ties: scipy's order is defined
    want, outside = scipy_run(f, x0, lo, hi, max_iter)
    sim, fsim = want.final_simplex
    assert np.array_equal(got['sim'][:, :, 0], sim) and np.array_equal(got['fsim'][:, 0], fsim)
    assert int(got['n_iter'][0]) == want.nit and int(got['status'][0]) == want.status
    assert np.array_equal(got['x'][:, 0], want.x) and got['fun'][0] == want.fun
    h = got['history'][:want.nit, 0]
    assert np.isfinite(h).all() and (np.diff(h) <= 0).all() and np.isnan(got['history'][want.nit:, 0]).all()
    if case == 'rosen2_box':
        assert outside > 0
    if case == 'rough5':
        assert int(got['counts']['shrink'][0]) >= 1
    if case in ('rosen2_free', 'parabola1', 'quad5'):
        assert want.status == 0
    assert sum(int(c[0]) for c in got['counts'].values()) == want.nit - 1


def test_the_limit_counts_like_scipy():
    lo, hi = box_of(-FREE, FREE, 2)
    for max_iter in (1, 2, 7):
        got = nm.run(rosen, np.array([[-1.2], [1.0]]), lo, hi, max_iter=max_iter)
        want, _ = scipy_run(rosen, (-1.2, 1.0), lo, hi, max_iter)
        assert int(got['n_iter'][0]) == want.nit == max_iter and int(got['status'][0]) == want.status == 2
        assert np.array_equal(got['sim'][:, :, 0], want.final_simplex[0])


def many(n_dim, S, seed):
    lo, hi = box_of(-1.0, 1.0, n_dim)
    x0 = nm.uniform_starts(seed, n_dim, S, 0.8 * lo, 0.8 * hi)
    return x0, lo, hi


@pytest.mark.parametrize('n_dim', [1, 3, 4, 16])
def test_the_schedule_of_many_equals_single_runs(n_dim):
    """Four slots, EVAL over several runs (N + 1 = 2, 4, 5, 17), simplexes in different phases side by side."""
    S = 7
    f = rough
    x0, lo, hi = many(n_dim, S, 5)
    max_iter = 60
    got = nm.run(f, x0, lo, hi, max_iter=max_iter)
    phases_mixed = False
    st = nm.new_state(nm.initial_simplex(x0, lo, hi))
    hist = np.full((max_iter, S), np.nan)
    while (st['phase'] != nm.DONE).any():                        # the same run, watched
        pr = nm.propose(st, lo, hi)
        assert pr['prop'].shape == (n_dim, 4 * S) and pr['inside'].shape == (4 * S,)
        assert not (pr['inside'] & ~pr['used']).any()
        nm.update(st, pr['prop'], pr['inside'], -f(pr['run_point']), max_iter, history=hist)
        act = st['phase'][st['phase'] != nm.DONE]
        phases_mixed = phases_mixed or (len(set(act.tolist())) == 2)
    assert np.array_equal(st['sim'], got['sim']) and np.array_equal(hist, got['history'], equal_nan=True)
    for s in range(S):
        one = nm.run(f, x0[:, s:s + 1], lo, hi, max_iter=max_iter)
        assert np.array_equal(one['sim'][:, :, 0], got['sim'][:, :, s]) and np.array_equal(one['fsim'][:, 0], got['fsim'][:, s])
        assert one['n_iter'][0] == got['n_iter'][s] and one['status'][0] == got['status'][s]
        assert np.array_equal(one['history'][:, 0], got['history'][:, s], equal_nan=True)
        for m in nm.MOVES:
            assert one['counts'][m][0] == got['counts'][m][s]
    if n_dim > 1:                                                # (in one dimension this function never makes a contraction fail)
        assert got['counts']['shrink'].sum() >= 1 and phases_mixed
    assert (got['fsim'][:-1] <= got['fsim'][1:]).all()
    # the first run evaluates vertices 0..3, the next 4..7, ...: ceil((N + 1) / 4) runs before the first step
    st = nm.new_state(nm.initial_simplex(x0, lo, hi))
    for k in range(-(-(n_dim + 1) // 4)):
        assert (st['phase'] == nm.EVAL).all() and (st['cursor'] == 4 * k).all()
        pr = nm.propose(st, lo, hi)
        used = pr['used'].reshape(4, S)
        assert np.array_equal(used[:, 0], 4 * k + np.arange(4) <= n_dim)
        nm.update(st, pr['prop'], pr['inside'], -f(pr['run_point']), max_iter)
    assert (st['phase'] == nm.STEP).all() and (st['n_iter'] == 1).all()


def test_continuing_from_a_state_equals_the_longer_call():
    x0, lo, hi = many(3, 5, 9)
    whole = nm.run(rosen, x0, lo, hi, max_iter=40)
    first = nm.run(rosen, x0, lo, hi, max_iter=17)
    assert (first['status'] == nm.MAXITER).all()
    second = nm.run(rosen, None, lo, hi, max_iter=40, state=first['state'])
    for k in ('sim', 'fsim', 'n_iter', 'status'):
        assert np.array_equal(second[k], whole[k]), k
    assert np.array_equal(second['history'], whole['history'], equal_nan=True)


def test_a_point_outside_the_box_is_never_evaluated():
    lo, hi = np.array([-1.5, -0.5]), np.array([0.75, 1.08])
    seen = []

    def f(x):
        seen.append(x.copy())
        return rosen(x)

    got = nm.run(f, np.array([[-1.2, 0.5], [1.0, 0.2]]), lo, hi, max_iter=80)
    pts = np.concatenate(seen, axis=1)
    assert ((pts >= lo[:, None]) & (pts < hi[:, None])).all()
    assert ((got['sim'] >= lo[None, :, None]) & (got['sim'] < hi[None, :, None])).all()


def test_a_nan_or_minus_infinite_log_posterior_counts_as_plus_infinity():
    x0, lo, hi = many(2, 3, 1)
    st = nm.new_state(nm.initial_simplex(x0, lo, hi))
    pr = nm.propose(st, lo, hi)
    lp = -rosen(pr['run_point'])
    lp[0], lp[1] = np.nan, -np.inf                          # vertex 0 of simplexes 0 and 1
    info = nm.update(st, pr['prop'], pr['inside'], lp, 50)
    assert st['status'].tolist() == [nm.NONFINITE_START, nm.NONFINITE_START, nm.RUNNING]
    assert st['phase'].tolist() == [nm.DONE, nm.DONE, nm.STEP] and (st['fsim'][-1, :2] == np.inf).all()
    assert info == dict(n_active=1, n_converged=0, n_shrinking=0, n_nonfinite_start=2)


def test_initial_simplex_and_its_errors():
    lo, hi = np.array([0.0, -1.0, 0.0]), np.array([1.0, 1.0, 10.0])
    x0 = np.array([[0.5, 0.99], [0.0, 0.5], [2.0, 9.9]])
    sim = nm.initial_simplex(x0, lo, hi)
    assert sim.shape == (4, 3, 2) and np.array_equal(sim[0], x0)
    assert np.array_equal(sim[1, 0], [1.05 * 0.5, 0.95 * 0.99])               # 1.05 x leaves the box: 0.95 x
    assert np.array_equal(sim[2, 1], [0.00025, 1.05 * 0.5]) and np.array_equal(sim[3, 2], [1.05 * 2.0, 0.95 * 9.9])
    for j in range(1, 4):                                                     # one coordinate differs per vertex
        assert (sim[j] != x0).sum(axis=0).tolist() == [1, 1]
    with pytest.raises(ValueError, match='outside the box'):
        nm.initial_simplex(np.array([[1.0], [0.0], [1.0]]), lo, hi)
    with pytest.raises(ValueError, match='both sides'):
        nm.initial_simplex(np.array([[0.5]]), np.array([0.49]), np.array([0.51]))
    with pytest.raises(ValueError, match='n_dim must be'):
        nm.initial_simplex(np.zeros((17, 1)), -np.ones(17), np.ones(17))
    with pytest.raises(ValueError, match='lo < hi'):
        nm.initial_simplex(np.zeros((2, 1)), np.array([0.0, 1.0]), np.array([1.0, 1.0]))
    with pytest.raises(ValueError, match='max_iter'):
        nm.run(rosen, np.zeros((2, 1)), -np.ones(2), np.ones(2), max_iter=0)


def test_uniform_starts_are_the_documented_philox_draws():
    lo, hi = np.array([-1.0, 10.0, 0.0]), np.array([1.0, 20.0, 1e-3])
    x = nm.uniform_starts(77, 3, 50, lo, hi)
    u, _ = predictive.uniforms(77, np.arange(50)[None, :], np.arange(3)[:, None], 0, nm.START_STREAM)
    assert np.array_equal(x, lo[:, None] + (hi - lo)[:, None] * u)
    assert ((x >= lo[:, None]) & (x < hi[:, None])).all() and len(np.unique(x)) == 150
    assert not np.array_equal(x, nm.uniform_starts(78, 3, 50, lo, hi))


def test_start_ball_is_the_samplers_default_start():
    from simplyp_amd import calibrate
    priors = {'fc': (200.0, 400.0), 'm_Q': (0.01, 1.0)}
    centre = np.array([290.0, 0.4])
    got = calibrate.start_ball(centre, priors, 12, seed=5)
    z = predictive.standard_normal(5, np.arange(12)[None, :], np.arange(2)[:, None], 0, calibrate.START_SERIES)
    lo, hi = np.array([200.0, 0.01]), np.array([400.0, 1.0])
    assert np.array_equal(got, centre[:, None] + (1e-4 * (hi - lo))[:, None] * z) and got.shape == (2, 12)
    with pytest.raises(ValueError, match='one value per name'):
        calibrate.start_ball(centre[:1], priors, 12, seed=5)
    with pytest.raises(ValueError, match='outside the prior box'):
        calibrate.start_ball(np.array([200.0, 0.4]), priors, 64, seed=5)
