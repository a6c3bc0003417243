"""The particle filter's rules on the CPU: the integer resampling rule of simplyp_amd/csrc/simplyp_resample.h against its
statement in Python integers (simplyp_amd/particle.py), the mirror's own properties, the weights, the window likelihood against
the reference's, the size of simplyp_pf_info, and the whole loop with a toy model.  tests/particle_host_main.cpp includes the
header, is built once per session with the host compiler under AddressSanitizer and UBSan, and runs as a child process that
reads cases as text.  No GPU needed."""

import ctypes as C

import numpy as np
import pytest

import helpers
import host_program
from c_header import c_values
from oracle import gof as ogof
from simplyp_amd import abi, engine, particle, visualise_results as vr

ONE = 1 << particle.WEIGHT_BITS


@pytest.fixture(scope='session')
def driver():
    """cases: lines of text -> one list of integers per case."""
    run = host_program.case_runner(host_program.build('particle_host_main.cpp'), timeout=300)
    return lambda cases: [[rc] + [int(x) for x in rest.split()] for rc, rest in run(cases)]


def patterns(E, rng):
    """name -> q [E] (Python ints): the weight patterns both the CPU and the GPU tests resample."""
    q = {'equal': [ONE] * E, 'random': [int(x) for x in rng.integers(0, ONE + 1, E)]}
    one = [0] * E
    one[int(rng.integers(0, E))] = 12345
    q['one_live'] = one
    if E >= 2:
        q['tiny_beside_full'] = [1 if i % 2 else ONE for i in range(E)]
    if E >= 8:
        z = [int(x) for x in rng.integers(1, ONE + 1, E)]
        z[:E // 4] = [0] * (E // 4)
        z[-(E // 3):] = [0] * (E // 3)
        q['zeros_at_both_ends'] = z
    return q


def test_128_bit_product_offset_and_quantisation(driver):
    rng = np.random.default_rng(3)
    vals = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 64) - 1, 1 << 62] + [int(x) for x in rng.integers(0, 1 << 63, 20)]
    pairs = [(a, b) for a in vals[:6] for b in vals[:6]] + list(zip(vals[6:16], vals[16:]))
    got = driver(['mul %d %d' % ab for ab in pairs])
    assert got == [[(a * b) >> 64, (a * b) & ((1 << 64) - 1)] for a, b in pairs]
    xs = [(x, T) for x in (0, 1, (1 << 64) - 1, int(rng.integers(0, 1 << 63))) for T in (1, 2, ONE, 1 << 62, 3 * ONE + 7)]
    got = driver(['offset %d %d' % xt for xt in xs])
    assert got == [[(x * T) >> 64] for x, T in xs] and all(0 <= r[0] < T for r, (_, T) in zip(got, xs))
    ws = [0.0, 1.0, 0.5, 2.0 ** -40, np.nextafter(2.0 ** -40, 0), np.nextafter(1.0, 0), float('nan'), 1e-300] + list(rng.uniform(0, 1, 20))
    got = driver(['quantise %s' % float(w).hex() for w in ws])
    want = particle.weights(np.log(np.array([w for w in ws if w == w and w > 0])))            # exp(log w) need not be w: the rule itself
    assert got == [[int(np.floor(w * 2.0 ** 40)) if w == w else 0] for w in ws] and got[1] == [ONE] and int(want['q'].max()) == ONE


@pytest.mark.parametrize('E', [1, 2, 63, 64, 65, 1000])
def test_cpp_rule_equals_the_mirror(driver, E):
    rng = np.random.default_rng(100 + E)
    cases, want = [], []
    for name, q in patterns(E, rng).items():
        T = sum(q)
        for r in sorted({0, T - 1, particle.resample_offset(7, 3, T), particle.resample_offset(2 ** 63 + 5, 2 ** 32 - 1, T)}):
            cases.append('resample %d %d %s' % (r, E, ' '.join(str(x) for x in q)))
            want.append((name, r, particle.resample(q, 0, 0, r=r)))
    got = driver(cases)
    for a, (name, r, m) in zip(got, want):
        assert a == list(m['ancestors']), (name, r)
        if name == 'equal':
            assert a == list(range(E)), r
        if name == 'one_live':
            assert len(set(a)) == 1 and m['n_unique'] == 1


def test_largest_products(driver):
    """E = 2^22 particles of weight 2^40: T = 2^62, the products reach 2^84; every particle is its own ancestor whatever r."""
    E = particle.MAX_E
    T = E * ONE
    rs = [0, T - 1, particle.resample_offset(11, 5, T)]
    got = driver(['uniform %d %d %d' % (r, E, ONE) for r in rs])
    assert got == [[E, 0, 0, E - 1]] * 3
    m = particle.resample(np.full(E, ONE, dtype=np.uint64), 11, 5)
    assert m['r'] == rs[2] and np.array_equal(m['ancestors'], np.arange(E)) and m['n_unique'] == E


@pytest.mark.parametrize('E', [1, 2, 65, 1000, 4097])
def test_mirror_properties(E):
    rng = np.random.default_rng(E)
    for name, q in patterns(E, rng).items():
        for seed, t in ((0, 0), (12345, 7), (2 ** 64 - 1, 2 ** 32 - 1)):
            m = particle.resample(q, seed, t)
            a, off, T = m['ancestors'], m['offspring'], sum(q)
            assert 0 <= m['r'] < T and (np.diff(a) >= 0).all() and a.min() >= 0 and a.max() < E
            assert off.sum() == E and m['n_unique'] == len(set(a.tolist()))
            for i in range(E):
                assert (E * q[i]) // T <= off[i] <= -((-E * q[i]) // T), (name, i)
            # the definition, particle by particle
            Cs = np.cumsum(np.array(q, dtype=object))
            for k in rng.integers(0, E, min(E, 40)):
                i = int(a[k])
                assert E * int(Cs[i]) > int(k) * T + m['r'] and (i == 0 or E * int(Cs[i - 1]) <= int(k) * T + m['r'])
    dead = particle.resample([0] * E, 1, 2)
    assert np.array_equal(dead['ancestors'], np.arange(E)) and dead['n_unique'] == 0 and not dead['offspring'].any()


def test_weights_mirror():
    lw = np.array([-3.0, -800.0, -np.inf, np.inf, np.nan, -1.5, -1.5 - 40 * np.log(2) - 1e-9, -1.5 - 39.5 * np.log(2)])
    w = particle.weights(lw)
    assert w['lw_max'] == -1.5 and w['q'][5] == ONE and w['w'][5] == 1.0
    assert list(w['q'][[1, 2, 3, 4, 6]]) == [0] * 5 and w['q'][7] > 0 and w['n_nan'] == 2 and w['n_alive'] == 3
    assert w['T'] == int(w['q'].astype(object).sum()) and w['sum_w'] == w['w'].sum()
    assert w['q'][0] == int(np.floor(np.exp(-1.5) * 2.0 ** 40))
    dead = particle.weights(np.array([-np.inf, np.nan, np.inf]))
    assert dead['lw_max'] == -np.inf and dead['T'] == 0 and not dead['w'].any() and not dead['q'].any() and dead['n_alive'] == 0
    assert particle.ess(4.0, 4.0) == 4.0 and particle.log_mean(-2.0, 3.0, 3) == -2.0


def window_case():
    """The golden Tarland 2004 reach series scaled into three members, with the shipped observations."""
    name = 'tarland_2004_dynamic'
    R = helpers.golden_tables(name, 'tight')['R'][1]
    info = helpers.meta()[name]['inputs']
    obs = vr.observation_array(helpers.observations(info['p_SU']['st_dt'], info['p_SU']['end_dt']), [1], R.index)[0]
    scale = np.array([1.0, 0.8, 1.3])
    out4 = np.stack([R[c].values[:, None] * scale for c in ('Qr', 'Msus_kg/day', 'TDP_kg/day', 'PP_kg/day')])
    A, f = np.full(3, info['p_SC']['1']['A_catch']), np.full(3, info['p']['f_TDP'])
    return out4, A, f, obs


def test_loglik_increment_is_the_reference_likelihood_without_its_ten_observation_rule():
    out4, A, f, obs = window_case()
    sims = ogof.simulated_series(out4[0], out4[1], out4[2], out4[3], A, f)
    variables = ['Q', 'TP', 'SRP']
    vi = [abi.GOF_VARS.index(v) for v in variables]
    m = np.array([[0.1, 0.2, 0.3], [0.4, 0.4, 0.4], [0.25, 0.5, 0.75]])
    # the whole year: every variable has more than 10 observations, and the increment is the reference's likelihood of the gof table
    st = ogof.ensemble_stats(out4, A, f, obs)
    assert (st[0, vi, 0] > 10).all()
    want = sum(vr.loglik(st[:, v], m[p]) for p, v in enumerate(vi))
    inc, scale = particle.loglik_increment(np.stack([sims[v] for v in variables]), obs[vi], m)
    assert np.isfinite(inc).all() and (np.abs(inc - want) <= 1e-12 * scale).all(), (inc, want)
    # windows that keep 1 .. 10 observations of TP (the gof table is NaN there), and none
    days = np.flatnonzero(~np.isnan(obs[vi[1]]))
    for n in (1, 2, 10):
        sl = slice(days[0], days[n - 1] + 1)
        assert np.isnan(ogof.ensemble_stats(out4[:, sl], A, f, obs[:, sl])[1:, vi[1]]).all()
        inc, scale = particle.loglik_increment(sims['TP'][None, sl], obs[vi[1]][None, sl], m[1:2])
        o, s = obs[vi[1]][sl][:, None], sims['TP'][sl]
        ok = ~np.isnan(o[:, 0])
        ref = (-0.5 * n * np.log(2 * np.pi) - n * np.log(0.4) - np.log(s[ok]).sum(axis=0) - ((o[ok] / s[ok] - 1) ** 2).sum(axis=0) / (2 * 0.4 * 0.4))
        assert ok.sum() == n and np.isfinite(inc).all() and (np.abs(inc - ref) <= 1e-12 * scale).all()
    g = int(np.argmax(np.diff(days)))                                  # the longest stretch without a sample
    gap = slice(days[g] + 1, days[g + 1])
    assert gap.stop > gap.start
    inc, scale = particle.loglik_increment(sims['TP'][None, gap], obs[vi[1]][None, gap], m[1:2])
    assert (inc == 0).all() and not np.signbit(inc).any() and (scale == 0).all()
    # what kills a particle
    sl = slice(days[g], days[g + 1] + 1)
    bad =sims['TP'][None, sl].copy()
    bad[0, 0, 1] = np.nan                                              # a NaN on an observation day
    bad[0, 1, 2] = np.nan                                              # ... and on a day without one
    inc, _ = particle.loglik_increment(bad, obs[vi[1]][None, sl], 0.4, status_ok=[False, True, True])
    assert inc[0] == -np.inf and inc[1] == -np.inf and np.isfinite(inc[2])
    inc, _ = particle.loglik_increment(sims['TP'][None, sl], obs[vi[1]][None, sl], np.array([[0.4, 0.0, -1.0]]))
    assert np.isfinite(inc[0]) and inc[1] == -np.inf and inc[2] == -np.inf


def test_pf_info_size_and_exports():
    assert c_values(['sizeof(simplyp_pf_info)'])['sizeof(simplyp_pf_info)'] == C.sizeof(abi.PfInfo) == 64
    assert {'simplyp_pf_loglik', 'simplyp_pf_weights', 'simplyp_pf_resample', 'simplyp_gather_members', 'simplyp_pf_jitter'} <= set(engine.ABI_SYMBOLS)


def toy_step(target):
    """A toy model: the per-particle state is a running sum of the first coordinate; the likelihood pulls theta towards target."""
    def step(t, theta, x):
        x = np.zeros((2, theta.shape[1])) if x is None else x
        x = x + np.stack([theta[0], np.full(theta.shape[1], float(t))])
        return -0.5 * ((theta - target[:, None]) ** 2).sum(axis=0) / 0.05 ** 2 - 1e-3 * x[0] ** 2, x
    return step


def test_run_filter_with_a_toy_model():
    lo, hi = np.array([0.0, -1.0]), np.array([1.0, 1.0])
    E = 300
    theta0 = particle.uniform_start(5, 2, E, lo, hi)
    assert ((theta0 >= lo[:, None]) & (theta0 < hi[:, None])).all()
    step = toy_step(np.array([0.3, 0.2]))
    one = particle.run_filter(step, theta0, 6, lo, hi, seed=5, record=True)
    a = particle.run_filter(step, theta0, 2, lo, hi, seed=5, record=True)
    b = particle.run_filter(step, None, 4, lo, hi, state=a['state'], record=True)
    for k in ('theta', 'lw', 'x'):
        assert np.array_equal(one[k], b[k]), k
    for k in ('ess', 'log_evidence', 'resampled', 'n_unique', 'n_outside', 'ancestors', 'inc', 'q', 'theta_after'):
        assert np.array_equal(one[k], np.concatenate([a[k], b[k]])), k
    assert one['state']['t'] == 6 and one['resampled'].all() and (one['ess'] >= 1).all() and (one['ess'] <= E).all()
    assert one['log_evidence_total'] == pytest.approx(one['log_evidence'].sum())
    again = particle.run_filter(step, theta0, 6, lo, hi, seed=5)
    other = particle.run_filter(step, theta0, 6, lo, hi, seed=6)
    assert np.array_equal(again['theta'], one['theta']) and not np.array_equal(other['theta'], one['theta'])
    # the filter finds the target, and rejuvenation keeps the duplicates apart
    assert np.abs(one['theta'].mean(axis=1) - [0.3, 0.2]).max() < 0.05
    assert len(np.unique(one['theta'][0])) > one['n_unique'][-1]
    # resampling only when the effective sample size falls below half: the log weights carry over
    lazy = particle.run_filter(step, theta0, 3, lo, hi, seed=5, resample_threshold=0.5)
    assert lazy['log_evidence_total'] == pytest.approx(lazy['log_evidence'].sum())
    with pytest.raises(RuntimeError, match='window 0'):
        particle.run_filter(lambda t, th, x: (np.full(th.shape[1], -np.inf), x), theta0, 1, lo, hi)
