"""The particle filter's device steps (simplyp_pf_loglik, simplyp_pf_weights, simplyp_pf_resample, simplyp_gather_members,
simplyp_pf_jitter) against their NumPy statement (simplyp_amd/particle.py), and ``assimilate`` end to end.  All model runs use the
Tarland 2004 scenario, one reach.

Tolerances.
* log-likelihood, device against the mirror applied to the device's own table: 1e-12 times the mirror's sum of the absolute
  values of its terms -- the project's bar for log-bearing sums (tests/test_gpu_mcmc.py), on a scale that cancellation can
  neither hide behind nor inflate.  The same bar against ``mcmc_log_prob`` of ``gof`` and against an independent ensemble run.
* q: ``|q_device - q_mirror| <= 1`` -- the device's exp and NumPy's may differ by an ulp, which moves floor across an integer
  and no further; T is the exact integer sum of the device's q; sum_w and sum_w2 against NumPy's sums of the device's w within
  ``E 2^-52`` relative, the bound of any summation order over non-negative terms.
* ancestors, offspring, gathered words: bit for bit.
* the move: ``|y_device - y_mirror| <= scale[d] 2^-45 + 2 ulp(y)`` -- 2^-45 is the bound tests/test_gpu_predictive.py derives
  and asserts for the normals --; the inside decision wherever the mirror's y is further than that from both faces of the box."""

import numpy as np
import pytest
import torch

import helpers
import simplyp_amd as sp
from oracle import gof as ogof
from simplyp_amd import abi, engine, marshal, particle, visualise_results as vr

pytestmark = pytest.mark.gpu

NAME = 'tarland_2004_dynamic'
FLUX = ['Qr', 'Msus_kg/day', 'TDP_kg/day', 'PP_kg/day']
MASK = marshal.mask_of_columns(FLUX)
ONE = 1 << particle.WEIGHT_BITS
SENTINEL = -777.25
V = {v: i for i, v in enumerate(abi.GOF_VARS)}
SIZES = [1, 2, 63, 64, 65, 1000, 4097, 65537]
NAN_WORD = 0x7ff8000000000000


def dev(eng, a, dtype=torch.float64):
    return eng.to_device(np.ascontiguousarray(a), dtype)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


# ---- the window's log-likelihood ----------------------------------------------------------------------------------------------

_windows = {}


def window(eng, E):
    """The first 40 days of 2004 for E members that differ in fc, a_Q and f_TDP: the device table, what came with it, and the
    shipped observations -- 39 days of Q (more than 10), 5 of SS, TDP and SRP (1 to 10), none of PP and TP."""
    if E not in _windows:
        m = helpers.marshal_scenario(NAME, E, out_mask=MASK)
        rng = np.random.default_rng(E)
        mp = m['member_params'].copy()
        mp[marshal.PM_NAMES.index('fc')] *= rng.uniform(0.8, 1.2, E)
        mp[marshal.PM_NAMES.index('a_Q')] *= rng.uniform(0.8, 1.2, E)
        f = rng.uniform(0.3, 0.9, E)
        D = 40
        out, status, _ = eng.run(m['forcing'][:, :, :D], m['doy'][:D], mp, m['reach_params'], m['up_ptr'], m['up_idx'], m['opts'])
        assert int(status.cpu().numpy().max()) == 0
        obs = vr.observation_array(helpers.observations('2004-01-01', '2004-12-31'), [1], m['met'].index)[:, :, :D]
        n = (~np.isnan(obs[0])).sum(axis=1)
        assert n[V['Q']] > 10 and 1 <= n[V['SS']] <= 10 and n[V['PP']] == 0 and n[V['TP']] == 0
        _windows[E] = dict(out=out, status=status, obs=obs, f=f, rp=m['reach_params'], D=D,
                           A=m['reach_params'][marshal.PR_NAMES.index('A_catch'), 0])
    return _windows[E]


def mirror_inc(w, table, pairs, m, status_ok=None):
    """The mirror applied to a table [4, D, 1, E] on the host."""
    sims = ogof.simulated_series(table[0, :, 0], table[1, :, 0], table[2, :, 0], table[3, :, 0], w['A'], w['f'])
    with np.errstate(all='ignore'):
        return particle.loglik_increment(np.stack([sims[abi.GOF_VARS[v]] for v, _ in pairs]), np.stack([w['obs'][r, v] for v, r in pairs]),
                                         m, status_ok)


def device_inc(eng, w, pairs, m, lw=None, table=None, accumulate=False, **kw):
    E = w['out'].shape[-1]
    lw_d = torch.full((E,), SENTINEL, dtype=torch.float64, device=eng.tdev) if lw is None else dev(eng, lw)
    inc_d = torch.full((E,), SENTINEL, dtype=torch.float64, device=eng.tdev)
    info = eng.pf_loglik(w['out'] if table is None else table, MASK, w['obs'], pairs, dev(eng, np.broadcast_to(m, (len(pairs), E))), lw_d,
                         w['f'], w['rp'], inc=inc_d, accumulate=accumulate, **kw)
    return lw_d.cpu().numpy(), inc_d.cpu().numpy(), info


PAIR_CASES = {'more_than_10': [(V['Q'], 0)], 'one_to_10': [(V['SS'], 0)], 'none': [(V['PP'], 0)],
              'mixed': [(V['SRP'], 0), (V['PP'], 0), (V['Q'], 0), (V['TDP'], 0), (V['TP'], 0)]}


@pytest.mark.parametrize('E', [1, 63, 64, 65, 200])
def test_loglik_matches_the_mirror(engine0, E):
    w = window(engine0, E)
    table = w['out'].cpu().numpy()
    rng = np.random.default_rng(7 * E)
    for name, pairs in PAIR_CASES.items():
        m = rng.uniform(0.1, 0.6, (len(pairs), E))
        lw, inc, info = device_inc(engine0, w, pairs, m)
        want, scale = mirror_inc(w, table, pairs, m)
        err = np.abs(inc - want)
        print('%s E = %d: max |inc - mirror| / scale = %.3e' % (name, E, float((err / np.maximum(scale, 1e-300)).max())))
        assert np.isfinite(want).all() and (err <= 1e-12 * scale).all(), name
        assert np.array_equal(bits(lw), bits(inc)) and info['n_nan'] == 0
        if name == 'none':
            assert (inc == 0).all() and not np.signbit(inc).any()
    # more than 10 observations: the same number through the goodness-of-fit table
    gof, _ = engine0.gof(w['out'], MASK, w['obs'], w['f'], w['rp'])
    m = rng.uniform(0.1, 0.6, (1, E))
    lp = torch.full((E,), SENTINEL, dtype=torch.float64, device=engine0.tdev)
    engine0.mcmc_log_prob(gof, [(V['Q'], 0)], [0, -1, -1, -1, -1, -1], [float('nan')] * 6, dev(engine0, m), lp, status=w['status'])
    _, inc, _ = device_inc(engine0, w, [(V['Q'], 0)], m)
    _, scale = mirror_inc(w, table, [(V['Q'], 0)], m)
    assert (np.abs(inc - lp.cpu().numpy()) <= 1e-12 * scale).all()


def test_loglik_without_observations_leaves_the_weights_alone(engine0):
    w = window(engine0, 200)
    lw0 = np.random.default_rng(1).normal(-30, 5, 200)
    lw, inc, _ = device_inc(engine0, w, [(V['PP'], 0), (V['TP'], 0)], 0.3, lw=lw0, accumulate=True)
    assert np.array_equal(bits(inc), bits(np.zeros(200))) and np.array_equal(bits(lw), bits(lw0))


def test_loglik_is_minus_infinity_where_the_particle_does_not_count(engine0):
    E = 200
    w = window(engine0, E)
    table = w['out'].cpu().numpy()
    pairs = [(V['Q'], 0), (V['SS'], 0)]
    m = np.full((2, E), 0.3)
    m[0, 5], m[1, 6] = 0.0, -0.1
    st = np.zeros(E, dtype=np.int32)
    st[7], st[8] = abi.STATUS_NONFINITE, abi.STATUS_STEPCAP
    q_days, ss_days = np.flatnonzero(~np.isnan(w['obs'][0, V['Q']])), np.flatnonzero(~np.isnan(w['obs'][0, V['SS']]))
    free = np.setdiff1d(np.arange(w['D']), q_days)                                      # a day without any paired observation
    assert len(free) >= 1 and not np.isin(free, ss_days).any()
    bad = table.copy()
    bad[0, q_days[3], 0, 11] = np.nan                                                   # Qr on an observation day
    bad[1, ss_days[1], 0, 12] = np.nan                                                  # the SS flux on an SS day
    bad[0, free[0], 0, 13] = np.nan                                                     # a day nobody observed
    bad[2, q_days[0], 0, 14] = np.nan                                                   # a column the pairs do not read
    lw, inc, info = device_inc(engine0, w, pairs, m, table=dev(engine0, bad), status=dev(engine0, st, torch.int32))
    dead = [5, 6, 7, 11, 12]
    assert (inc[dead] == -np.inf).all() and info['n_nan'] == 2
    ok = np.setdiff1d(np.arange(E), dead)
    _, clean, _ = device_inc(engine0, w, pairs, m)
    assert np.array_equal(bits(inc[ok]), bits(clean[ok]))                               # members 8, 13, 14 among them: nothing changed
    want, scale = mirror_inc(w, bad, pairs, m, status_ok=(st & abi.STATUS_NONFINITE) == 0)
    assert np.array_equal(np.isneginf(want), np.isneginf(inc)) and (np.abs(inc[ok] - want[ok]) <= 1e-12 * scale[ok]).all()


def test_loglik_through_member_of_slot_and_accumulation(engine0):
    E = 200
    w = window(engine0, E)
    rng = np.random.default_rng(5)
    perm = rng.permutation(E).astype(np.int32)                                          # slot j holds member perm[j]
    pairs = PAIR_CASES['mixed']
    m = rng.uniform(0.1, 0.6, (len(pairs), E))
    _, inc, _ = device_inc(engine0, w, pairs, m)
    shuffled = w['out'][..., torch.from_numpy(perm).long().to(engine0.tdev)].contiguous()
    _, inc_p, _ = device_inc(engine0, w, pairs, m, table=shuffled, member_of_slot=dev(engine0, perm, torch.int32))
    assert np.array_equal(bits(inc_p), bits(inc))
    lw0 = rng.normal(-10, 2, E)
    _, inc2, _ = device_inc(engine0, w, PAIR_CASES['one_to_10'], 0.4)
    lw_d = dev(engine0, lw0)
    em1, em2 = dev(engine0, m), dev(engine0, np.full((1, E), 0.4))
    engine0.pf_loglik(w['out'], MASK, w['obs'], pairs, em1, lw_d, w['f'], w['rp'], accumulate=True)
    engine0.pf_loglik(w['out'], MASK, w['obs'], PAIR_CASES['one_to_10'], em2, lw_d, w['f'], w['rp'], accumulate=True)
    assert np.array_equal(bits(lw_d.cpu().numpy()), bits((lw0 + inc) + inc2))


# ---- weights --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('E', [1, 2, 65, 4096])
def test_weights_match_the_mirror(engine0, E):
    rng = np.random.default_rng(E)
    lw = rng.uniform(-800.0, 0.0, E)
    lw[rng.integers(0, E)] = -1e-3                                                      # the maximum, and near it a crowd
    if E >= 65:
        lw[rng.choice(E, E // 3, replace=False)] = -1e-3 - rng.uniform(0, 35, E // 3)
        lw[[4, 9]], lw[[5, 17]], lw[[6]] = -np.inf, np.inf, np.nan
    want = particle.weights(lw)
    w_d, q_d, info = engine0.pf_weights(dev(engine0, lw))
    w, q = w_d.cpu().numpy(), q_d.cpu().numpy()
    assert info['lw_max'] == want['lw_max'] == np.max(lw[np.isfinite(lw)])
    assert np.abs(q - want['q'].astype(np.int64)).max() <= 1
    top = lw == want['lw_max']
    assert (q[top] == ONE).all() and (w[top] == 1.0).all() and (q[~np.isfinite(lw)] == 0).all() and (w[~np.isfinite(lw)] == 0).all()
    assert np.array_equal(q, np.floor(w * 2.0 ** 40).astype(np.int64))
    assert info['T'] == sum(int(x) for x in q) and info['n_alive'] == int((q > 0).sum()) and info['n_nan'] == want['n_nan']
    assert abs(info['sum_w'] - w.sum()) <= E * 2.0 ** -52 * w.sum() and abs(info['sum_w2'] - (w * w).sum()) <= E * 2.0 ** -52 * (w * w).sum()


def test_weights_when_every_particle_is_dead(engine0):
    lw = np.array([-np.inf, np.nan, np.inf, -np.inf] * 20)
    w_d, q_d, info = engine0.pf_weights(dev(engine0, lw))
    assert not w_d.cpu().numpy().any() and not q_d.cpu().numpy().any()
    assert info['lw_max'] == -np.inf and info['T'] == 0 and info['n_alive'] == 0 and info['sum_w'] == 0 and info['n_nan'] == 40


# ---- resampling -----------------------------------------------------------------------------------------------------------------

def patterns(E, rng):
    """The weight patterns of tests/test_particle_host.py."""
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


@pytest.mark.parametrize('E', SIZES)
def test_resample_matches_the_mirror_bit_for_bit(engine0, E):
    rng = np.random.default_rng(100 + E)
    draws = [(0, 0), (0xDEADBEEF12345678, 7), (2 ** 64 - 1, 2 ** 32 - 1)][:3 if E <= 4097 else 1]
    for name, q in patterns(E, rng).items():
        q_d = dev(engine0, np.array(q, dtype=np.int64), torch.int64)
        for seed, t in draws:
            want = particle.resample(q, seed, t)
            anc = torch.full((E,), -5, dtype=torch.int32, device=engine0.tdev)
            off = torch.full((E,), -5, dtype=torch.int32, device=engine0.tdev)
            _, _, info = engine0.pf_resample(q_d, seed, t, ancestors=anc, offspring=off)
            assert np.array_equal(anc.cpu().numpy(), want['ancestors']), (name, seed, t)
            assert np.array_equal(off.cpu().numpy(), want['offspring']), (name, seed, t)
            assert info['n_unique'] == want['n_unique'] and info['T'] == want['T'] == sum(q)
        if name == 'equal':
            assert np.array_equal(want['ancestors'], np.arange(E))
    dead = torch.zeros((E,), dtype=torch.int64, device=engine0.tdev)
    anc, off, info = engine0.pf_resample(dead, 3, 4)
    assert np.array_equal(anc.cpu().numpy(), np.arange(E)) and info['n_unique'] == 0 and info['T'] == 0 and not off.cpu().numpy().any()
    anc, off, info = engine0.pf_resample(q_d, 3, 4, offspring=False)                    # without the offspring
    assert off is None and np.array_equal(anc.cpu().numpy(), particle.resample(q, 3, 4)['ancestors'])


def test_resample_at_the_largest_products(engine0):
    """2^22 particles of weight 2^40: T = 2^62, products up to 2^84; every particle is its own ancestor whatever the offset."""
    E = particle.MAX_E
    q_d = torch.full((E,), ONE, dtype=torch.int64, device=engine0.tdev)
    anc, off, info = engine0.pf_resample(q_d, 11, 5)
    assert torch.equal(anc, torch.arange(E, dtype=torch.int32, device=engine0.tdev)) and bool((off == 1).all())
    assert info['n_unique'] == E and info['T'] == E * ONE


# ---- the gather -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('E', SIZES)
def test_gather_equals_numpy_take(engine0, E):
    rng = np.random.default_rng(E)
    anc = np.sort(rng.integers(0, E, E)).astype(np.int32)
    anc_d = dev(engine0, anc, torch.int32)
    for n_rows in (0, 1, 16, 47):
        src = rng.integers(-2 ** 63, 2 ** 63 - 1, (n_rows, E), dtype=np.int64)           # every bit pattern, NaN payloads included
        src[:, ::7] = bits(np.array([np.nan]))[0] | 0x5A5
        src_d = dev(engine0, src.view(np.float64))
        dst = torch.full((n_rows, E), SENTINEL, dtype=torch.float64, device=engine0.tdev)
        _, info = engine0.gather_members(src_d, anc_d, dst)
        assert np.array_equal(bits(dst.cpu().numpy()), np.take(src, anc, axis=1)) and info['n_bad'] == 0, n_rows
        assert np.array_equal(bits(src_d.cpu().numpy()), src)
    st = dev(engine0, rng.normal(size=(3, abi.N_STATE, E)))                              # a state-shaped tensor, a new destination
    got, _ = engine0.gather_members(st, anc_d)
    assert np.array_equal(got.cpu().numpy(), st.cpu().numpy()[..., anc])
    if E >= 8:                                                                           # ancestors outside [0, E) are never read
        wild = anc.copy()
        wild[3], wild[5], wild[E - 1] = -1, E, 2 ** 31 - 1
        got, info = engine0.gather_members(src_d, dev(engine0, wild, torch.int32))
        g = bits(got.cpu().numpy())
        okk = np.setdiff1d(np.arange(E), [3, 5, E - 1])
        assert info['n_bad'] == 3 and (g[:, [3, 5, E - 1]] == NAN_WORD).all() and np.array_equal(g[:, okk], np.take(src, wild[okk], axis=1))


@pytest.mark.parametrize('E', [3, 65])
def test_gather_past_the_grid_cap(engine0, E):
    """The launch caps grid.y at 65535 blocks of 8 rows and simplyp_gather_members_kernel strides over the rest
    (r0 += gridDim.y * PF_GATHER_ROWS): 8 * 65535 + 11 rows give the first 11 row blocks a second trip, the last of them a
    partial one.  The destination is followed by 8 rows nobody may write."""
    n_rows = 8 * 65535 + 11
    rng = np.random.default_rng(E)
    anc = np.sort(rng.integers(0, E, E)).astype(np.int32)
    src = rng.integers(-2 ** 63, 2 ** 63 - 1, (n_rows, E), dtype=np.int64)               # every bit pattern, NaN payloads included
    src[:, ::7] = bits(np.array([np.nan]))[0] | 0x5A5
    src_d = dev(engine0, src.view(np.float64))
    wild = anc.copy()                                                                    # three ancestors outside [0, E)
    at = [3, 5, E - 1] if E >= 8 else [0, 1, 2]
    wild[at] = -1, E, 2 ** 31 - 1
    okk = np.setdiff1d(np.arange(E), at)
    for a, n_bad in ((anc, 0), (wild, 3)):
        whole = torch.full((n_rows + 8, E), SENTINEL, dtype=torch.float64, device=engine0.tdev)
        _, info = engine0.gather_members(src_d, dev(engine0, a, torch.int32), whole[:n_rows])
        got = bits(whole.cpu().numpy())
        assert info['n_bad'] == n_bad and (got[n_rows:] == bits(np.array([SENTINEL]))[0]).all()
        assert np.array_equal(got[:n_rows, okk], np.take(src, a[okk], axis=1))
        if n_bad:
            assert (got[:n_rows, at] == NAN_WORD).all()                                  # in both trips
        else:
            assert np.array_equal(got[:n_rows], np.take(src, a, axis=1))
    assert np.array_equal(bits(src_d.cpu().numpy()), src)


# ---- the rejuvenation move --------------------------------------------------------------------------------------------------------

def jitter_problem(E, n_dim):
    rng = np.random.default_rng(1000 * E + n_dim)
    lo = -1.0 - np.arange(n_dim) * 0.125
    hi = 1.5 + np.arange(n_dim) * 0.25
    theta = lo[:, None] + (hi - lo)[:, None] * rng.uniform(size=(n_dim, E))
    centre = theta.mean(axis=1) + 0.01
    scale = 0.15 * (hi - lo)
    scale[n_dim // 2] = 0.0                                                              # a dimension that only shrinks
    target = np.array([2, abi.MCMC_TARGET_F_TDP, abi.MCMC_TARGET_NONE] + list(range(5, 5 + n_dim)), dtype=np.int32)[:n_dim]
    return theta, lo, hi, centre, scale, target


def margin_of(y, scale):
    return scale[:, None] * 2.0 ** -45 + 2 * np.spacing(np.abs(y))


@pytest.mark.parametrize('E,n_dim', [(1, 1), (65, 16), (4097, 5), (1000, 2)])
def test_jitter_matches_the_mirror(engine0, E, n_dim):
    theta, lo, hi, centre, scale, target = jitter_problem(E, n_dim)
    seed, a = 0xDEADBEEF12345678, 0.9
    for t in (0, 7, 2 ** 32 - 1):
        want = particle.jitter(theta, t, a, centre, scale, lo, hi, seed)
        y, tol = want['y'], margin_of(want['y'], scale)
        near = ((np.abs(y - lo[:, None]) <= tol) | (np.abs(y - hi[:, None]) <= tol)).any(axis=0)
        assert near.mean() <= 0.01                                                       # the decision is settled for (nearly) all
        th_d = dev(engine0, theta)
        mp = torch.full((marshal.NP_M, E), SENTINEL, dtype=torch.float64, device=engine0.tdev)
        ft = torch.full((E,), SENTINEL, dtype=torch.float64, device=engine0.tdev)
        info = engine0.pf_jitter(th_d, t, a, centre, scale, lo, hi, target, mp, ft, seed=seed)
        got = th_d.cpu().numpy()
        ins = want['inside']
        keep = ~near & ~ins
        assert np.array_equal(bits(got[:, keep]), bits(theta[:, keep]))                 # outside: the whole particle stays
        go = ~near & ins
        assert (np.abs(got[:, go] - y[:, go]) <= tol[:, go]).all()
        assert abs(info['n_outside'] - int((~ins).sum())) <= int(near.sum())
        if E > 64:
            assert 0 < int((~ins).sum()) < E
        got_mp, got_ft = mp.cpu().numpy(), ft.cpu().numpy()
        named = set()
        for d in range(n_dim):
            if target[d] >= 0:
                assert np.array_equal(bits(got_mp[target[d]]), bits(got[d])), d
                named.add(int(target[d]))
            elif target[d] == abi.MCMC_TARGET_F_TDP:
                assert np.array_equal(bits(got_ft), bits(got[d]))
        rest = [r for r in range(marshal.NP_M) if r not in named]
        assert (got_mp[rest] == SENTINEL).all()                                          # rows that no dimension names are untouched
        if n_dim < 2:
            assert (got_ft == SENTINEL).all()
    # a = 1 around 0 with no noise is the identity, bit for bit
    th_d = dev(engine0, theta)
    none = np.full(n_dim, abi.MCMC_TARGET_NONE, dtype=np.int32)
    info = engine0.pf_jitter(th_d, 3, 1.0, np.zeros(n_dim), np.zeros(n_dim), lo, hi, none)
    assert np.array_equal(bits(th_d.cpu().numpy()), bits(theta)) and info['n_outside'] == 0


# ---- argument errors of the ABI ---------------------------------------------------------------------------------------------------

def test_abi_argument_errors(engine0):
    E = 65
    w = window(engine0, E)
    f64 = dict(dtype=torch.float64, device=engine0.tdev)
    i32 = dict(dtype=torch.int32, device=engine0.tdev)
    lw, inc, em = torch.full((E,), SENTINEL, **f64), torch.full((E,), SENTINEL, **f64), torch.full((1, E), 0.3, **f64)

    def refused(name, call):
        with pytest.raises(engine.EngineError, match=r'%s failed \(-1\): %s' % (name, name)):
            call()

    L = engine.lib()
    import ctypes as C
    for pairs in ([(6, 0)], [(0, 1)], [(0, 0)] * 33, []):
        refused('simplyp_pf_loglik', lambda: engine0.pf_loglik(w['out'], MASK, w['obs'], pairs, torch.full((len(pairs), E), 0.3, **f64), lw,
                                                               w['f'], w['rp'], inc=inc))
    refused('simplyp_pf_loglik', lambda: engine0.pf_loglik(w['out'][:3].contiguous(), MASK & ~(1 << marshal.ALL_COLUMNS.index('Qr')), w['obs'],
                                                           [(0, 0)], em, lw, w['f'], w['rp']))
    assert (lw == SENTINEL).all() and (inc == SENTINEL).all()
    info = abi.PfInfo()
    h = engine0._h
    big = (1 << 22) + 1
    q = torch.zeros((E,), dtype=torch.int64, device=engine0.tdev)
    anc = torch.full((E,), -5, **i32)
    wt = torch.full((E,), SENTINEL, **f64)
    bad_calls = [L.simplyp_pf_weights(h, 0, lw.data_ptr(), wt.data_ptr(), q.data_ptr(), C.byref(info)),
                 L.simplyp_pf_weights(h, big, lw.data_ptr(), wt.data_ptr(), q.data_ptr(), C.byref(info)),
                 L.simplyp_pf_weights(h, E, None, wt.data_ptr(), q.data_ptr(), C.byref(info)),
                 L.simplyp_pf_weights(h, E, lw.data_ptr(), wt.data_ptr(), None, C.byref(info)),
                 L.simplyp_pf_resample(h, 0, q.data_ptr(), 0, 0, anc.data_ptr(), None, C.byref(info)),
                 L.simplyp_pf_resample(h, big, q.data_ptr(), 0, 0, anc.data_ptr(), None, C.byref(info)),
                 L.simplyp_pf_resample(h, E, None, 0, 0, anc.data_ptr(), None, C.byref(info)),
                 L.simplyp_pf_resample(h, E, q.data_ptr(), 0, 0, None, None, C.byref(info)),
                 L.simplyp_gather_members(h, 0, 1, anc.data_ptr(), lw.data_ptr(), wt.data_ptr(), C.byref(info)),
                 L.simplyp_gather_members(h, E, -1, anc.data_ptr(), lw.data_ptr(), wt.data_ptr(), C.byref(info)),
                 L.simplyp_gather_members(h, E, 1, None, lw.data_ptr(), wt.data_ptr(), C.byref(info)),
                 L.simplyp_gather_members(h, E, 1, anc.data_ptr(), None, wt.data_ptr(), C.byref(info)),
                 L.simplyp_gather_members(h, E, 1, anc.data_ptr(), lw.data_ptr(), None, C.byref(info))]
    assert bad_calls == [-1] * len(bad_calls)
    assert (wt == SENTINEL).all() and (anc == -5).all()
    both = torch.full((3, E), SENTINEL, **f64)                                           # overlapping source and destination
    idn = torch.arange(E, **i32)
    refused('simplyp_gather_members', lambda: engine0.gather_members(both[0:2], idn, both[1:3]))
    refused('simplyp_gather_members', lambda: engine0.gather_members(both[1:3], idn, both[0:2]))
    refused('simplyp_gather_members', lambda: engine0.gather_members(both[0:1], idn, both[0:1]))
    assert (both == SENTINEL).all()
    engine0.gather_members(both[0:1], idn, both[1:2])                                    # neighbours do not overlap
    assert L.simplyp_gather_members(h, E, 0, None, None, None, C.byref(info)) == 0       # no rows: nothing to do

    theta, lo, hi, centre, scale, target = jitter_problem(E, 3)
    th_d = dev(engine0, theta)
    mp, ft = torch.full((marshal.NP_M, E), SENTINEL, **f64), torch.full((E,), SENTINEL, **f64)
    nan = float('nan')

    def jit(theta_d=th_d, a=0.9, centre_=centre, scale_=scale, lo_=lo, hi_=hi, tg=target, mp_=mp, ft_=ft):
        return engine0.pf_jitter(theta_d, 0, a, centre_, scale_, lo_, hi_, tg, mp_, ft_)

    z17 = np.zeros(17)
    for kw in (dict(a=nan), dict(a=float('inf')), dict(centre_=np.array([0, nan, 0])), dict(scale_=np.array([0.1, -0.1, 0])),
               dict(scale_=np.array([0.1, nan, 0])), dict(lo_=np.array([0.0, 5.0, 0.0]), hi_=np.array([1.0, 5.0, 1.0])),
               dict(hi_=np.array([1.0, nan, 1.0])), dict(tg=np.array([2, -3, 5])), dict(tg=np.array([2, 2, 5])),
               dict(tg=np.array([marshal.NP_M, 0, 1])), dict(mp_=None), dict(ft_=None),
               dict(theta_d=torch.zeros((17, E), **f64), centre_=z17, scale_=z17, lo_=z17, hi_=z17 + 1, tg=np.full(17, -2))):
        refused('simplyp_pf_jitter', lambda: jit(**kw))
    assert np.array_equal(bits(th_d.cpu().numpy()), bits(theta)) and (mp == SENTINEL).all() and (ft == SENTINEL).all()
    jit()                                                                                # a valid call afterwards works
    assert not np.array_equal(th_d.cpu().numpy(), theta)


# ---- the public call --------------------------------------------------------------------------------------------------------------

E_PUB, SEED_PUB, Q_BAND = 256, 11, [0.025, 0.5, 0.975]


def public(days=slice(None), **kw):
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
    obs_dict = helpers.observations(p_SU['st_dt'], p_SU['end_dt'])
    priors = {nm: (0.7 * float(p[nm]), 1.3 * float(p[nm])) for nm in ('fc', 'T_g', 'a_Q')}
    priors['m_Q'] = (0.01, 1.0)
    args = dict(priors=priors, variables=['Q'], n_particles=E_PUB, window=30, seed=SEED_PUB, record=True, quantiles=Q_BAND)
    args.update(kw)
    return sp.assimilate(met.iloc[days], p_struc, p_SU, p_LU, p_SC, p, dyn, obs_dict, **args), priors, obs_dict


@pytest.fixture(scope='module')
def year(engine0):
    return public()


def test_public_bookkeeping(engine0, year):
    res, priors, _ = year
    n = len(res['windows'])
    assert res['names'] == ['fc', 'T_g', 'a_Q', 'm_Q'] and n == 13 and res['windows'][-1][2:] == (360, 366)
    assert res['log_evidence_total'] == pytest.approx(float(np.sum(res['log_evidence'])), rel=1e-15) and np.isfinite(res['log_evidence']).all()
    assert (res['ess'] >= 1).all() and (res['ess'] <= E_PUB).all() and res['resampled'].all()
    assert all(len(res['kernel_ms'][k]) == n for k in ('run', 'loglik', 'weights', 'resample', 'gather', 'jitter')) and len(res['pilot_ms']) == n
    assert min(res['kernel_ms']['run']) > 0 and min(res['kernel_ms']['gather']) > 0
    lo = np.array([priors[nm][0] for nm in res['names']])[:, None]
    hi = np.array([priors[nm][1] for nm in res['names']])[:, None]
    assert ((res['theta'] >= lo) & (res['theta'] < hi)).all() and not res['log_weights'].any()
    assert sorted(res['overrides']) == ['T_g', 'a_Q', 'fc'] and np.array_equal(res['error_m']['Q_cumecs'], res['theta'][3])
    assert res['state']['t'] == n and res['state']['day'] == 366 and res['state']['data'].shape == (1, abi.N_STATE, E_PUB)
    # rejuvenation keeps the duplicates apart
    assert len(np.unique(res['theta'][0])) > res['n_unique'][-1] and (res['n_unique'] < E_PUB).all()


def test_public_ancestors_states_and_positions_travel_together(engine0, year):
    res, priors, obs_dict = year
    for w in range(len(res['windows'])):
        want = particle.resample(res['q'][w], SEED_PUB, w)
        assert np.array_equal(res['ancestors'][w], want['ancestors']) and res['n_unique'][w] == want['n_unique'], w
        if w + 1 < len(res['windows']):
            assert np.array_equal(bits(res['state_in'][w + 1]), bits(res['state_out'][w][..., res['ancestors'][w]])), w
            assert np.array_equal(bits(res['theta_before'][w + 1]), bits(res['theta_after'][w]))
    assert res['state_in'][0] is None and np.array_equal(bits(res['state']['data']), bits(res['state_out'][-1][..., res['ancestors'][-1]]))
    # every window's increment from an independent ensemble run at the recorded positions, started from the recorded state
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
    obs = vr.observation_array(obs_dict, [1], met.index)
    A = float(p_SC.loc['A_catch', 1])
    for w, (_, _, d_lo, d_hi) in enumerate(res['windows']):
        th = res['theta_before'][w]
        met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
        ens = sp.run_simply_p_ensemble(met.iloc[d_lo:d_hi], p_struc, p_SU, p_LU, p_SC, p, dyn, overrides={nm: th[d] for d, nm in enumerate(res['names'][:3])},
                                       outputs=FLUX, initial_state=res['state_in'][w])
        assert ens['columns'] == FLUX and int(ens['status'].max()) == 0
        Q = ens['data'][0, :, 0] * A * 1000 / 86400
        want, scale = particle.loglik_increment(Q[None], obs[0, V['Q']][None, d_lo:d_hi], th[3][None])
        assert (np.abs(res['inc'][w] - want) <= 1e-12 * scale).all(), (w, np.abs(res['inc'][w] - want).max())


def test_public_first_forecast_band_is_the_ensemble_calls(engine0, year):
    res, _, _ = year
    fc = res['forecast']
    assert fc['series'] == ['Q_cumecs'] == fc['overall_series'] and fc['param_only'].shape == (3, 1, 366, 1) == fc['overall'].shape
    assert (fc['overall'][0] <= fc['overall'][2]).all() and np.isfinite(fc['overall']).all()
    th = res['theta_before'][0]
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
    ens = sp.run_simply_p_ensemble(met.iloc[:30], p_struc, p_SU, p_LU, p_SC, p, dyn, overrides={nm: th[d] for d, nm in enumerate(res['names'][:3])},
                                   quantiles=Q_BAND, predictive_series=['Q_cumecs'], predictive_m={'Q_cumecs': th[3]},
                                   predictive_seed=SEED_PUB, predictive_day0=0, keep_daily=False)
    assert np.array_equal(bits(ens['predictive']['param_only']['data']), bits(fc['param_only'][:, :, :30]))
    assert np.array_equal(bits(ens['predictive']['overall']['data']), bits(fc['overall'][:, :, :30]))


def test_public_two_calls_joined_by_state_equal_the_single_call(engine0, year):
    res, _, _ = year
    first, _, _ = public(days=slice(0, 150))
    second, _, _ = public(days=slice(150, None), state=first['state'], seed=999)         # the state's seed holds
    for k in ('ess', 'log_evidence', 'resampled', 'n_unique', 'n_outside'):
        assert np.array_equal(np.concatenate([first[k], second[k]]), res[k]), k
    for k in ('inc', 'q', 'ancestors', 'theta_after'):
        assert all(np.array_equal(a, b) for a, b in zip(first[k] + second[k], res[k])), k
    assert np.array_equal(bits(second['theta']), bits(res['theta'])) and np.array_equal(bits(second['state']['data']), bits(res['state']['data']))
    assert second['state']['t'] == res['state']['t'] and second['state']['day'] == 366
    for k in ('param_only', 'overall'):
        assert np.array_equal(bits(np.concatenate([first['forecast'][k], second['forecast'][k]], axis=2)), bits(res['forecast'][k])), k
    again, _, _ = public(days=slice(0, 60))
    other, _, _ = public(days=slice(0, 60), seed=SEED_PUB + 1)
    assert np.array_equal(again['theta'], first['theta_after'][1]) and not np.array_equal(other['theta'], again['theta'])


def test_public_errors(engine0):
    for kw, msg in ((dict(resample_threshold=0.5), 'resample_threshold >= 1'), (dict(n_particles=None), 'n_particles'),
                    (dict(n_particles=0), 'particles'), (dict(rejuvenate='shake'), 'rejuvenate'), (dict(delta=0.2), 'delta'),
                    (dict(start=np.zeros((4, 3))), 'start must have shape'), (dict(window=0), 'window'),
                    (dict(forecast_series=['nonsense']), 'forecast_series'), (dict(quantiles=[1.5]), 'quantiles'),
                    (dict(variables=['Q', 'nonsense']), 'variables'), (dict(priors={'nonsense': (0, 1)}, error_m={'Q': 0.2}), 'unknown parameter'),
                    (dict(quantiles=None, forecast_series=['Q_cumecs']), 'needs quantiles'), (dict(seed=-1), 'seed')):
        with pytest.raises(ValueError, match=msg):
            public(days=slice(0, 60), **kw)
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
    with pytest.raises(ValueError, match='obs_dict'):
        sp.assimilate(met, p_struc, p_SU, p_LU, p_SC, p, dyn, None, {'fc': (200.0, 380.0)}, error_m={'Q': 0.2}, n_particles=8)
    # every particle dead: an error model that allows no misfit at all
    with pytest.raises(RuntimeError, match=r'every particle is dead in window 0 \(2004-01-01 to 2004-01-30\)'):
        public(days=slice(0, 60), priors={'fc': (200.0, 380.0)}, error_m={'Q': 0.0}, quantiles=None)
    # fewer resamplings, plain jitter, no move: the filter still runs, and the log weights carry over where it does not resample
    lazy, _, _ = public(days=slice(0, 90), resample_threshold=0.05, quantiles=None, rejuvenate={'fc': 0.01})
    assert len(lazy['ess']) == 3 and np.isfinite(lazy['log_evidence']).all() and (lazy['ess'] >= 1).all()
    carried = ~lazy['resampled']
    assert not lazy['log_weights'].any() if lazy['resampled'][-1] else lazy['log_weights'].any()
    assert (lazy['n_unique'][carried] == E_PUB).all() and not lazy['n_outside'][carried].any()
    still, _, _ = public(days=slice(0, 60), quantiles=None, rejuvenate=None)
    assert len(np.unique(still['theta'][0])) <= still['n_unique'][-1] < E_PUB and not still['n_outside'].any()
