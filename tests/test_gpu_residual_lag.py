"""The lag-one sums (simplyp_gof_lag), the AR(1) log-probability (simplyp_mcmc_log_prob_ar1) and the public calls that use them,
against the NumPy statement simplyp_amd/residuals.py.

Tables built by hand, in the manner of test_gpu_gof_synthetic.py: 130 days, two output reaches with different observations, day
lists long enough to be cut into slices, NaN simulated values for a few members only.  n_link is exact; A, B, C lie within the
bound tests/residual_lag_bounds.py derives (the statement's terms added with math.fsum); a log-probability within the bound it
derives from sp_log's pinned error.  Then Tarland 2004 through sample_posterior, find_map and run_simply_p_ensemble."""

import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import helpers
import residual_lag_bounds as rb
import simplyp_amd as sp
from simplyp_amd import abi, engine, marshal, mcmc, neldermead as nm, residuals, visualise_results as vr
from oracle import gof as ogof

pytestmark = pytest.mark.gpu

FLUX = ['Qr', 'Msus_kg/day', 'TDP_kg/day', 'PP_kg/day']
MASK = marshal.mask_of_columns(FLUX)
V = {v: i for i, v in enumerate(abi.GOF_VARS)}
ST = {s: i for i, s in enumerate(abi.GOF_STATS)}
LG = {s: i for i, s in enumerate(abi.LAG_STATS)}
D, R = 130, 2
NAME = 'tarland_2004_dynamic'
SENTINEL = -777.25


def dev(eng, a, dtype=torch.float64):
    return eng.to_device(np.ascontiguousarray(a), dtype)


def reach_params(A):
    rp = np.ones((len(marshal.PR_NAMES),) + A.shape)
    rp[marshal.PR_NAMES.index('A_catch')] = A
    return rp


def simulated(tab, A, f, r):
    with np.errstate(all='ignore'):
        return ogof.simulated_series(*[tab[c, :, r, :] for c in range(4)], A[r], f)


def day_lists(obs):
    """Per reach, the discharge days and the chemistry days of the device's lists (variables with more than 10 observations)."""
    out = []
    for r in range(obs.shape[0]):
        use = (~np.isnan(obs[r])).sum(axis=1) > 10
        q = np.flatnonzero(~np.isnan(obs[r, 0])) if use[0] else np.zeros(0, dtype=np.int64)
        c = np.flatnonzero((~np.isnan(obs[r, 1:]) & use[1:, None]).any(axis=0))
        out.append((q, c))
    return out


def n_slices(lists, which):
    """simplyp_gof's rule where the waves of one slice fit the chip many times over: as many slices as leave 32 days per slice and reach."""
    return max(1, min(64, sum(len(l[which]) for l in lists) // len(lists) // 32))


def slice_starts(days, n):
    return [len(days) * c // n for c in range(n)]


def rereads(lists, which, n):
    """The slices whose first day continues a segment."""
    k = 0
    for l in lists:
        days = l[which]
        for c in range(n):
            b, e = len(days) * c // n, len(days) * (c + 1) // n
            k += int(b < e and b > 0 and days[b] == days[b - 1] + 1)
    return k


@functools.lru_cache(maxsize=None)
def case(E):
    """The table [4, D, 2, E], A [2, E], f [E], obs [2, 6, D] and where the NaN simulated values were put."""
    rng = np.random.default_rng(7000 + E)
    tab = np.stack([rng.uniform(0.2, 3.0, (D, R, E)), rng.uniform(5.0, 500.0, (D, R, E)),
                    rng.uniform(0.02, 0.5, (D, R, E)), rng.uniform(0.05, 1.0, (D, R, E))])
    A, f = rng.uniform(20.0, 120.0, (R, E)), rng.uniform(0.4, 0.95, E)
    days = np.arange(D)
    pattern = [dict(Q=days,                                                        # every day: a link straddles every slice boundary
                    SS=days[5:105],
                    TDP=np.r_[3:61, 110, 120:127],                                 # day 110: TDP observed, SS not
                    PP=days[::2],                                                  # 65 observations and not one link
                    TP=days[days % 7 < 3],                                         # runs of three days
                    SRP=days[30:40]),                                              # exactly 10: NaN rows
               dict(Q=days[(days % 11 != 0) & (days % 11 != 5)],                   # gappy, row 0 missing
                    SS=days[40:], TDP=days[:51])]
    obs = np.full((R, 6, D), np.nan)
    for r in range(R):
        sim = simulated(tab, A, f, r)
        for v, dd in pattern[r].items():
            obs[r, V[v], dd] = sim[v][dd, 0] * rng.uniform(0.7, 1.4, len(dd))
    lists = day_lists(obs)
    nq, nc = n_slices(lists, 0), n_slices(lists, 1)
    assert nq >= 2 and nc >= 2
    # NaN simulated values, per member class e % 5: inside a segment, on a slice's first day, on the day before one, on row 0
    q0, c0 = lists[0]
    first_q, first_c = q0[slice_starts(q0, nq)[1]], c0[slice_starts(c0, nc)[1]]
    before_q = q0[slice_starts(q0, nq)[-1]] - 1
    assert before_q in q0 and first_c - 1 in c0
    e = np.arange(E)
    where = {'inside a segment': (20, e % 5 == 0), "on a slice's first day": (first_q, e % 5 == 1),
             'on the day before a slice': (before_q, e % 5 == 2), 'on row 0': (0, e % 5 == 3)}
    for d, members in where.values():
        tab[0, d, 0, members] = np.nan                                             # Qr: every variable of the day
    tab[2, first_c, 0, e % 3 == 0] = np.nan                                        # the TDP flux alone: TDP, TP and SRP, not SS or PP
    tab[0, 60, 1, e % 4 == 1] = np.nan
    tab.setflags(write=False); obs.setflags(write=False)
    return tab, A, f, obs, lists, (nq, nc)


@functools.lru_cache(maxsize=None)
def reference(E):
    """Per (stat, variable, reach, member): the statement's sums added with math.fsum, and their bounds; also SUM_RELSQ's pieces."""
    tab, A, f, obs, _, _ = case(E)
    want = np.full((4, 6, R, E), np.nan)
    bound = np.full((4, 6, R, E), np.nan)
    unlinked = np.full((6, R, E), np.nan)
    relsq_bound = np.full((6, R, E), np.nan)
    for r in range(R):
        sim = simulated(tab, A, f, r)
        for v, vi in V.items():
            if (~np.isnan(obs[r, vi])).sum() <= 10:
                continue
            paired, rr, link = residuals.lag_terms(obs[r, vi], sim[v])
            linked_row = np.concatenate([np.zeros((1, E), dtype=bool), link])
            for e in range(E):
                at = np.flatnonzero(link[:, e])
                head, tail = rr[1:][at, e], rr[:-1][at, e]
                want[:, vi, r, e] = [len(at), math.fsum(head * head), math.fsum(tail * tail), math.fsum(head * tail)]
                bound[1:, vi, r, e] = rb.lag_bounds(head, tail)
                bound[0, vi, r, e] = 0.0
                lone = rr[paired[:, e] & ~linked_row[:, e], e]
                unlinked[vi, r, e] = math.fsum(lone * lone)
                relsq_bound[vi, r, e] = rb.relsq_bound(rr[paired[:, e], e])
    return want, bound, unlinked, relsq_bound


def device_lag(engine0, E, permuted=False):
    tab, A, f, obs, _, _ = case(E)
    mos = None
    if permuted:
        perm = np.random.default_rng(E).permutation(E).astype(np.int32)
        tab, mos = tab[..., perm], dev(engine0, perm, torch.int32)
    t = dev(engine0, tab)
    lag, info = engine0.gof_lag(t, MASK, obs, f, reach_params(A), member_of_slot=mos)
    gof, ginfo = engine0.gof(t, MASK, obs, f, reach_params(A), member_of_slot=mos)
    return lag, info, gof, ginfo


# ---- the sums ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('E', [1, 63, 64, 65, 130])
def test_lag_sums_against_the_statement(engine0, E):
    tab, A, f, obs, lists, (nq, nc) = case(E)
    want, bound, unlinked, relsq_bound = reference(E)
    lag_d, info, gof_d, ginfo = device_lag(engine0, E)
    lag, gof = lag_d.cpu().numpy(), gof_d.cpu().numpy()
    # the slices: a link straddles every boundary of the every-day discharge list
    assert info['n_chunks_q'] == nq >= 2 and info['n_chunks_chem'] == nc >= 2
    assert (info['n_q_days'], info['n_chem_days']) == (ginfo['n_q_days'], ginfo['n_chem_days']) \
        == (sum(len(l[0]) for l in lists), sum(len(l[1]) for l in lists))
    assert (ginfo['n_chunks_q'], ginfo['n_chunks_chem']) == (nq, nc)
    rq, rc = rereads(lists, 0, nq), rereads(lists, 1, nc)
    assert rq >= nq - 1 and rc >= 1
    assert info['bytes_read'] == ginfo['bytes_read'] + (8 * rq + 32 * rc) * E
    # NaN rows exactly where the variable has 10 or fewer observations
    assert np.array_equal(np.isnan(lag), np.isnan(want))
    assert np.isnan(lag[:, V['SRP'], 0]).all() and np.isnan(lag[:, V['PP'], 1]).all() and not np.isnan(lag[:, V['Q']]).any()
    used = ~np.isnan(want)
    assert np.array_equal(lag[0][used[0]], want[0][used[0]])                       # n_link: exact
    assert (lag[:, V['PP'], 0] == 0.0).all()                                       # observed every second day: no link, sums exactly 0
    err = np.abs(lag - want)
    assert (err[used] <= bound[used]).all(), np.argwhere(used & ~(err <= bound))[:8].tolist()
    with np.errstate(invalid='ignore', divide='ignore'):
        frac = np.where(used & (bound > 0), err / bound, 0.0)
    print('E = %d: largest |device - statement| / bound = %.3f (A %.3f, B %.3f, C %.3f)'
          % (E, frac.max(), frac[1].max(), frac[2].max(), frac[3].max()))
    # the lane-divergent breaks are there: the member classes differ in n_link of the every-day discharge series
    n0 = want[0, V['Q'], 0]
    clean = D - 1
    for e in range(E):
        assert n0[e] == {0: clean - 2, 1: clean - 2, 2: clean - 2, 3: clean - 1, 4: clean}[e % 5], e
    # r is simplyp_gof's: the linked squares and the statement's unlinked ones make up the device's SUM_RELSQ
    u = used[0]
    total = lag[LG['sq_head']] + unlinked
    assert (np.abs(total - gof[ST['sum_relsq']])[u] <= relsq_bound[u]).all()
    assert np.array_equal(gof[ST['N obs']][u] > 10, np.ones(int(u.sum()), dtype=bool))


@pytest.mark.parametrize('E', [63, 65, 130])
def test_lag_sums_follow_the_member_not_the_slot(engine0, E):
    lag, _, _, _ = device_lag(engine0, E)
    lag_p, _, _, _ = device_lag(engine0, E, permuted=True)
    assert np.array_equal(lag.cpu().numpy(), lag_p.cpu().numpy(), equal_nan=True)


def test_lag_writes_into_a_given_tensor_and_checks_its_shape(engine0):
    tab, A, f, obs, _, _ = case(1)
    t = dev(engine0, tab)
    mine = torch.full((4, 6, R, 1), SENTINEL, dtype=torch.float64, device=engine0.tdev)
    got, _ = engine0.gof_lag(t, MASK, obs, f, reach_params(A), lag=mine)
    assert got is mine and not bool((mine == SENTINEL).any())
    with pytest.raises(ValueError, match='lag must be a contiguous float64 tensor'):
        engine0.gof_lag(t, MASK, obs, f, reach_params(A), lag=torch.zeros((4, 6, R, 2), dtype=torch.float64, device=engine0.tdev))
    with pytest.raises(ValueError, match='obs must have shape'):
        engine0.gof_lag(t, MASK, obs[:, :, :-1], f, reach_params(A))


# ---- the log-probability ----------------------------------------------------------------------------------------------------

PAIRS = [(V['Q'], 0), (V['Q'], 1), (V['SS'], 0), (V['TDP'], 1)]
M_DIM, M_CONST = [0, -1, -1, -1, -1, -1], [np.nan, 0.35, 0.2, np.nan, np.nan, np.nan]


@pytest.fixture(scope='module')
def tables(engine0):
    E = 65
    lag, _, gof, _ = device_lag(engine0, E)
    rng = np.random.default_rng(65)
    prop = np.stack([rng.uniform(0.05, 0.9, E), np.zeros(E), rng.uniform(-0.95, 0.95, E)])      # m_Q, a phi of 0, a phi
    return E, gof, lag, gof.cpu().numpy(), lag.cpu().numpy(), prop


def statement(g, lg, prop, phi_of):
    """(sum over PAIRS of residuals.loglik_ar1, the bound of the device's value) from the downloaded tables."""
    want, tol = 0.0, 0.0
    for v, r in PAIRS:
        m = prop[0] if M_DIM[v] >= 0 else M_CONST[v]
        a = (g[ST['N obs'], v, r], g[ST['sum_log_sim'], v, r], g[ST['sum_relsq'], v, r], lg[0, v, r], lg[1, v, r], lg[2, v, r],
             lg[3, v, r], m, phi_of(v))
        term = residuals.loglik_ar1(*a)
        want = want + term
        tol = tol + rb.loglik_bound(*a) + rb.U * np.abs(want)
    return want, tol


def test_log_prob_ar1_at_phi_zero_is_log_prob_bit_for_bit(engine0, tables):
    E, gof, lag, g, lg, prop = tables
    prop_d = dev(engine0, prop)
    inside = np.ones(E, dtype=np.int32); inside[[0, 33]] = 0
    st = np.zeros(E, dtype=np.int32); st[7] = abi.STATUS_NONFINITE; st[8] = abi.STATUS_STEPCAP
    prop2 = prop.copy(); prop2[0, 5], prop2[0, 6] = 0.0, -0.1
    for p_d, kw in ((prop_d, {}), (dev(engine0, prop2), dict(status=dev(engine0, st, torch.int32), inside=dev(engine0, inside, torch.int32)))):
        lp0 = torch.full((E,), SENTINEL, dtype=torch.float64, device=engine0.tdev)
        info0 = engine0.mcmc_log_prob(gof, PAIRS, M_DIM, M_CONST, p_d, lp0, **kw)
        want = lp0.cpu().numpy()
        for phi_dim, phi_const in (([-1] * 6, [0.0] * 6), ([1, -1, 1, -1, -1, -1], [0.7, 0.0, 0.7, 0.0, 0.0, 0.0]),
                                   ([1] * 6, [0.0] * 6), ([-1] * 6, [-0.0] * 6)):
            lp = torch.full((E,), SENTINEL, dtype=torch.float64, device=engine0.tdev)
            info = engine0.mcmc_log_prob_ar1(gof, lag, PAIRS, M_DIM, M_CONST, phi_dim, phi_const, p_d, lp, **kw)
            assert np.array_equal(lp.cpu().numpy().view(np.uint64), want.view(np.uint64)), (phi_dim, phi_const)
            assert (info['n_inside'], info['n_nan'], info['n_accepted']) == (info0['n_inside'], info0['n_nan'], 0)
        if kw:
            assert (want[[0, 33, 5, 6, 7]] == -np.inf).all() and np.isfinite(np.delete(want, [0, 33, 5, 6, 7])).all()
        else:
            assert np.isfinite(want).all()


@pytest.mark.parametrize('phi', [-0.9, 0.3, 0.99])
def test_log_prob_ar1_against_the_statement(engine0, tables, phi):
    E, gof, lag, g, lg, prop = tables
    prop_d = dev(engine0, prop)
    lp = torch.full((E,), SENTINEL, dtype=torch.float64, device=engine0.tdev)
    # every variable at the constant phi; then Q's sampled (row 2 of prop) and the others' constant
    for phi_dim, phi_of in (([-1] * 6, lambda v: phi), ([2, -1, -1, -1, -1, -1], lambda v: prop[2] if v == V['Q'] else phi)):
        info = engine0.mcmc_log_prob_ar1(gof, lag, PAIRS, M_DIM, M_CONST, phi_dim, [phi] * 6, prop_d, lp)
        got = lp.cpu().numpy()
        want, tol = statement(g, lg, prop, phi_of)
        assert np.isfinite(want).all() and info['n_inside'] == E and info['n_nan'] == 0
        err = np.abs(got - want)
        print('phi = %g, phi_dim[Q] = %d: largest |device - statement| / bound = %.3f; largest relative difference %.2e'
              % (phi, phi_dim[0], (err / tol).max(), (err / np.abs(want)).max()))
        assert (err <= tol).all()
    # the lag terms matter on this table
    assert not np.allclose(want, statement(g, lg, prop, lambda v: 0.0)[0], rtol=1e-6)


def test_log_prob_ar1_is_minus_infinity_where_the_point_does_not_count(engine0, tables):
    E, gof, lag, g, lg, prop = tables
    p = np.stack([np.full(E, 0.3), np.full(E, 0.5)])
    bad_phi = {1: 1.0, 2: -1.0, 3: np.nan, 4: 1.5, 9: np.inf, 10: np.nextafter(1.0, 2.0)}
    for e, x in bad_phi.items():
        p[1, e] = x
    p[1, 11], p[1, 13] = np.nextafter(1.0, 0.0), np.nextafter(-1.0, 0.0)       # the last values inside ...
    p[1, 12] = np.nextafter(-1.0, -2.0)                                        # ... and the first outside
    p[0, 5], p[0, 6] = 0.0, -0.1
    inside = np.ones(E, dtype=np.int32); inside[[0, 33]] = 0
    st = np.zeros(E, dtype=np.int32); st[7] = abi.STATUS_NONFINITE; st[8] = abi.STATUS_STEPCAP
    lp = torch.full((E,), SENTINEL, dtype=torch.float64, device=engine0.tdev)
    pairs = [(V['Q'], 0)]
    info = engine0.mcmc_log_prob_ar1(gof, lag, pairs, [0, -1, -1, -1, -1, -1], [np.nan] * 6, [1, -1, -1, -1, -1, -1], [0.0] * 6,
                                     dev(engine0, p), lp, status=dev(engine0, st, torch.int32), inside=dev(engine0, inside, torch.int32))
    got = lp.cpu().numpy()
    bad = sorted(list(bad_phi) + [12, 5, 6, 0, 33, 7])
    assert (got[bad] == -np.inf).all()
    ok = np.setdiff1d(np.arange(E), bad)
    assert np.isfinite(got[ok]).all() and info['n_inside'] == E - 2
    v = V['Q']
    with np.errstate(all='ignore'):                                            # the statement at the lanes that do not count
        want = residuals.loglik_ar1(g[0, v, 0], g[6, v, 0], g[7, v, 0], lg[0, v, 0], lg[1, v, 0], lg[2, v, 0], lg[3, v, 0], p[0], p[1])
    assert (np.abs(got[ok] - want[ok]) <= 1e-12 * np.abs(want[ok])).all()      # the step-cap bit does not disqualify (member 8)


# ---- refusals of the two entries --------------------------------------------------------------------------------------------

def refused(engine0, entry, args, info_class):
    """(rc, message, the info's bytes) of a raw call with the info filled with 0xA5."""
    info = info_class()
    C.memset(C.byref(info), 0xA5, C.sizeof(info))
    rc = getattr(engine.lib(), entry)(*(args + (C.byref(info),)))
    return int(rc), engine.lib().simplyp_last_error(engine0._h).decode(), bytes(info)


def test_refusals_of_gof_lag(engine0):
    scratch = torch.zeros(4096, dtype=torch.float64, device=engine0.tdev)
    p = scratch.data_ptr()
    obs = np.ones((1, 6, 3))
    o = obs.ctypes.data_as(C.POINTER(C.c_double))
    qr_only = marshal.mask_of_columns(['Qr'])

    def args(E=4, S=1, D_=3, mask=MASK, out=p, f=p, rp=p, ob=o, lag=p):
        dims = abi.Dims(E, S, D_, 1)
        return (engine0._h, C.byref(dims), mask, None, 0, out, None, f, rp, ob, lag), dims

    cases = [(dict(E=0), 'bad dims'), (dict(S=0), 'bad dims'), (dict(D_=0), 'bad dims'),
             (dict(mask=qr_only), 'out_mask must contain Qr, Msus_kg/day, TDP_kg/day and PP_kg/day'),
             (dict(mask=0), 'the mask must select 1..26 of the columns'),
             (dict(out=None), 'a required pointer is NULL'), (dict(f=None), 'a required pointer is NULL'),
             (dict(rp=None), 'a required pointer is NULL'), (dict(ob=None), 'a required pointer is NULL'),
             (dict(lag=None), 'a required pointer is NULL')]
    for kw, text in cases:
        a, keep = args(**kw)
        rc, msg, info = refused(engine0, 'simplyp_gof_lag', a, abi.GofInfo)
        assert (rc, msg) == (-1, 'simplyp_gof_lag: ' + text), (kw, rc, msg)
        assert set(info) == {0xA5}, kw
    torch.cuda.synchronize()
    assert not bool(scratch.any())
    a, dims = args(E=4, S=1, D_=3, mask=0)
    assert engine.lib().simplyp_gof_lag(*(a[:1] + (None,) + a[2:] + (None,))) == -1            # dims = NULL, info = NULL
    assert engine.lib().simplyp_gof_lag(*((None,) + a[1:] + (None,))) == -1                    # a NULL context


def test_refusals_of_log_prob_ar1(engine0):
    scratch = torch.zeros(4096, dtype=torch.float64, device=engine0.tdev)
    p = scratch.data_ptr()
    i32, dbl = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    keep = []

    def hi(*v):
        keep.append(np.ascontiguousarray(v, dtype=np.int32))
        return keep[-1].ctypes.data_as(i32)

    def hd(*v):
        keep.append(np.ascontiguousarray(v, dtype=np.float64))
        return keep[-1].ctypes.data_as(dbl)

    def args(W=4, n_dim=1, n_or=1, gof=p, lag=p, pv=(0,), pr=(0,), n_pairs=1, m_dim=(-1,) * 6, phi_dim=(-1,) * 6,
             phi_const=(0.0,) * 6, prop=p, lp=p, null=None):
        a = dict(pv=hi(*pv), pr=hi(*pr), m_dim=hi(*m_dim), m_const=hd(*([0.1] * 6)), phi_dim=hi(*phi_dim), phi_const=hd(*phi_const))
        if null:
            a[null] = None
        return (engine0._h, W, n_dim, n_or, gof, lag, None, None, a['pv'], a['pr'], n_pairs, a['m_dim'], a['m_const'], a['phi_dim'],
                a['phi_const'], prop, lp)

    nulls = 'gof, lag, pair_var, pair_reach, m_dim, m_const, phi_dim, phi_const, prop and lp_prop must not be NULL'
    nan = float('nan')
    cases = [(dict(n_dim=0), 'n_dim must be in [1, 16] (got 0)'), (dict(n_dim=17, W=40), 'n_dim must be in [1, 16] (got 17)'),
             (dict(W=3), 'W must be even and >= 2 n_dim (got W = 3, n_dim = 1)'),
             (dict(n_or=0), 'n_out_reaches must be >= 1 (got 0)'),
             (dict(n_pairs=0), 'n_pairs must be in [1, 32] (got 0)'), (dict(n_pairs=33), 'n_pairs must be in [1, 32] (got 33)'),
             (dict(m_dim=(1, -1, -1, -1, -1, -1)), 'm_dim[0] = 1 is neither -1 nor a row of prop'),
             (dict(phi_dim=(1, -1, -1, -1, -1, -1)), 'phi_dim[0] = 1 is neither -1 nor a row of prop'),
             (dict(phi_dim=(-1, -1, -2, -1, -1, -1)), 'phi_dim[2] = -2 is neither -1 nor a row of prop'),
             (dict(phi_const=(1.0, 0, 0, 0, 0, 0)), 'phi_const[0] = 1 is not inside (-1, 1)'),
             (dict(phi_const=(-1.0, 0, 0, 0, 0, 0)), 'phi_const[0] = -1 is not inside (-1, 1)'),
             (dict(phi_const=(nan, 0, 0, 0, 0, 0)), 'phi_const[0] = nan is not inside (-1, 1)'),
             (dict(pv=(2,), phi_const=(0, 0, 1.5, 0, 0, 0)), 'phi_const[2] = 1.5 is not inside (-1, 1)'),
             (dict(gof=None), nulls), (dict(lag=None), nulls), (dict(prop=None), nulls), (dict(lp=None), nulls),
             (dict(null='phi_dim'), nulls), (dict(null='phi_const'), nulls), (dict(null='pv'), nulls), (dict(null='m_const'), nulls)]
    for kw, text in cases:
        rc, msg, info = refused(engine0, 'simplyp_mcmc_log_prob_ar1', args(**kw), abi.McmcInfo)
        assert (rc, msg) == (-1, 'simplyp_mcmc_log_prob_ar1: ' + text), (kw, rc, msg)
        assert set(info) == {0xA5}, kw
    for kw, name in ((dict(pv=(6,)), 'pair_var'), (dict(pr=(1,)), 'pair_reach')):
        rc, msg, info = refused(engine0, 'simplyp_mcmc_log_prob_ar1', args(**kw), abi.McmcInfo)
        assert rc == -1 and msg.startswith('simplyp_mcmc_log_prob_ar1: ') and set(info) == {0xA5}, (kw, msg)
    torch.cuda.synchronize()
    assert not bool(scratch.any())
    # a phi_const outside (-1, 1) is no matter for a variable that is not in pair_var, or whose phi is sampled
    lp = torch.full((2,), SENTINEL, dtype=torch.float64, device=engine0.tdev)
    gof = torch.ones((8, 6, 1, 2), dtype=torch.float64, device=engine0.tdev)
    lag = torch.ones((4, 6, 1, 2), dtype=torch.float64, device=engine0.tdev)
    prop = torch.full((1, 2), 0.25, dtype=torch.float64, device=engine0.tdev)
    engine0.mcmc_log_prob_ar1(gof, lag, [(0, 0)], [-1] * 6, [0.5] * 6, [0, -1, -1, -1, -1, -1], [7.0, nan, 2.0, 0, 0, 0], prop, lp)
    assert np.isfinite(lp.cpu().numpy()).all()
    with pytest.raises(ValueError, match='lag .* does not match gof'):
        engine0.mcmc_log_prob_ar1(gof, lag[:, :, :, :1].contiguous(), [(0, 0)], [-1] * 6, [0.5] * 6, [-1] * 6, [0.0] * 6, prop, lp)


def test_both_entries_refuse_while_a_run_is_pending(engine0):
    """As every analysis entry does (test_gpu_pending.py): between Engine.run(defer_sync=True) and its finish() the two entries
    return SIMPLYP_ERR_ARG with the entry frame's text, launch nothing and leave the info they were handed as it was."""
    m = helpers.marshal_scenario('tarland_2004_static', E=64)
    args = (m['forcing'], m['doy'], m['member_params'], m['reach_params'], m['up_ptr'], m['up_idx'], m['opts'])
    ref, _, _ = engine0.run(*args)
    scratch = torch.zeros(4096, dtype=torch.float64, device=engine0.tdev)
    p = scratch.data_ptr()
    torch.cuda.synchronize()
    obs = np.ones((1, 6, 3))
    dims = abi.Dims(4, 1, 3, 1)
    i6, d6, one = np.full(6, -1, dtype=np.int32), np.zeros(6), np.zeros(1, dtype=np.int32)
    i32, dbl = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    calls = {'simplyp_gof_lag': ((engine0._h, C.byref(dims), MASK, None, 0, p, None, p, p, obs.ctypes.data_as(dbl), p), abi.GofInfo),
             'simplyp_mcmc_log_prob_ar1': ((engine0._h, 4, 1, 1, p, p, None, None, one.ctypes.data_as(i32), one.ctypes.data_as(i32), 1,
                                            i6.ctypes.data_as(i32), d6.ctypes.data_as(dbl), i6.ctypes.data_as(i32), d6.ctypes.data_as(dbl),
                                            p, p), abi.McmcInfo)}
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out, status, st = engine0.run(*args, defer_sync=True)
        for entry, (a, info_class) in calls.items():
            rc, msg, info = refused(engine0, entry, a, info_class)
            assert (rc, msg) == (-1, '%s: a run is pending on this context; call simplyp_sync first' % entry)
            assert set(info) == {0xA5}, entry
        st.update(st.pop('finish')())
    s.synchronize()
    assert not bool(scratch.any()) and bool(torch.equal(out, ref))


# ---- the public calls: Tarland 2004 -----------------------------------------------------------------------------------------

W_PUB, STEPS_PUB, SEED_PUB = 8, 3, 11
KEYS_TODAY = {'wall_ms', 'run_kernel_ms', 'gof_ms', 'sampler_ms', 'n_inside', 'n_accepted', 'start_wall_ms', 'start_run_kernel_ms'}


def inputs():
    got = helpers.scenario_inputs(NAME)
    return got, helpers.observations(got[2]['st_dt'], got[2]['end_dt'])


def posterior(**kw):
    (met, p_struc, p_SU, p_LU, p_SC, p, dyn), obs_dict = inputs()
    priors = {'fc': (0.7 * float(p['fc']), 1.3 * float(p['fc'])), 'm_Q': (0.05, 1.0), 'phi_Q': (-0.5, 0.95)}
    args = dict(priors=priors, variables=['Q'], n_walkers=W_PUB, n_steps=STEPS_PUB, seed=SEED_PUB, record_proposals=True)
    args.update(kw)
    return sp.sample_posterior(met, p_struc, p_SU, p_LU, p_SC, p, dyn, obs_dict, **args), args['priors'], obs_dict


@pytest.fixture(scope='module')
def res3(engine0):
    return posterior()


def test_posterior_chain_is_the_mirrors_replay_of_the_recorded_proposals(engine0, res3):
    res, priors, _ = res3
    assert res['names'] == ['fc', 'm_Q', 'phi_Q'] and res['chain'].shape == (STEPS_PUB, 3, W_PUB)
    h = W_PUB // 2
    lo = np.array([priors[n][0] for n in res['names']]); hi = np.array([priors[n][1] for n in res['names']])
    calls = iter([(n, k) for n in range(STEPS_PUB) for k in (0, 1)])

    def recorded(points):
        n, k = next(calls)
        lp_y = res['proposal_log_prob'][n, k * h:(k + 1) * h]
        ran = np.isfinite(lp_y)
        assert np.array_equal(points[:, ran], res['proposals'][n, :, k * h:(k + 1) * h][:, ran])
        return lp_y

    st = res['start']
    assert st['theta'][2, 0] != 0.0 and abs(st['theta'][2].mean() - 0.5 * (-0.5 + 0.95)) < 1e-3       # phi starts at its box's centre
    rep = mcmc.run_chain(recorded, st['theta'], st['lp'], STEPS_PUB, lo, hi, seed=SEED_PUB, t0=st['t'])
    assert rep['min_abs_margin'] > 1e-9, rep['min_abs_margin']
    assert np.array_equal(rep['chain'], res['chain']) and np.array_equal(rep['log_prob'], res['log_prob'])
    assert rep['n_inside'] == res['stats']['n_inside'] and rep['n_accepted'] == res['stats']['n_accepted']
    assert set(res['stats']) == KEYS_TODAY | {'lag_ms'} and len(res['stats']['lag_ms']) == 2 * STEPS_PUB
    assert min(res['stats']['lag_ms']) > 0.0
    assert list(res['error_phi']) == ['Q_cumecs'] and np.array_equal(res['error_phi']['Q_cumecs'], res['state']['theta'][2])
    assert list(res['error_m']) == ['Q_cumecs'] and sorted(res['overrides']) == ['fc']


def test_posterior_log_probabilities_are_the_statement_on_an_ensemble_runs_sums(engine0, res3):
    res, priors, obs_dict = res3
    flat = res['proposals'].transpose(1, 0, 2).reshape(3, -1)                       # [n_dim, steps * W]
    got = res['proposal_log_prob'].reshape(-1)
    ran = np.isfinite(got)
    assert ran.sum() >= len(got) // 2
    (met, p_struc, p_SU, p_LU, p_SC, p, dyn), _ = inputs()
    fc = np.where(ran, flat[0], float(p['fc']))                                     # a proposal outside the box was never run
    ens = sp.run_simply_p_ensemble(met, p_struc, p_SU, p_LU, p_SC, p, dyn, overrides={'fc': fc}, obs_dict=obs_dict,
                                   keep_daily=False, residual_lag=True)
    assert int(ens['status'].max()) == 0
    g, lag, q = ens['gof']['data'], ens['residual_lag'], V['Q']
    a = (g[ST['N obs'], q, 0], g[ST['sum_log_sim'], q, 0], g[ST['sum_relsq'], q, 0], lag['n_link'][q, 0], lag['sq_head'][q, 0],
         lag['sq_tail'][q, 0], lag['cross'][q, 0], np.where(ran, flat[1], 0.5), np.where(ran, flat[2], 0.0))
    want, tol = residuals.loglik_ar1(*a), rb.loglik_bound(*a)
    err = np.abs(got - want)[ran]
    print('largest |recorded - statement| / bound = %.3f' % (err / tol[ran]).max())
    assert (err <= tol[ran]).all()
    assert (lag['n_link'][q, 0] == 356.0).all()                                     # the shipped record's consecutive-day pairs in 2004
    assert np.allclose(lag['phi_hat'][q, 0], lag['cross'][q, 0] / lag['sq_tail'][q, 0], rtol=0, atol=0)
    assert ((lag['phi_hat'][q, 0] > 0.0) & (lag['phi_hat'][q, 0] < 1.0)).all()      # the autocorrelation the error model is for


def test_posterior_continues_from_its_state_and_takes_a_fixed_phi(engine0, res3):
    res, _, _ = res3
    first, _, _ = posterior(n_steps=2)
    second, _, _ = posterior(n_steps=1, state=first['state'])
    assert np.array_equal(first['chain'], res['chain'][:2]) and np.array_equal(second['chain'], res['chain'][2:])
    assert np.array_equal(second['log_prob'], res['log_prob'][2:]) and np.array_equal(second['state']['theta'], res['state']['theta'])
    (met, p_struc, p_SU, p_LU, p_SC, p, dyn), obs_dict = inputs()
    pri = {'fc': (0.7 * float(p['fc']), 1.3 * float(p['fc'])), 'm_Q': (0.05, 1.0)}
    fixed, _, _ = posterior(priors=pri, error_phi={'Q': 0.6}, n_steps=1)
    plain, _, _ = posterior(priors=pri, n_steps=1)
    assert set(fixed['stats']) == KEYS_TODAY | {'lag_ms'} and np.array_equal(fixed['error_phi']['Q_cumecs'], np.full(W_PUB, 0.6))
    assert set(plain['stats']) == KEYS_TODAY and plain['error_phi'] == {}           # without a phi: exactly today's keys
    assert np.array_equal(fixed['start']['theta'], plain['start']['theta']) and not np.array_equal(fixed['start']['lp'], plain['start']['lp'])
    zero, _, _ = posterior(priors=pri, error_phi={'Q': 0.0}, n_steps=1)             # phi = 0 through the AR(1) entries: the same chain
    assert np.array_equal(zero['chain'], plain['chain']) and np.array_equal(zero['log_prob'], plain['log_prob'])


def test_find_map_with_phi_is_the_mirrors_replay(engine0):
    (met, p_struc, p_SU, p_LU, p_SC, p, dyn), obs_dict = inputs()
    priors = {'fc': (0.7 * float(p['fc']), 1.3 * float(p['fc'])), 'm_Q': (0.05, 1.0), 'phi_Q': (-0.5, 0.95)}
    res = sp.find_map(met, p_struc, p_SU, p_LU, p_SC, p, dyn, obs_dict, priors, variables=['Q'], n_starts=4, max_iter=4, seed=5,
                      record_evaluations=True)
    lo = np.array([priors[n][0] for n in res['names']]); hi = np.array([priors[n][1] for n in res['names']])
    runs = iter(range(len(res['evaluations'])))

    def recorded(points):
        k = next(runs)
        lp = res['evaluation_log_prob'][k]
        ran = np.isfinite(lp)
        assert np.array_equal(points[:, ran], res['evaluations'][k][:, ran])
        return -lp

    rep = nm.run(recorded, None, lo, hi, max_iter=4, state=res['start'])
    assert rep['n_runs'] == len(res['evaluations'])
    assert np.array_equal(rep['sim'], res['final_simplex'][0]) and np.array_equal(rep['fsim'], res['final_simplex'][1])
    assert np.array_equal(rep['n_iter'], res['n_iter']) and np.array_equal(rep['status'], res['status'])
    assert np.array_equal(rep['history'], res['history'], equal_nan=True)
    assert 'lag_ms' in res['stats'] and len(res['stats']['lag_ms']) == len(res['stats']['gof_ms'])
    assert list(res['error_phi']) == ['Q_cumecs'] and res['error_phi']['Q_cumecs'][0] == res['x'][2, res['best']] == res['map']['phi_Q']
    assert res['start']['sim'][0][2, 0] == 0.5 * (-0.5 + 0.95)                      # simplex 0 starts phi at its box's centre


def test_ensemble_residual_lag(engine0):
    (met, p_struc, p_SU, p_LU, p_SC, p, dyn), obs_dict = inputs()
    E = 16
    factor = np.random.default_rng(16).uniform(0.85, 1.15, E)
    kw = dict(overrides={'fc': float(p['fc']) * factor}, obs_dict=obs_dict, residual_lag=True)
    run = lambda **more: sp.run_simply_p_ensemble(*inputs()[0], **dict(kw, **more))
    one = run()
    lag = one['residual_lag']
    assert lag['variables'] == abi.GOF_VARS and set(lag) == set(abi.LAG_STATS) | {'variables', 'phi_hat', 'info'}
    assert all(lag[k].shape == (6, 1, E) for k in abi.LAG_STATS + ['phi_hat']) and one['data'] is not None
    # the direct entry on a table of its own
    m = helpers.marshal_scenario(NAME, E=E, out_mask=MASK)
    m['member_params'][marshal.PM_NAMES.index('fc')] = float(p['fc']) * factor
    out, status, _ = engine0.run(m['forcing'], m['doy'], m['member_params'], m['reach_params'], m['up_ptr'], m['up_idx'], m['opts'])
    obs = vr.observation_array(obs_dict, [1], m['met'].index)
    direct, dinfo = engine0.gof_lag(out, MASK, obs, float(p['f_TDP']), m['reach_params'])
    direct = direct.cpu().numpy()
    for i, k in enumerate(abi.LAG_STATS):
        assert np.array_equal(lag[k], direct[i], equal_nan=True), k
    assert lag['info']['n_q_days'] == dinfo['n_q_days'] == 360 and lag['info']['n_chunks_q'] == dinfo['n_chunks_q']
    with np.errstate(all='ignore'):
        assert np.array_equal(lag['phi_hat'], direct[3] / direct[2], equal_nan=True)
    assert (lag['n_link'][V['Q'], 0] == 356.0).all()
    # two member blocks, and without the table kept: the same bits
    for other in (run(devices=[0, 0]), run(keep_daily=False)):
        for k in abi.LAG_STATS + ['phi_hat']:
            assert np.array_equal(other['residual_lag'][k], lag[k], equal_nan=True), k
    assert run(keep_daily=False)['data'] is None
    # on the device, and per window: a link does not cross a window's edge
    on_dev = run(to_host=False)['residual_lag']
    assert torch.is_tensor(on_dev['phi_hat']) and np.array_equal(on_dev['phi_hat'].cpu().numpy(), lag['phi_hat'], equal_nan=True)
    wins = list(sp.run_simply_p_ensemble_windows(*inputs()[0], window=183, **kw))
    assert len(wins) == 2
    q_obs = ~np.isnan(obs[0, 0])
    cut = int(q_obs[182] and q_obs[183])
    assert np.array_equal(sum(w['residual_lag']['n_link'][V['Q'], 0] for w in wins), lag['n_link'][V['Q'], 0] - cut)
    no = sp.run_simply_p_ensemble(*inputs()[0], overrides=kw['overrides'], obs_dict=obs_dict)
    assert 'residual_lag' not in no
