"""The goodness-of-fit family (simplyp_gof, simplyp_gof_spearman, simplyp_waterbody, simplyp_gof_waterbody) on tables built by
hand -- no model run -- so that the corners a model-made table never reaches are reached: values on either side of the
1e-290 / 1e290 switch between the device's own log / reciprocal and libm's, zero / negative / infinite / NaN values on single
days, observations that are 0 or negative, A_catch and f_TDP that differ per member under a permuted slot order, day lists at
the edges of the load batches (8 discharge days, 4 chemistry days) and of the Spearman tile (32), and ill-conditioned r2.

Two references.  The numpy oracle (oracle/gof.py, oracle/waterbody.py) for every member: it defines the NaN / inf semantics.
An exact one (mpmath, 40 digits, from the fp64 table without intermediate rounding) on a few members: before the device is
compared, every test holds the oracle to it at 1e-12 wherever the exact statistics exist (positive finite series).

The bar is test_gpu_gof.py's: the device's NaN / inf pattern equals the oracle's and finite entries agree to
1e-9 * max(1, |ref|); waterbody tables are bit-identical."""

import functools
import warnings

import mpmath
import numpy as np
import pytest

from simplyp_amd import abi, marshal
from oracle import gof as ogof
from oracle import waterbody as owb

pytestmark = pytest.mark.gpu

FLUX = ['Qr', 'Msus_kg/day', 'TDP_kg/day', 'PP_kg/day']
MASK = marshal.mask_of_columns(FLUX)
assert marshal.columns_of_mask(MASK) == FLUX
V = {v: i for i, v in enumerate(abi.GOF_VARS)}
ST = {s: i for i, s in enumerate(abi.GOF_STATS)}
A_UNIT = 86.4                      # A_catch at which Q = Qr A 1000/86400 is Qr itself on the device (the folded factor is exactly 1)
assert A_UNIT * 1000 / 86400 == 1.0


# ---- tables, device calls, references ----

def make_table(rng, D, R, E):
    """[4, D, R, E] = Qr (mm/d) and the three fluxes (kg/day), ordinary positive values."""
    return np.stack([rng.uniform(0.2, 3.0, (D, R, E)), rng.uniform(5.0, 500.0, (D, R, E)),
                     rng.uniform(0.02, 0.5, (D, R, E)), rng.uniform(0.05, 1.0, (D, R, E))])


def reach_params(A):
    rp = np.ones((len(marshal.PR_NAMES),) + A.shape)
    rp[marshal.PR_NAMES.index('A_catch')] = A
    return rp


def obs_like(rng, tab, A, f, days_by_var, member=0, r=0):
    """[6, D] observations: the simulated series of one member times a factor in [0.7, 1.4] on the given days."""
    D = tab.shape[1]
    sim = ogof.simulated_series(*[tab[c, :, r, member] for c in range(4)], A[r, member], f[member])
    obs = np.full((6, D), np.nan)
    for v, days in days_by_var.items():
        days = np.asarray(days, dtype=np.int64)
        obs[V[v], days] = sim[v][days] * rng.uniform(0.7, 1.4, len(days))
    return obs


def device_gof(engine0, tab, obs, f, A, out_reaches=None, member_of_slot=None, spearman=True):
    """tab [4, D, R, E] numpy; A [S, E].  Returns (gof [8, 6, R, E], rho [6, R, E] or None, info)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(tab)).to(engine0.tdev)
    mos = None if member_of_slot is None else torch.from_numpy(np.asarray(member_of_slot, dtype=np.int32)).to(engine0.tdev)
    g, info = engine0.gof(t, MASK, obs, f, reach_params(A), out_reaches=out_reaches, member_of_slot=mos, spearman=spearman)
    return g.cpu().numpy(), (info['spearman'].cpu().numpy() if spearman else None), info


def oracle_gof(tab, obs, f, A):
    """[8, 6, R, E]; A [R, E] are the rows of the table's reaches."""
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                      # means of empty slices, 0/0: the semantics under test
        return np.stack([ogof.ensemble_stats(tab[:, :, r, :], A[r], f, obs[r]) for r in range(tab.shape[2])], axis=2)


def oracle_spearman(tab, obs, f, A, r, e, v):
    """What simplyp_gof_spearman returns for one (reach, member, variable): NaN for a dropped variable and for a member with a
    NaN on an observation day, otherwise pandas' value (spearman_of_pair)."""
    o = obs[r, V[v]]
    if int((~np.isnan(o)).sum()) <= ogof.MIN_OBS:
        return np.nan
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        sim = ogof.simulated_series(*[tab[c, :, r, e] for c in range(4)], A[r, e], f[e])[v]
        if np.isnan(sim[~np.isnan(o)]).any():
            return np.nan
        return ogof.spearman_of_pair(o, sim)


def same_pattern(got, ref):
    return bool((np.isnan(got) == np.isnan(ref)).all() and (np.isposinf(got) == np.isposinf(ref)).all()
                and (np.isneginf(got) == np.isneginf(ref)).all())


def assert_close(got, ref, tol=1e-9, what=None):
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    assert same_pattern(got, ref), (what, np.argwhere((np.isnan(got) != np.isnan(ref)) | (np.isinf(got) != np.isinf(ref))
                                                      | (np.isinf(ref) & (got != ref)))[:8].tolist())
    fin = np.isfinite(ref)
    with np.errstate(invalid='ignore'):
        err = np.where(fin, np.abs(got - ref) / np.maximum(1.0, np.abs(ref)), 0.0)
    assert err.max() <= tol, (what, float(err.max()), np.argwhere(err == err.max())[0].tolist())
    return float(err.max())


def exact_stats(obs, qr, ms, td, pp, A, f, v, r2_only=False):
    """The eight statistics of one (member, variable) in 40-digit arithmetic from the fp64 table, None where not defined here
    (a non-positive or non-finite simulated value; log rows with an observation of 0).  A NaN simulated value drops its day; a
    negative observation has no log and is skipped by both log sums, as pandas skips it.  Also returns
    kappa = sum (s - c)^2 / sum (s - mean s)^2 with c the mean of all observations: the cancellation a one-pass sum shifted by
    c suffers in the variance of the simulated series.  r2_only: N obs, r2 and kappa alone (a third of the work)."""
    with mpmath.workdps(40):
        mp = mpmath.mpf
        days = np.flatnonzero(~np.isnan(obs))
        n_obs = len(days)
        if n_obs <= ogof.MIN_OBS:
            return None, None
        c_all = mpmath.fsum(mp(float(obs[d])) for d in days) / n_obs
        Am, fm = mp(float(A)), mp(float(f))
        q_factor = Am * 1000 / 86400
        need = {'Q': [0], 'SS': [0, 1], 'TDP': [0, 2], 'PP': [0, 3], 'TP': [0, 2, 3], 'SRP': [0, 2]}[v]
        o, s = [], []
        for d in days:
            cols = [float(x[d]) for x in (qr, ms, td, pp)]
            if any(cols[c] != cols[c] for c in need):
                continue
            if not all(np.isfinite(cols[c]) for c in need) or cols[0] <= 0.0:
                return None, None
            q = mp(cols[0])
            val = q * q_factor if v == 'Q' else (mp(cols[2]) + mp(cols[3])) / q / Am if v == 'TP' \
                else fm * mp(cols[2]) / q / Am if v == 'SRP' else mp(cols[need[1]]) / q / Am
            if val <= 0:
                return None, None
            o.append(mp(float(obs[d]))); s.append(val)
        n = len(o)
        if n == 0:
            return None, None
        row = [mp(n_obs)] + [None] * 7
        mo, msim = mpmath.fsum(o) / n, mpmath.fsum(s) / n
        var_o = mpmath.fsum((a - mo) ** 2 for a in o)
        var_s = mpmath.fsum((b - msim) ** 2 for b in s)
        kappa = float(mpmath.fsum((b - c_all) ** 2 for b in s) / var_s) if var_s > 0 else None
        if var_o > 0 and var_s > 0:
            row[3] = mpmath.fsum((a - mo) * (b - msim) for a, b in zip(o, s)) ** 2 / (var_o * var_s)
        if r2_only:
            return row, kappa
        if var_o > 0:
            row[1] = 1 - mpmath.fsum((a - b) ** 2 for a, b in zip(o, s)) / var_o
            row[5] = 100 * (mpmath.fsum(abs(b - a) for a, b in zip(o, s)) / n) / mpmath.sqrt(var_o / n)
        if all(a != 0 for a in o):
            lp = [(mpmath.log(a), mpmath.log(b)) for a, b in zip(o, s) if a > 0]
            mlo = mpmath.fsum(a for a, _ in lp) / len(lp)
            var_lo = mpmath.fsum((a - mlo) ** 2 for a, _ in lp)
            if var_lo > 0:
                row[2] = 1 - mpmath.fsum((a - b) ** 2 for a, b in lp) / var_lo
        row[4] = 100 * mpmath.fsum(b - a for a, b in zip(o, s)) / mpmath.fsum(o)
        row[6] = mpmath.fsum(mpmath.log(b) for b in s)
        row[7] = mpmath.fsum((a / b - 1) ** 2 for a, b in zip(o, s))
        return row, kappa


def hold_oracle_to_exact(ref, tab, obs, f, A, members, variables=abi.GOF_VARS, bar=1e-12, r2_only=False):
    """ref [8, 6, R, E] (oracle): within `bar` of the exact statistics for the given members, wherever those exist.  Returns
    {(r, e, v): (exact row, kappa)}."""
    out, checked = {}, 0
    for r in range(tab.shape[2]):
        for e in members:
            for v in variables:
                row, kappa = exact_stats(obs[r, V[v]], *[tab[c, :, r, e] for c in range(4)], A[r, e], f[e], v, r2_only)
                if row is None:
                    continue
                out[(r, e, v)] = (row, kappa)
                for j, x in enumerate(row):
                    if x is None or not np.isfinite(ref[j, V[v], r, e]):
                        continue
                    with mpmath.workdps(40):
                        err = float(abs(mpmath.mpf(float(ref[j, V[v], r, e])) - x) / max(1, abs(x)))
                    assert err <= bar, ('oracle vs exact', r, e, v, abi.GOF_STATS[j], err)
                    checked += 1
    assert checked > 0
    return out


# ---- 1. member versus slot ----

def test_a_catch_and_f_tdp_follow_the_member_not_the_slot(engine0):
    """65 members, each with its own A_catch per reach and its own f_TDP, the table's member axis a random permutation; the
    table holds reaches [2, 0] of three.  Statistics and Spearman's r come back per MEMBER and equal the identity-order call."""
    rng = np.random.default_rng(101)
    E, D, S, reaches = 65, 300, 3, [2, 0]
    tab = make_table(rng, D, 2, E)
    A_full = rng.uniform(20.0, 120.0, (S, E))
    A = A_full[reaches]
    f = rng.uniform(0.4, 0.95, E)
    q_days = np.sort(rng.choice(D, 130, replace=False))
    c_days = np.sort(rng.choice(D, 41, replace=False))
    obs = np.stack([obs_like(rng, tab, A, f, dict(Q=q_days, SS=c_days, TDP=c_days[::2], PP=c_days, TP=c_days[1:], SRP=c_days[:30]), r=r)
                    for r in range(2)])
    ref = oracle_gof(tab, obs, f, A)
    hold_oracle_to_exact(ref, tab, obs, f, A, members=range(0, E, 9))
    mos = rng.permutation(E).astype(np.int32)
    g0, rho0, _ = device_gof(engine0, tab, obs, f, A_full, out_reaches=reaches)
    g1, rho1, _ = device_gof(engine0, tab[..., mos], obs, f, A_full, out_reaches=reaches, member_of_slot=mos)
    assert_close(g0, ref, what='identity order')
    assert_close(g1, ref, what='permuted slots')
    assert np.array_equal(g0, g1, equal_nan=True) and np.array_equal(rho0, rho1, equal_nan=True)
    for r in range(2):
        for e in (0, 1, 31, 63, 64):
            for v in abi.GOF_VARS:
                want = oracle_spearman(tab, obs, f, A, r, e, v)
                assert abs(rho1[V[v], r, e] - want) < 1e-9, (r, e, v, rho1[V[v], r, e], want)
    # the lookups matter on this table: the statistics of a member change when it is given its neighbour's A_catch / f_TDP
    assert not np.allclose(oracle_gof(tab, obs, np.roll(f, 1), A)[1, V['SRP']], ref[1, V['SRP']], rtol=1e-6)
    assert not np.allclose(oracle_gof(tab, obs, f, np.roll(A, 1, axis=1))[1, V['Q']], ref[1, V['Q']], rtol=1e-6)


# ---- 2. list lengths ----

@functools.lru_cache(maxsize=None)
def _lengths_table():
    rng = np.random.default_rng(202)
    E, D = 70, 2100
    return make_table(rng, D, 2, E), np.stack([rng.uniform(20.0, 120.0, E), rng.uniform(20.0, 120.0, E)]), rng.uniform(0.4, 0.95, E)


@pytest.mark.parametrize('n_q, n_c', [(10, 11), (11, 12), (12, 13), (31, 15), (32, 11), (33, 12), (63, 13), (64, 15), (65, 11), (2049, 13)])
def test_day_lists_at_the_edges_of_the_batches(engine0, n_q, n_c):
    """n_q discharge observations (10: the variable is dropped) and n_c chemistry days on reach 0, the first on day 0 and the last
    on day D - 1; reach 1 has no observation at all.  PP lacks one of the chemistry days when that leaves it more than 10."""
    tab, A, f = _lengths_table()
    D, E = tab.shape[1], tab.shape[3]
    rng = np.random.default_rng(1000 * n_q + n_c)
    ends = np.array([0, D - 1])
    q_days = np.sort(np.concatenate([ends, rng.choice(np.arange(1, D - 1), n_q - 2, replace=False)]))
    c_days = np.sort(np.concatenate([ends, rng.choice(np.arange(1, D - 1), n_c - 2, replace=False)]))
    pp_days = np.delete(c_days, 3) if n_c > 11 else c_days
    obs = np.full((2, 6, D), np.nan)
    obs[0] = obs_like(rng, tab, A, f, dict(Q=q_days, SS=c_days, TDP=c_days, PP=pp_days, TP=c_days, SRP=c_days[:8]))
    ref = oracle_gof(tab, obs, f, A)
    hold_oracle_to_exact(ref, tab, obs, f, A, members=(0, 69))
    g, rho, info = device_gof(engine0, tab, obs, f, A)
    assert info['n_q_days'] == (n_q if n_q > 10 else 0) and info['n_chem_days'] == n_c
    # slices of a day list: at most 64, and at least 32 days per slice and reach
    for key, n in (('n_chunks_q', info['n_q_days']), ('n_chunks_chem', n_c)):
        assert 1 <= info[key] <= max(1, min(64, n // 2 // 32)), (key, info[key], n)
    if n_q == 2049:
        assert info['n_chunks_q'] > 1
    assert_close(g, ref, what=(n_q, n_c))
    assert (g[0, :, 1] == 0).all() and np.isnan(g[1:, :, 1]).all()                       # the reach without observations
    assert (g[0, V['Q'], 0] == n_q).all() and np.isnan(g[1:, V['Q'], 0]).all() == (n_q <= 10)
    assert (g[0, V['SRP'], 0] == 8).all() and np.isnan(g[1:, V['SRP'], 0]).all()
    for e in (0, 64, 69):
        for v in abi.GOF_VARS:
            want = oracle_spearman(tab, obs, f, A, 0, e, v)
            assert (np.isnan(want) and np.isnan(rho[V[v], 0, e])) or abs(rho[V[v], 0, e] - want) < 1e-9, (e, v, rho[V[v], 0, e], want)
    assert np.isnan(rho[:, 1]).all()


# ---- 3. the 1e-290 / 1e290 switch ----

def _neighbours3(x):
    return [np.nextafter(x, 0.0), x, np.nextafter(x, np.inf)]


def test_values_on_either_side_of_the_switch_to_libm(engine0):
    """One member per magnitude, the value on ONE observation day: members 0-7 carry it as their simulated discharge (A_catch =
    86.4: Q is Qr itself), members 8-15 as their Qr on a chemistry day (concentrations of the order of 1 / value), member 16 is
    ordinary.  At 1e+-290 and their neighbours squares overflow: N obs, sum_log_sim and the NaN / inf pattern are the oracle's;
    at 1e+-150 every row is."""
    rng = np.random.default_rng(303)
    mags = _neighbours3(1e-290) + _neighbours3(1e290) + [1e-150, 1e150]
    E, D = 17, 80
    tab = make_table(rng, D, 1, E)
    A = np.full((1, E), A_UNIT)
    f = rng.uniform(0.4, 0.95, E)
    q_days = np.arange(0, 60, 2)                             # even days
    c_days = np.arange(1, 41, 2)                             # odd days
    obs = obs_like(rng, tab, A, f, dict(Q=q_days, SS=c_days, TDP=c_days, PP=c_days, TP=c_days, SRP=c_days), member=16)[None]
    for i, m in enumerate(mags):
        tab[0, 10, 0, i] = m                                 # a discharge day
        tab[0, 11, 0, 8 + i] = m                             # a chemistry day
    ref = oracle_gof(tab, obs, f, A)
    hold_oracle_to_exact(ref, tab, obs, f, A, members=(6, 7, 14, 15, 16))
    g, _, _ = device_gof(engine0, tab, obs, f, A, spearman=False)
    assert same_pattern(g, ref)
    assert_close(g[[ST['N obs'], ST['sum_log_sim']]], ref[[ST['N obs'], ST['sum_log_sim']]], what='N obs, sum_log_sim')
    assert_close(g[..., [6, 7, 14, 15, 16]], ref[..., [6, 7, 14, 15, 16]], what='1e+-150 and ordinary')
    # the untouched variables of every member are ordinary
    assert_close(g[:, 1:, :, :8], ref[:, 1:, :, :8], what='chemistry of the discharge members')
    assert_close(g[:, :1, :, 8:], ref[:, :1, :, 8:], what='discharge of the chemistry members')


# ---- 4. special simulated values ----

def test_special_simulated_values_on_single_days(engine0):
    """Members 0-4: on one discharge day Q is 0, -0.0, negative, +inf, NaN.  Members 5-9: on one chemistry day Qr is 0 (a
    positive flux over 0: +inf concentrations), -0.0 (-inf), the SS flux is 0, negative, NaN.  Member 10: NaN on all observation
    days but one; member 11: NaN throughout; member 12: ordinary.  Spearman's r is NaN for a member with a NaN on an observation
    day."""
    rng = np.random.default_rng(404)
    E, D = 13, 80
    tab = make_table(rng, D, 1, E)
    A = np.full((1, E), A_UNIT)
    f = rng.uniform(0.4, 0.95, E)
    q_days, c_days = np.arange(0, 60, 2), np.arange(1, 41, 2)
    obs = obs_like(rng, tab, A, f, dict(Q=q_days, SS=c_days, TDP=c_days, PP=c_days, TP=c_days, SRP=c_days), member=12)[None]
    for e, x in enumerate([0.0, -0.0, -1.5, np.inf, np.nan]):
        tab[0, 10, 0, e] = x
    tab[0, 11, 0, 5], tab[0, 11, 0, 6] = 0.0, -0.0
    for e, x in zip((7, 8, 9), (0.0, -20.0, np.nan)):
        tab[1, 11, 0, e] = x
    keep = np.zeros(D, dtype=bool); keep[[10, 11]] = True
    tab[:, ~keep, 0, 10] = np.nan
    tab[:, :, 0, 11] = np.nan
    ref = oracle_gof(tab, obs, f, A)
    hold_oracle_to_exact(ref, tab, obs, f, A, members=(4, 9, 12))
    g, rho, _ = device_gof(engine0, tab, obs, f, A)
    for e in range(E):
        assert_close(g[..., e], ref[..., e], what='member %d' % e)
    assert np.isneginf(ref[ST['sum_log_sim'], V['Q'], 0, 0]) and np.isnan(ref[ST['sum_log_sim'], V['Q'], 0, 2])      # the cases are the intended ones
    assert np.isposinf(ref[ST['Bias (%)'], V['SS'], 0, 5]) and np.isnan(ref[ST['r2'], V['Q'], 0, 3])
    assert np.isnan(ref[1:6, :, 0, 11]).all() and (ref[6:, :, 0, 11] == 0).all()
    for e in range(E):
        for v in abi.GOF_VARS:
            want = oracle_spearman(tab, obs, f, A, 0, e, v)
            got = rho[V[v], 0, e]
            assert (np.isnan(want) and np.isnan(got)) or abs(got - want) < 1e-9, (e, v, got, want)
    assert np.isnan(rho[V['Q'], 0, [4, 10, 11]]).all() and np.isnan(rho[V['SS'], 0, 9]) and np.isfinite(rho[V['TDP'], 0, 9])


# ---- 5. special observations ----

def test_an_observation_of_zero_and_a_negative_observation(engine0):
    """TDP has an observation of exactly 0 (its log is -inf: log NSE is NaN in the reference too); Q and SS have one NEGATIVE
    observation each: np.log of it is NaN, which pandas skips in both sums of log NSE (visualise_results.py:442-443), so log NSE
    is finite and its mean log runs over the days that have a log.  Members 66-69 also lack simulated values on some days."""
    rng = np.random.default_rng(505)
    E, D = 70, 120
    tab = make_table(rng, D, 1, E)
    A = rng.uniform(20.0, 120.0, (1, E))
    f = rng.uniform(0.4, 0.95, E)
    q_days = np.sort(rng.choice(D, 50, replace=False))
    c_days = np.sort(rng.choice(D, 23, replace=False))
    obs = obs_like(rng, tab, A, f, dict(Q=q_days, SS=c_days, TDP=c_days, PP=c_days, TP=c_days, SRP=c_days))[None]
    obs[0, V['TDP'], c_days[4]] = 0.0
    obs[0, V['Q'], q_days[17]] = -0.3
    obs[0, V['SS'], c_days[9]] = -2.0
    tab[:, q_days[3], 0, 66] = np.nan
    tab[:, q_days[17], 0, 67] = np.nan                       # the pair of the negative observation itself is dropped
    tab[:, c_days[9], 0, 68] = np.nan
    tab[:, c_days[2], 0, 69] = np.nan
    ref = oracle_gof(tab, obs, f, A)
    assert np.isfinite(ref[ST['log NSE'], V['Q']]).all() and np.isfinite(ref[ST['log NSE'], V['SS']]).all()
    assert np.isnan(ref[ST['log NSE'], V['TDP']]).all()
    hold_oracle_to_exact(ref, tab, obs, f, A, members=(0, 1, 66, 67, 68, 69))
    g, rho, _ = device_gof(engine0, tab, obs, f, A)
    assert_close(g, ref)
    for e in (0, 65, 67):
        for v in ('Q', 'SS', 'TDP'):
            want = oracle_spearman(tab, obs, f, A, 0, e, v)
            got = rho[V[v], 0, e]
            assert (np.isnan(want) and np.isnan(got)) or abs(got - want) < 1e-9, (e, v, got, want)


# ---- 6. conditioning of r2 ----

def test_r2_degrades_no_faster_than_the_shifted_sums_allow(engine0):
    """n = 4303 discharge days (the Tarland record's count), the simulated series at k times the observed mean with a
    coefficient of variation cv, s = k mu (1 + cv (x - 1)): kappa = sum (s - c)^2 / sum (s - mean s)^2 ~ ((k - 1) / (k cv))^2 + 1
    runs from 1 to 1e6.  The
    device's variance of s is a difference of two one-pass sums shifted by c, each a sum of n terms rounded to 2^-53 relative:
    its relative error, and that of r2, is at most about n 2^-52 kappa.  Every other statistic stays at 1e-9."""
    rng = np.random.default_rng(606)
    ks, cvs = [1.0, 10.0, 100.0, 1000.0], [1.0, 0.1, 0.01, 0.001]
    n = 4303
    E, D = len(ks) * len(cvs), n
    x, w = rng.exponential(1.0, n), rng.uniform(-1.0, 1.0, n)               # x: mean 1, coefficient of variation 1, positive
    mu = 1.7
    obs = np.full((1, 6, D), np.nan)
    obs[0, 0] = mu * (1.0 + 0.3 * (x - 1.0) + 0.2 * w)
    tab = make_table(rng, D, 1, E)
    kc = [(k, cv) for k in ks for cv in cvs]
    for e, (k, cv) in enumerate(kc):
        tab[0, :, 0, e] = k * mu * (1.0 + cv * (x - 1.0))
    assert (tab[0] > 0.0).all() and (obs[0, 0] > 0.0).all()
    A = np.full((1, E), A_UNIT)
    f = np.full(E, 0.7)
    ref = oracle_gof(tab, obs, f, A)
    corners = [0, 3, 12, 15]                                 # every row for the four corners of the ladder, r2 and kappa for the rest
    exact = hold_oracle_to_exact(ref, tab, obs, f, A, members=corners, variables=['Q'])
    exact.update(hold_oracle_to_exact(ref, tab, obs, f, A, members=sorted(set(range(E)) - set(corners)), variables=['Q'], r2_only=True))
    g, _, info = device_gof(engine0, tab, obs, f, A, spearman=False)
    assert info['n_q_days'] == n
    keep = [j for j in range(len(abi.GOF_STATS)) if j != ST['r2']]
    assert_close(g[keep], ref[keep], what='all rows but r2')
    worst_ok = 0.0
    for e, (k, cv) in enumerate(kc):
        row, kappa = exact[(0, e, 'Q')]
        err = abs(g[ST['r2'], 0, 0, e] - float(row[ST['r2']]))
        print('k = %6g  cv = %5g  kappa = %.3e  |r2 - exact| = %.3e' % (k, cv, kappa, err))
        assert err <= max(1e-9, n * 2.0 ** -52 * kappa), (k, cv, kappa, err)
        if err <= 1e-9:
            worst_ok = max(worst_ok, kappa)
    print('largest kappa at which r2 meets 1e-9: %.3e' % worst_ok)
    assert max(kp for _, kp in exact.values()) > 5e5 and min(kp for _, kp in exact.values()) < 2.0


# ---- 7. Spearman ----

@pytest.mark.parametrize('n', [11, 31, 32, 33, 64, 65, 97])
def test_spearman_at_the_edges_of_its_tile(engine0, n):
    """n paired days around the tile of 32 values per lane.  Per member (pattern = member % 7): 0 ordinary; 1 heavy ties (three
    distinct values); 2 zeros of both signs, which tie; 3 +inf and -inf among the values; 4 constant (NaN, as pandas gives it);
    5 ties that mirror the tied observations; 6 strictly monotone in time, no ties.  The observations
    are rounded to one decimal: ties on their side too."""
    rng = np.random.default_rng(700 + n)
    E, D = 70, 130
    tab = make_table(rng, D, 1, E)
    A = np.full((1, E), A_UNIT)
    f = np.full(E, 0.7)
    days = np.sort(rng.choice(D, n, replace=False))
    obs = np.full((1, 6, D), np.nan)
    obs[0, 0, days] = np.round(rng.uniform(0.2, 3.0, n), 1)
    for e in range(E):
        p = e % 7
        q = tab[0, :, 0, e]
        if p == 1:
            q[:] = rng.choice([0.5, 1.0, 1.5], D)
        elif p == 2:
            q[:] = rng.choice([-0.0, 0.0, 1.0], D)
        elif p == 3:
            q[days[2]], q[days[7]] = np.inf, -np.inf
        elif p == 4:
            q[:] = 1.25
        elif p == 5:
            q[days] = obs[0, 0, days] * 2.0
        elif p == 6:
            q[:] = np.linspace(5.0, 1.0, D)
    g, rho, _ = device_gof(engine0, tab, obs, f, A)
    assert np.isnan(rho[1:]).all()
    seen = 0
    for e in range(E):
        want = oracle_spearman(tab, obs, f, A, 0, e, 'Q')
        got = rho[0, 0, e]
        if e % 7 == 4:
            assert np.isnan(want) and np.isnan(got), (e, got, want)
        else:
            assert abs(got - want) < 1e-9, (e, e % 7, got, want)
            seen += 1
    assert seen == 60


# ---- 8. waterbody ----

@pytest.mark.parametrize('E', [65, 66])                      # one / two member slots per lane
@pytest.mark.parametrize('n_sum', [1, 16])
def test_waterbody_sums_with_missing_cells_and_their_statistics(engine0, E, n_sum):
    """A NaN in one reach's cell of each of the four columns counts as 0 in that column's sum; on a day on which every summed
    reach is NaN the discharge is 0 and the concentrations 0/0.  The table is the oracle's bit for bit; the statistics of the
    summed series (simplyp_gof_waterbody) meet the bar of the reach statistics."""
    import torch
    rng = np.random.default_rng(800 + E + n_sum)
    D, R = 40, 16
    tab = make_table(rng, D, R, E)
    A = rng.uniform(20.0, 120.0, (R, E))
    f = rng.uniform(0.4, 0.95, E)
    reaches = list(range(R)) if n_sum == 16 else [5]
    for c in range(4):
        tab[c, 3 + c, reaches[c % n_sum], [1, E - 1]] = np.nan              # one cell of one column
    tab[:, 19, :, [2, E - 2]] = np.nan                                       # a day without any value
    t = torch.from_numpy(tab).to(engine0.tdev)
    wb, info = engine0.waterbody(t, MASK, reaches, f, reach_params(A))
    with np.errstate(all='ignore'):
        want = owb.sum_to_waterbody(*[tab[c][:, reaches, :] for c in range(4)], A[reaches], f)
    got = wb.cpu().numpy()
    assert info['columns'] == owb.COLUMNS and np.array_equal(got, want, equal_nan=True)
    assert (got[0, 19, [2, E - 2]] == 0).all() and np.isnan(got[4:8, 19, [2, E - 2]]).all() and np.isfinite(got[..., 0]).all()
    names = ['Q_cumecs', 'SS_mgl', 'TDP_mgl', 'PP_mgl', 'TP_mgl', 'SRP_mgl']
    obs = np.full((6, D), np.nan)
    for vi, name in enumerate(names):
        days = np.arange(4, 36) if vi == 0 else np.arange(1, 40, 3) if vi < 5 else np.arange(0, 40, 5)      # 32, 13, 8 observations
        obs[vi, days] = want[owb.COLUMNS.index(name), days, 0] * rng.uniform(0.7, 1.4, len(days))
    gof, ginfo = engine0.gof_waterbody(wb, info['columns'], obs, f)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        ref = np.stack([[ogof.stats_of_pair(obs[vi], want[owb.COLUMNS.index(name), :, e]) for e in range(E)]
                        for vi, name in enumerate(names)]).transpose(2, 0, 1)
    assert_close(gof.cpu().numpy()[:, :, 0, :], ref)
    assert ginfo['n_q_days'] == 32 and ginfo['n_chem_days'] == 13
    assert np.isneginf(ref[ST['sum_log_sim'], 0, 2]) and np.isfinite(ref[1:, 1:5, 2]).all()      # Q = 0 on an observed day; its concentrations are dropped
