"""Sobol' indices on the device (simplyp_sobol_design, simplyp_sobol_indices, sp.sobol_indices) against their NumPy statement
(simplyp_amd/sobol.py): the design bit for bit, the contraction on exact integer data bit for bit and on real data within the
summation bound, the ratios bit for bit from the device's own sums, validity, edge cases, argument errors, the percentile
interval, and the public call end to end."""

import ctypes as C

import numpy as np
import pandas as pd
import pytest
import torch

import helpers
import simplyp_amd as sp
from simplyp_amd import abi, engine, marshal, sobol

pytestmark = pytest.mark.gpu

NAME = 'tarland_2004_dynamic'
SENTINEL = -777.25
SHAPES = [(2, 1), (5, 3), (64, 16), (67, 7), (260, 2)]          # 4, 8, 34, 16 and 6 term columns; K and tiles with tails
N_ROWS = [1, 3, 17]
N_BOOT = [0, 1, 16, 19, 70]
U53 = 2.0 ** -53


def dev(eng, a, dtype=torch.float64):
    return eng.to_device(np.ascontiguousarray(a), dtype)


def box(d):
    return -np.pi * (1.0 + 0.1 * np.arange(d)), np.pi * (1.0 + 0.05 * np.arange(d))


def exact_table(n_rows, N, d):
    """Small integers with an asymmetric pattern, (3 r + 5 j + 7 n) mod 11 - 5, and mu exactly 0: the B block mirrors n and
    negates the A block."""
    r = np.arange(n_rows)[:, None, None]
    j = np.arange(d + 2)[None, :, None]
    n = np.arange(N)[None, None, :]
    f = ((3 * r + 5 * j + 7 * n) % 11 - 5).astype(np.float64)
    f[:, 1] = -f[:, 0, ::-1]
    return np.ascontiguousarray(f.reshape(n_rows, (d + 2) * N))


def real_table(n_rows, N, d, seed=0):
    """Row 0: Ishigami + 100 of the design's points; the others lognormal in one coordinate and noise."""
    lo, hi = box(d)
    x = sobol.design(N, lo, hi, seed=seed)
    rng = np.random.default_rng(seed)
    t = np.empty((n_rows, x.shape[1]))
    t[0] = np.sin(x[0]) + 7.0 * np.sin(x[1 % d]) ** 2 + 0.1 * x[2 % d] ** 4 * np.sin(x[0]) + 100.0
    for r in range(1, n_rows):
        t[r] = np.exp(0.5 * x[r % d] + 0.3 * rng.normal(size=x.shape[1])) * 10.0 ** (r % 5 - 2)
    return t


def sums_bound(table, N, d, counts, valid=None):
    """N 2^-53 sum_n |c_n term_n|, element by element: [B, n_rows, 2 d + 2]."""
    valid = np.ones(N, dtype=bool) if valid is None else valid
    terms, _ = sobol.row_terms(table, N, d, valid)
    return N * U53 * np.einsum('bn,rnt->brt', counts[:, valid].astype(np.float64), np.abs(terms))


def run(eng, table, N, d, n_boot, seed=0, status=None):
    ind, sums, n_used, info = eng.sobol_indices(dev(eng, table), N, d, status=None if status is None else dev(eng, status, torch.int32),
                                                n_boot=n_boot, seed=seed)
    return ind.cpu().numpy(), sums.cpu().numpy(), n_used.cpu().numpy(), info


# ---- the design ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('N,d', SHAPES)
@pytest.mark.parametrize('own_unit', [False, True])
def test_design_is_the_mirror_bit_for_bit(engine0, N, d, own_unit):
    E = N * (d + 2)
    lo, hi = box(d)
    rows = np.random.default_rng(d).permutation(marshal.NP_M)[:d].astype(np.int32)
    target = rows.copy()
    if d >= 2:
        target[1] = abi.MCMC_TARGET_F_TDP
    if d >= 3:
        target[2] = abi.MCMC_TARGET_NONE
    unit = np.random.default_rng(N).random((2, d, N)) if own_unit else None
    f64 = dict(dtype=torch.float64, device=engine0.tdev)
    mp, ft = torch.full((marshal.NP_M, E), SENTINEL, **f64), torch.full((E,), SENTINEL, **f64)
    x_d, info = engine0.sobol_design(N, lo, hi, target, mp, ft, seed=12345678901234567, unit=unit)
    want = sobol.design(N, lo, hi, seed=12345678901234567, unit=unit)
    assert np.array_equal(x_d.cpu().numpy(), want) and info['kernel_ms'] > 0.0
    mp_h, ft_h = mp.cpu().numpy(), ft.cpu().numpy()
    named = [int(t) for t in target if t >= 0]
    for k, t in enumerate(target):
        if t >= 0:
            assert np.array_equal(mp_h[t], want[k])
    assert (np.delete(mp_h, named, axis=0) == SENTINEL).all()             # rows nobody names still hold the sentinel
    assert np.array_equal(ft_h, want[1]) if d >= 2 else (ft_h == SENTINEL).all()


# ---- the contraction -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('N,d', SHAPES)
def test_exact_integer_data_bit_for_bit(engine0, N, d):
    """The operand maps of the fp64 MFMA on data every sum of which is exactly representable: any wrong lane, row or column
    changes an integer."""
    for n_rows in N_ROWS:
        table = exact_table(n_rows, N, d)
        for n_boot in N_BOOT:
            want = sobol.sobol_indices(table, N, d, n_boot=n_boot, seed=n_boot + 3)
            ind, sums, n_used, info = run(engine0, table, N, d, n_boot, seed=n_boot + 3)
            assert np.array_equal(sums, want['sums']), (n_rows, n_boot, np.argwhere(sums != want['sums'])[:4])
            assert np.array_equal(n_used, want['n_used']) and info['n_valid'] == N and info['n_resamples'] == 1 + n_boot
            assert np.array_equal(ind, want['indices'], equal_nan=True)
            assert info['flops'] == 2 * (1 + n_boot) * n_rows * N * (2 * d + 2)
    assert np.abs(want['sums']).max() > 0 and len(np.unique(want['sums'])) > 8


def test_largest_base_sample(engine0):
    """N = 32768: the counts kernel's histogram fills the 64 KB of LDS a block may have, and a bin can reach 2^15."""
    N, d = sobol.MAX_BASE, 1
    table = exact_table(2, N, d)
    want = sobol.sobol_indices(table, N, d, n_boot=2, seed=1)
    ind, sums, n_used, info = run(engine0, table, N, d, 2, seed=1)
    assert np.array_equal(sums, want['sums']) and np.array_equal(n_used, want['n_used']) and info['n_valid'] == N
    assert np.array_equal(ind, want['indices'], equal_nan=True)


@pytest.mark.parametrize('N,d', SHAPES)
def test_real_data_within_the_summation_bound(engine0, N, d):
    for n_rows in N_ROWS:
        table = real_table(n_rows, N, d, seed=n_rows)
        for n_boot in N_BOOT:
            want = sobol.sobol_indices(table, N, d, n_boot=n_boot, seed=7)
            ind, sums, n_used, _ = run(engine0, table, N, d, n_boot, seed=7)
            bound = sums_bound(table, N, d, want['counts'])
            err = np.abs(sums - want['sums'])
            assert (err <= bound).all(), (n_rows, n_boot, float((err / np.maximum(bound, 1e-300)).max()))
            assert np.array_equal(n_used, want['n_used'])
            # the ratios: the stated formula applied to the device's own sums, bit for bit
            own, _ = sobol.indices_from_sums(sums, n_used, d)
            assert np.array_equal(ind, own, equal_nan=True)
            again = run(engine0, table, N, d, n_boot, seed=7)
            assert np.array_equal(again[0], ind, equal_nan=True) and np.array_equal(again[1], sums)
            point = run(engine0, table, N, d, 0)
            assert np.array_equal(point[0][..., 0], ind[..., 0], equal_nan=True)        # resample 0 is the point estimate
    if N >= 64:
        assert np.isfinite(ind).all() and 0.0 < ind[1, 0, 0, 0] < 1.5


def test_leading_axes_are_rows(engine0):
    N, d = 67, 7
    table = real_table(6, N, d).reshape(2, 3, -1)
    ind, sums, n_used, _ = engine0.sobol_indices(dev(engine0, table), N, d, n_boot=5, seed=1)
    flat = run(engine0, table.reshape(6, -1), N, d, 5, seed=1)
    assert tuple(ind.shape) == (2, d, 2, 3, 6) and tuple(sums.shape) == (6, 2, 3, 2 * d + 2)
    assert np.array_equal(ind.cpu().numpy().reshape(flat[0].shape), flat[0]) and np.array_equal(sums.cpu().numpy().reshape(flat[1].shape), flat[1])


# ---- validity --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('N,d', [(5, 3), (67, 7), (260, 2)])
def test_invalid_samples_take_part_in_nothing(engine0, N, d):
    n_rows, n_boot = 3, 19
    clean = real_table(n_rows, N, d, seed=4)
    status = np.zeros(N * (d + 2), dtype=np.int32)
    hit = [(0, 1), (1, N - 1), (d + 1, N // 2)]                            # an A member, a B member, the last AB block's
    table = clean.copy()
    for j, n in hit:
        status[j * N + n] = abi.STATUS_NONFINITE
        table[:, j * N + n] = np.nan
    status[2 * N] = abi.STATUS_STEPCAP                                     # not a reason
    valid = sobol.valid_samples(status, N, d)
    assert valid.sum() == N - 3
    want = sobol.sobol_indices(table, N, d, status=status, n_boot=n_boot, seed=2)
    ind, sums, n_used, info = run(engine0, table, N, d, n_boot, seed=2, status=status)
    assert np.isfinite(sums).all() and info['n_valid'] == N - 3 and n_used[0] == N - 3
    assert np.array_equal(n_used, (want['counts'] * valid).sum(axis=1)) and np.array_equal(n_used, want['n_used'])
    bound = sums_bound(table, N, d, want['counts'], valid)
    assert (np.abs(sums - want['sums']) <= bound).all()
    assert np.array_equal(ind, sobol.indices_from_sums(sums, n_used, d)[0], equal_nan=True)
    # without the status the NaN reaches every sum of the row
    assert np.isnan(run(engine0, table, N, d, 0)[1]).all()


# ---- edges -------------------------------------------------------------------------------------------------------------------------

def test_constant_row_and_no_rows(engine0):
    N, d = 67, 7
    E = N * (d + 2)
    table = real_table(3, N, d)
    table[1] = 3.5
    ind, sums, n_used, _ = run(engine0, table, N, d, 4)
    assert np.isnan(ind[:, :, 1]).all() and np.isfinite(ind[:, :, [0, 2]]).all()
    ind, sums, n_used, info = engine0.sobol_indices(torch.empty((0, E), dtype=torch.float64, device=engine0.tdev), N, d, n_boot=4)
    assert tuple(ind.shape) == (2, d, 0, 5) and info['kernel_ms'] == 0.0 and info['n_valid'] == 0 and info['n_resamples'] == 5
    assert int(n_used.abs().sum()) == 0                                   # nothing was launched: n_used is as allocated


def test_abi_argument_errors(engine0):
    N, d = 5, 3
    E = N * (d + 2)
    lo, hi = box(d)
    target = np.array([2, abi.MCMC_TARGET_F_TDP, abi.MCMC_TARGET_NONE], dtype=np.int32)
    f64 = dict(dtype=torch.float64, device=engine0.tdev)
    x, mp, ft = torch.full((d, E), SENTINEL, **f64), torch.full((marshal.NP_M, E), SENTINEL, **f64), torch.full((E,), SENTINEL, **f64)
    nan = float('nan')

    def design(N_=N, lo_=lo, hi_=hi, tg=target, mp_=mp, ft_=ft, x_=x):
        return engine0.sobol_design(N_, lo_, hi_, tg, mp_, ft_, x=x_)

    bad = [dict(N_=1), dict(N_=32769), dict(lo_=np.zeros(17), hi_=np.ones(17), tg=np.full(17, -2)),
           dict(lo_=np.array([0.0, 1.0, 0.0]), hi_=np.array([1.0, 1.0, 1.0])), dict(lo_=np.array([nan, 0.0, 0.0])),
           dict(hi_=np.array([1.0, nan, 1.0])), dict(tg=np.array([2, -3, 0])), dict(tg=np.array([marshal.NP_M, 0, 1])),
           dict(tg=np.array([4, 4, -2])), dict(mp_=None), dict(ft_=None)]
    for kw in bad:
        with pytest.raises(engine.EngineError, match=r'simplyp_sobol_design failed \(-1\): simplyp_sobol_design'):
            design(**kw)
    L = engine.lib()
    dbl, i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    rc = L.simplyp_sobol_design(engine0._h, N, d, C.c_uint64(0), lo.ctypes.data_as(dbl), hi.ctypes.data_as(dbl), target.ctypes.data_as(i32),
                                None, None, mp.data_ptr(), ft.data_ptr(), None)
    assert rc == -1 and L.simplyp_last_error(engine0._h).decode().startswith('simplyp_sobol_design: ')
    assert (x == SENTINEL).all() and (mp == SENTINEL).all() and (ft == SENTINEL).all()
    design()
    assert np.array_equal(x.cpu().numpy(), sobol.design(N, lo, hi))

    table = dev(engine0, real_table(2, N, d))
    ind = torch.full((2, d, 2, 3), SENTINEL, **f64)

    def indices(N_=N, d_=d, n_rows=2, table_=table.data_ptr(), n_boot=2, ind_=ind.data_ptr()):
        rc = L.simplyp_sobol_indices(engine0._h, N_, d_, n_rows, table_, None, n_boot, C.c_uint64(0), None, None, ind_, None)
        return rc, L.simplyp_last_error(engine0._h).decode()

    for kw in (dict(N_=1), dict(N_=32769), dict(d_=0), dict(d_=17), dict(n_rows=-1), dict(n_boot=-1), dict(table_=None), dict(ind_=None)):
        rc, msg = indices(**kw)
        assert rc == -1 and msg.startswith('simplyp_sobol_indices: '), (kw, rc, msg)
    torch.cuda.synchronize()
    assert (ind == SENTINEL).all()
    assert indices(n_rows=0, table_=None, ind_=None)[0] == 0 and (ind == SENTINEL).all()
    assert indices()[0] == 0
    assert np.array_equal(ind.cpu().numpy(), sobol.indices_from_sums(*run(engine0, table.cpu().numpy(), N, d, 2)[1:3], d)[0])
    with pytest.raises(ValueError, match='member axis has'):
        engine0.sobol_indices(table, N + 1, d)


# ---- the percentile interval -----------------------------------------------------------------------------------------------------

def test_quantiles_of_the_bootstrap_axis(engine0):
    N, d, n_rows, n_boot = 260, 2, 3, 70
    table = real_table(n_rows, N, d, seed=5)
    want = sobol.sobol_indices(table, N, d, n_boot=n_boot, seed=11)
    ind_d, sums_d, n_used_d, _ = engine0.sobol_indices(dev(engine0, table), N, d, n_boot=n_boot, seed=11)
    q = [0.025, 0.975]
    lower, upper, info = engine0.quantiles(ind_d[..., 1:].contiguous(), q)
    got = engine.interpolate_quantiles(lower.cpu().numpy(), upper.cpu().numpy(), q, info['n_used'])
    ref = np.quantile(want['indices'][..., 1:], q, axis=-1)
    # the summation bound of the sums, propagated to first order through the ratios, plus 8 roundings of the ratio itself; an order
    # statistic moves by no more than the largest move of a resample
    e = sums_bound(table, N, d, want['counts'])                            # [B, n_rows, T]
    s, n_c = want['sums'], want['n_used'].astype(np.float64)[:, None]
    var = want['var'].T                                                    # [B, n_rows]
    e_var = e[:, :, 1] / (2 * n_c) + 2 * np.abs(s[:, :, 0] / (2 * n_c)) * e[:, :, 0] / (2 * n_c)
    idx = want['indices'].transpose(0, 3, 2, 1)                            # [2, B, n_rows, d]
    e_idx = np.stack([e[:, :, 2:2 + d], 0.5 * e[:, :, 2 + d:]]) / (n_c * var)[None, :, :, None] \
        + np.abs(idx) * (e_var / var)[None, :, :, None] + 8 * U53 * np.abs(idx)
    bound = e_idx[:, 1:].max(axis=1).transpose(0, 2, 1)                     # [2, d, n_rows]
    assert info['n_used'] == n_boot and got.shape == ref.shape == (2, 2, d, n_rows)
    assert (np.abs(got - ref) <= bound[None]).all(), (np.abs(got - ref).max(), bound.min())
    assert (got[0] < got[1]).all()


# ---- the public call -------------------------------------------------------------------------------------------------------------

N_PUB, BOOT_PUB, SEED_PUB = 64, 16, 5
COLS_PUB = ['Qr', 'PP_kg/day']


def public(**kw):
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
    priors = {'fc': (200.0, 380.0), 'T_g': (45.0, 85.0), 'a_Q': (0.3, 0.7)}
    args = dict(priors=priors, n_base=N_PUB, columns=COLS_PUB, reduce='annual', n_boot=BOOT_PUB, seed=SEED_PUB, keep_table=True)
    args.update(kw)
    return sp.sobol_indices(met, p_struc, p_SU, p_LU, p_SC, p, dyn, **args), args['priors'], (p_LU, p_SC)


@pytest.fixture(scope='module')
def pub(engine0):
    return public()


def test_public_call_end_to_end(engine0, pub):
    res, priors, frames = pub
    names, d = res['names'], 3
    E = N_PUB * (d + 2)
    assert names == ['fc', 'T_g', 'a_Q'] and res['columns'] == COLS_PUB and res['n_valid'] == N_PUB
    lo, hi = np.array([priors[n][0] for n in names]), np.array([priors[n][1] for n in names])
    assert np.array_equal(res['x'], sobol.design(N_PUB, lo, hi, seed=SEED_PUB)) and int(res['status'].max()) == 0
    # an independent ensemble run of the same members gives the same table, bit for bit: members are independent
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
    ens = sp.run_simply_p_ensemble(met, p_struc, p_SU, p_LU, p_SC, p, dyn, overrides={n: res['x'][k] for k, n in enumerate(names)},
                                   outputs=COLS_PUB, reduce='annual')
    table = np.stack([ens['data'][list(ens['columns']).index(c)] for c in COLS_PUB])          # [n_cols, P, R, E]
    assert table.shape == res['table'].shape == (2, 1, len(res['reaches']), E)
    assert np.array_equal(table, res['table'])
    rows = table.reshape(-1, E)
    want = sobol.sobol_indices(rows, N_PUB, d, n_boot=BOOT_PUB, seed=SEED_PUB)
    bound = sums_bound(rows, N_PUB, d, want['counts'][:1])[0]                                 # [n_rows, T]
    var = want['var'][:, 0]
    e_var = bound[:, 1] / (2 * N_PUB) + 2 * np.abs(want['sums'][0, :, 0] / (2 * N_PUB)) * bound[:, 0] / (2 * N_PUB)
    for plane, key, e_t in ((0, 'S1', bound[:, 2:2 + d]), (1, 'ST', 0.5 * bound[:, 2 + d:])):
        ref = want['indices'][plane, :, :, 0]                                                  # [d, n_rows]
        tol = (e_t / (N_PUB * var[:, None])).T + np.abs(ref) * (e_var / var)[None] + 8 * U53 * np.abs(ref)
        got = res[key].reshape(d, -1)
        assert res[key].shape == (d, 2, 1, len(res['reaches'])) and (np.abs(got - ref) <= tol).all(), (key, np.abs(got - ref).max(), tol.min())
    assert np.allclose(res['var'].ravel(), var, rtol=1e-12) and (var > 0).all()
    assert res['S1_conf'].shape == (2, d, 2, 1, len(res['reaches'])) and (res['ST_conf'][0] <= res['ST_conf'][1]).all()
    assert (res['ST'] > -0.5).all() and (res['ST'] < 2.0).all()
    for k in ('run_kernel_ms', 'design_ms', 'counts_ms', 'contract_ms', 'wall_ms'):
        assert res['stats'][k] > 0.0, k
    # the caller's frames: edited exactly as run_simply_p edits them
    met, p_struc, p_SU, p_LU2, p_SC2, p, dyn = helpers.scenario_inputs(NAME)
    sp.run_simply_p(met, p_struc, p_SU, p_LU2, p_SC2, p, dyn)
    pd.testing.assert_frame_equal(frames[0], p_LU2)
    pd.testing.assert_frame_equal(frames[1], p_SC2)


def test_public_call_with_observations_and_unit_samples(engine0, pub):
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
    obs_dict = helpers.observations(p_SU['st_dt'], p_SU['end_dt'])
    unit = np.random.default_rng(1).random((2, 4, 16))
    res, priors, _ = public(priors={'fc': (200.0, 380.0), 'T_g': (45.0, 85.0), 'a_Q': (0.3, 0.7), 'f_TDP': (0.3, 0.7)}, n_base=16,
                            obs_dict=obs_dict, unit_samples=unit, reduce='total', n_boot=8)
    lo, hi = np.array([v[0] for v in priors.values()]), np.array([v[1] for v in priors.values()])
    assert np.array_equal(res['x'], sobol.design(16, lo, hi, unit=unit))
    g = res['gof']
    R = len(res['reaches'])
    assert g['S1'].shape == g['ST'].shape == (4, len(abi.GOF_STATS), len(abi.GOF_VARS), R) and g['S1_conf'].shape == (2,) + g['S1'].shape
    nse_q = g['ST'][:, abi.GOF_STATS.index('NSE'), abi.GOF_VARS.index('Q'), 0]
    assert np.isfinite(nse_q).all() and np.isfinite(g['S1'][:, abi.GOF_STATS.index('NSE'), abi.GOF_VARS.index('Q'), 0]).all()
    assert g['n_valid'] == 16 and res['S1'].shape == (4, 2, 1, R)
    # f_TDP moves no period sum of the run: its total-order index of the flows is exactly 0
    assert (res['ST'][3] == 0.0).all() and (res['S1'][3] == 0.0).all()
