"""Warm start on the device: a run of D1 + D2 days and a run of D1 days followed by a run of D2 days started from the first one's
state (simplyp_set_state) give the same tables, status, right-hand-side counts and final state, bit for bit -- for every integrator,
kernel path, lane layout and member order; the state means what include/simplyp.h says; a resumed run meets the reference's rows.

"Equal" throughout: np.array_equal(..., equal_nan=True) on the tables laid end to end, equal status (OR over the pieces), equal
summed rhs_evals / steps / rejected and per-member right-hand-side counts, equal final state.

Small ensembles over two or three years: the file takes 13 s on one MI355X."""

import copy
import ctypes
import os
import re
import subprocess

import numpy as np
import pandas as pd
import pytest

import helpers
import simplyp_amd as sp
from simplyp_amd import abi, engine, marshal

pytestmark = pytest.mark.gpu

ROW = {r: i for i, r in enumerate(abi.STATE_ROWS)}


def copy_opts(o):
    c = type(o)()
    ctypes.memmove(ctypes.byref(c), ctypes.byref(o), ctypes.sizeof(o))
    return c


def days(m, lo, hi, **over):
    """The problem `m` over days [lo, hi) (a shallow copy with its own opts)."""
    p = dict(m)
    p['forcing'] = np.ascontiguousarray(m['forcing'][:, :, lo:hi])
    p['doy'] = np.ascontiguousarray(m['doy'][lo:hi])
    p['opts'] = copy_opts(m['opts'])
    for k, v in over.items():
        setattr(p['opts'], k, v)
    if m.get('period_of_day') is not None:
        pod = np.asarray(m['period_of_day'])[lo:hi]
        p['period_of_day'] = np.ascontiguousarray(pod - pod.min(), dtype=np.int32)
        p['opts'].n_periods = int(p['period_of_day'].max()) + 1
    return p


def run(eng, m, state_in=None, state_out=True, **kw):
    """One engine run; the table comes back in MEMBER order whatever opts.out_slot_order says."""
    import torch
    E = m['member_params'].shape[1]
    rhs = torch.zeros(E, dtype=torch.int32, device=eng.tdev)
    out, status, stats = eng.run(m['forcing'], m['doy'], m['member_params'], m['reach_params'], m['up_ptr'], m['up_idx'], m['opts'],
                                 out_reaches=m.get('out_reaches'), forcing_of_member=m.get('fom'), period_of_day=m.get('period_of_day'),
                                 member_rhs=rhs, state_in=state_in, state_out=state_out, **kw)
    out = out.cpu().numpy()
    if m['opts'].out_slot_order:
        mos = stats['member_of_slot'].cpu().numpy()
        by_member = np.empty_like(out)
        by_member[..., mos] = out
        out = by_member
    return dict(out=out, status=status.cpu().numpy(), stats=stats, member_rhs=rhs.cpu().numpy().astype(np.int64),
                state=stats.get('state'))


def run_pieces(eng, m, cuts, piece_opts=None, alias=False):
    """Days [0, D) in pieces cut at `cuts`, the state threaded through on the device.  piece_opts: per piece, opts fields to override."""
    D = m['forcing'].shape[2]
    edges = [0] + list(cuts) + [D]
    state, parts = None, []
    for k, (lo, hi) in enumerate(zip(edges, edges[1:])):
        p = days(m, lo, hi, **((piece_opts or {}).get(k, {})))
        r = run(eng, p, state_in=state, state_out=state if (alias and state is not None) else True)
        if alias and state is not None:
            assert r['state'].data_ptr() == state.data_ptr()
        state = r['state']
        parts.append(r)
    return parts


def assert_pieces_equal_whole(whole, parts, what=None):
    out = np.concatenate([p['out'] for p in parts], axis=1)
    assert out.shape == whole['out'].shape
    assert np.array_equal(out, whole['out'], equal_nan=True), what
    status = np.bitwise_or.reduce([p['status'] for p in parts])
    assert np.array_equal(status, whole['status']), what
    for k in ('rhs_evals', 'steps', 'rejected'):
        assert sum(p['stats'][k] for p in parts) == whole['stats'][k], (k, what)
    assert np.array_equal(sum(p['member_rhs'] for p in parts), whole['member_rhs']), what
    assert np.array_equal(parts[-1]['state'].cpu().numpy(), whole['state'].cpu().numpy(), equal_nan=True), what


def tiled(name, E, n_tiles, solver=None, out_mask=None):
    m = helpers.marshal_scenario(name, E=E, solver=solver, out_mask=out_mask)
    m['forcing'] = np.ascontiguousarray(np.tile(m['forcing'], (1, 1, n_tiles)))
    m['doy'] = np.ascontiguousarray(np.tile(m['doy'], n_tiles))
    return m


def perturb(m, E, seed=41):
    rng = np.random.default_rng(seed)
    for pname, lo, hi in (('a_Q', 0.6, 1.6), ('T_s_A', 0.5, 2.0), ('fc', 0.8, 1.2)):
        m['member_params'][marshal.PM_NAMES.index(pname)] *= rng.uniform(lo, hi, E)
    return m


# ---- 1. split == unsplit on one reach: a covering set of integrator x lanes x kernel path x balance x slot order x step_len ----
# every value of every axis at least twice, every integrator on both kernel paths (RK4: the chain kernel only)
SOLVERS = {'rk4': dict(integrator='rk4', substeps=32), 'cashkarp': dict(integrator='cashkarp'), 'aug': dict(integrator='cashkarp_aug'),
           'f32': dict(integrator='cashkarp_aug_f32', rtol=1e-5, atol=1e-7)}
COVER = [  # integrator, lanes per member, queue, balance, out_slot_order, step_len
    ('rk4', 1, 0, 0, 0, 1.0), ('rk4', 1, 0, 0, 1, 2.0),
    ('cashkarp', 1, 0, 1, 0, 1.0), ('cashkarp', 1, 1, 0, 1, 2.0), ('cashkarp', 1, 1, 1, 1, 1.0),
    ('aug', 1, 0, 0, 1, 1.0), ('aug', 1, 1, 1, 0, 2.0), ('aug', 4, 0, 1, 1, 2.0), ('aug', 4, 1, 0, 0, 1.0), ('aug', 4, 1, 1, 1, 1.0),
    ('f32', 1, 0, 1, 1, 2.0), ('f32', 1, 1, 1, 0, 1.0)]


def test_the_covering_set_covers():
    for axis, values in ((0, SOLVERS), (1, (1, 4)), (2, (0, 1)), (3, (0, 1)), (4, (0, 1)), (5, (1.0, 2.0))):
        for v in values:
            assert sum(1 for c in COVER if c[axis] == v) >= 2, (axis, v)
    for integ in SOLVERS:
        assert {c[2] for c in COVER if c[0] == integ} == ({0} if integ == 'rk4' else {0, 1})


@pytest.mark.parametrize('integ,lanes,queue,balance,slot_order,step_len', COVER)
def test_split_equals_unsplit(engine0, integ, lanes, queue, balance, slot_order, step_len):
    """tarland_2004_dynamic tiled to 1098 days (5 time chunks of 256), 150 perturbed members, cut in two at day 500 and in three at
    days 400 and 750 -- none of them a multiple of 64, so neither a chunk nor a 256-day forcing-tile boundary.  With the balancer on
    (pilot 80 days) every piece orders its members by its own pilot: the pieces run in different member orders."""
    E = 150
    solver = dict(SOLVERS[integ], lanes_per_member=lanes if integ == 'aug' else 0, time_chunk_days=256 if queue else -1, balance=balance,
                  balance_pilot_days=80, out_slot_order=slot_order)
    m = perturb(tiled('tarland_2004_dynamic', E, 3, solver=solver), E)
    m['opts'].step_len = step_len
    whole = run(engine0, m)
    assert whole['stats']['queued'] == queue and whole['stats']['balanced'] == balance
    if integ == 'aug':
        assert whole['stats']['lanes_per_member'] == lanes and whole['status'].max() == 0
    assert np.isfinite(whole['out'][..., whole['status'] == 0]).all() and (whole['status'] == 0).sum() > E // 2
    for cuts in ([500], [400, 750]):
        assert all(c % 64 for c in cuts)
        parts = run_pieces(engine0, m, cuts)
        assert all(p['stats']['queued'] == queue and p['stats']['balanced'] == balance for p in parts)
        assert_pieces_equal_whole(whole, parts, cuts)
    if integ == 'rk4':        # no trial step to carry: the row holds step_len / substeps
        assert (whole['state'].cpu().numpy()[:, ROW['h_next']] == step_len / 32).all()
    assert (whole['state'].cpu().numpy()[:, ROW['D_snow']] == 0.0).all()          # opts.snow = 0


# ---- 2. networks: the chain kernel walks every reach of a member, the pipelined queue hands them over between waves ----
def network_problem(name, queue):
    solver = dict(time_chunk_days=256 if queue else -1, balance=0)
    if name == 'branch':
        return helpers.branch_network_inputs(12, '1981-01-01', '1982-12-31', solver=solver)
    E = 20
    m = tiled(name, E, 2, solver=solver)
    m['member_params'][marshal.PM_NAMES.index('a_Q')] *= np.linspace(0.6, 1.6, E)
    return m


@pytest.mark.parametrize('queue', [0, 1])
@pytest.mark.parametrize('name', ['chain4_val_2004', 'stiff_chain12_2004', 'branch', 'net5_static_erod_val_2004'])
def test_split_equals_unsplit_on_networks(engine0, name, queue):
    """The 4-reach chain, the stiff 12-reach chain, the branching 22-reach network and the five reaches under static EPC0 (constant conc_*,
    Plab_NC and TDPs_NC rows of S-type new land) over two years, the second pair on, cut at day 300: one state per (reach, member), chain
    kernel and pipelined task queue."""
    m = network_problem(name, queue)
    whole = run(engine0, m)
    S = m['reach_params'].shape[1]
    assert whole['stats']['queued'] == queue and whole['stats']['stiff_pair'] == 1 and S > 1
    assert tuple(whole['state'].shape) == (S, 16, m['member_params'].shape[1])
    parts = run_pieces(engine0, m, [300])
    assert all(p['stats']['queued'] == queue for p in parts)
    assert_pieces_equal_whole(whole, parts)


# ---- 3. the state belongs to the model, not to a kernel configuration ----
def test_state_written_by_one_configuration_is_consumed_by_another(engine0):
    """First piece four lanes per member through the task queue, second piece one lane through the chain kernel == the unsplit
    one-lane chain run (integrator 2): rests on the 1-lane == 4-lane and chain == queue identities."""
    E = 150
    m = perturb(tiled('tarland_2004_dynamic', E, 3, solver=dict(lanes_per_member=1, time_chunk_days=-1, balance=0)), E)
    whole = run(engine0, m)
    assert whole['stats']['queued'] == 0 and whole['stats']['lanes_per_member'] == 1
    parts = run_pieces(engine0, m, [500], piece_opts={0: dict(lanes_per_member=4, time_chunk_days=256, balance=1, balance_pilot_days=80),
                                                       1: dict(lanes_per_member=1, time_chunk_days=-1)})
    assert (parts[0]['stats']['lanes_per_member'], parts[0]['stats']['queued'], parts[0]['stats']['balanced']) == (4, 1, 1)
    assert (parts[1]['stats']['lanes_per_member'], parts[1]['stats']['queued']) == (1, 0)
    assert_pieces_equal_whole(whole, parts)


# ---- 4. in-kernel snow ----
@pytest.mark.parametrize('queue', [0, 1])
def test_snow_depth_is_part_of_the_state(engine0, queue):
    """opts.snow = 1 with perturbed f_DDSM / D_snow_0, the D_snow column requested, cut in mid-winter (1982-01-12) with snow on
    the ground."""
    E = 96
    m = helpers.marshal_scenario('tarland_1981_2010_dynamic', E=E, snow=True, out_mask=marshal.MASK_REACH5 | marshal.MASK_D_SNOW,
                                 solver=dict(time_chunk_days=256 if queue else -1, balance=0))
    m = days(m, 0, 800)
    rng = np.random.default_rng(11)
    m['member_params'][marshal.PM_NAMES.index('f_DDSM')] = rng.uniform(0.5, 6.0, E)
    m['member_params'][marshal.PM_NAMES.index('D_snow_0')] = rng.uniform(0.0, 40.0, E)
    cut = 376
    assert str(m['met'].index[cut].date()) == '1982-01-12'
    whole = run(engine0, m)
    assert whole['stats']['queued'] == queue and whole['status'].max() == 0
    parts = run_pieces(engine0, m, [cut])
    at_cut = parts[0]['state'].cpu().numpy()[0, ROW['D_snow']]
    assert (at_cut > 0).any(), "no member has snow on the ground at the cut"
    assert np.array_equal(at_cut, whole['out'][-1, cut - 1, 0])          # the D_snow column is the last one
    assert_pieces_equal_whole(whole, parts)
    assert not np.array_equal(whole['out'][-1, :, 0, 0], whole['out'][-1, :, 0, 1])


# ---- 5. time-reduced rows, several forcing sets, state_in aliasing state_out ----
def test_annual_sums_forcing_sets_and_aliased_state(engine0):
    """reduce = annual sums over 1981-1983 cut at 1 January 1982 and 1983: the per-year rows equal the unsplit run's; three
    forcing sets with forcing_of_member; every resumed piece reads and writes ONE state buffer (state_in == state_out)."""
    E = 150
    m = helpers.marshal_scenario('tarland_1981_2010_dynamic', E=E, out_mask=marshal.MASK_REACH5,
                                 solver=dict(time_chunk_days=256, balance=1, balance_pilot_days=80))
    m = perturb(days(m, 0, 1095), E)
    f = m['forcing']
    m['forcing'] = np.ascontiguousarray(np.concatenate([f, f * np.array([1.1, 1.0])[None, :, None], f * np.array([0.9, 1.05])[None, :, None]]))
    m['fom'] = (np.arange(E) % 3).astype(np.int32)
    years = np.asarray(m['met'].index.year[:1095])
    m['period_of_day'] = np.ascontiguousarray(years - years.min(), dtype=np.int32)
    m['opts'].n_periods = 3
    whole = run(engine0, m)
    assert whole['out'].shape[1] == 3 and whole['stats']['queued'] == 1
    assert not np.array_equal(whole['out'][..., 0], whole['out'][..., 1])
    parts = run_pieces(engine0, m, [365, 730], alias=True)
    assert [p['out'].shape[1] for p in parts] == [1, 1, 1]
    assert_pieces_equal_whole(whole, parts)
    # and on daily rows, with the aliased buffer on the chain kernel
    m['period_of_day'] = None
    m['opts'].n_periods = 0
    m['opts'].time_chunk_days = -1
    whole = run(engine0, m)
    assert_pieces_equal_whole(whole, run_pieces(engine0, m, [365, 730], alias=True))


# ---- 6. the state means what the header says ----
@pytest.mark.parametrize('name,snow', [('tarland_2004_dynamic', False), ('tarland_2004_dynamic', True), ('chain4_val_2004', False)])
def test_state_rows_are_the_last_days_columns(engine0, name, snow):
    E = 24
    mask = marshal.MASK_ALL | (marshal.MASK_D_SNOW if snow else 0)
    m = helpers.marshal_scenario(name, E=E, snow=snow, out_mask=mask)
    m['member_params'][marshal.PM_NAMES.index('fc')] *= np.linspace(0.85, 1.15, E)
    m['member_params'][marshal.PM_NAMES.index('T_g')] *= np.linspace(0.7, 1.4, E)
    if snow:
        m['member_params'][marshal.PM_NAMES.index('f_DDSM')] = np.linspace(0.5, 6.0, E)
        m = days(m, 0, 40)                                       # ends in February, snow on the ground for the slow melters
    r = run(engine0, m)
    state, last = r['state'].cpu().numpy(), r['out'][:, -1]           # [S, 16, E], [n_cols, S, E]
    col = {c: i for i, c in enumerate(marshal.columns_of_mask(mask))}
    same = {'VsA': 'VsA', 'VsS': 'VsS', 'Vr': 'Vr', 'Qr': 'Qr_EndOfDay', 'Msus': 'Msus_EndOfDay', 'TDPr': 'TDPr_EndOfDay',
            'PPr': 'PPr_EndOfDay', 'TDPs_A': 'TDPs_A_kg', 'Plab_A': 'P_labile_A_kg', 'conc_TDPs_A': 'conc_TDPs_A_kgmm',
            'TDPs_NC': 'TDPs_NC_kgmm', 'Plab_NC': 'P_labile_NC_kg', 'conc_TDPs_NC': 'conc_TDPs_NC_kgmm'}
    for row, c in same.items():
        assert np.array_equal(state[:, ROW[row]], last[col[c]]), (row, c)
    T_g = m['member_params'][marshal.PM_NAMES.index('T_g')]
    assert np.array_equal(state[:, ROW['Vg']], last[col['Qg']] * T_g[None, :])       # the carried value after the day-end reset
    if snow:
        assert np.array_equal(state[:, ROW['D_snow']], last[col['D_snow']]) and (state[:, ROW['D_snow']] > 0).any()      # (0.67 mm left at f_DDSM = 0.5)
    else:
        assert (state[:, ROW['D_snow']] == 0.0).all()
    h = state[:, ROW['h_next']]
    assert (h > 0).all() and np.isfinite(h).all()


# ---- 7. member order ----
def test_permuting_members_permutes_tables_and_state(engine0):
    """balance = 1 on an ensemble large enough that the balancer reorders: parameters and state columns permuted alike give the
    permuted tables and the permuted state."""
    E = 4000
    m = helpers.marshal_scenario('tarland_2004_dynamic', E=E, out_mask=marshal.MASK_REACH5,
                                 solver=dict(time_chunk_days=256, balance=1, balance_pilot_days=40))
    m = perturb(m, E, seed=5)
    first = run(engine0, days(m, 0, 170))
    assert first['stats']['balanced'] == 1
    second = run(engine0, days(m, 170, 366), state_in=first['state'])
    assert second['stats']['balanced'] == 1
    perm = np.random.default_rng(3).permutation(E)
    mp_ = dict(m, member_params=np.ascontiguousarray(m['member_params'][:, perm]),
               reach_params=np.ascontiguousarray(m['reach_params'][:, :, perm]))
    import torch
    st_perm = first['state'][..., torch.as_tensor(perm, device=first['state'].device)].contiguous()
    got = run(engine0, days(mp_, 170, 366), state_in=st_perm)
    assert np.array_equal(got['out'], second['out'][..., perm], equal_nan=True)
    assert np.array_equal(got['status'], second['status'][perm]) and np.array_equal(got['member_rhs'], second['member_rhs'][perm])
    assert np.array_equal(got['state'].cpu().numpy(), second['state'].cpu().numpy()[..., perm], equal_nan=True)
    assert not np.array_equal(got['out'], second['out'])


# ---- 8. against the reference, independent of the device's own uncut run ----
@pytest.mark.parametrize('name', ['tarland_2004_dynamic', 'chain4_val_2004'])
def test_resumed_second_half_against_the_reference(engine0, name):
    """The second half of the year, started from the first half's state, against the rows of those days in the tables the unmodified
    reference made for the whole year: north_star's bar (< 1e-6) on every reach column of every reach."""
    m = helpers.marshal_scenario(name, E=1)
    cut = 183
    first = run(engine0, days(m, 0, cut))
    second = run(engine0, days(m, cut, 366), state_in=first['state'])
    assert first['status'].max() == 0 and second['status'].max() == 0
    gold = helpers.golden_tables(name, 'tight')
    for j, sc in enumerate(m['scs']):
        for c in helpers.REACH_COLS:
            ref = gold['R'][sc][c].values
            err = helpers.max_rel_err(second['out'][marshal.OUT_COLUMNS.index(c), :, j, 0], ref[cut:], floor=1e-300)
            assert err < 1e-6, (sc, c, err)


def test_resumed_second_year_of_the_branch_network_against_the_reference(engine0):
    pr, tables = helpers.branch_network_problem()
    cut = 365
    first = run(engine0, days(pr, 0, cut))
    second = run(engine0, days(pr, cut, pr['forcing'].shape[2]), state_in=first['state'])
    assert second['status'].max() == 0
    for (k, j), tab in tables.items():
        for i, c in enumerate(helpers.REACH_COLS):
            err = helpers.max_rel_err(second['out'][marshal.OUT_COLUMNS.index(c), :, j, k], tab[cut:, i], floor=1e-300)
            assert err < 1e-6, (k, j, c, err)


def test_run_simply_p_drop_in_resumed(engine0):
    """run_simply_p(initial_state=...) over the second half of 2004 at the drop-in test's bars on all columns the reference returns;
    and the default call is unchanged (no 'state' key)."""
    name, cut = 'tarland_2004_dynamic', 183
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(name)
    _, _, _, od1 = sp.run_simply_p(met.iloc[:cut], p_struc, p_SU, p_LU, p_SC, p, dyn, return_state=True)
    st = od1['state']
    assert st['rows'] == abi.STATE_ROWS and st['data'].shape == (1, 16, 1) and st['end'] == met.index[cut - 1]
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(name)
    df_TC, df_R, Kf, od2 = sp.run_simply_p(met.iloc[cut:], p_struc, p_SU, p_LU, p_SC, p, dyn, initial_state=st)
    assert 'state' not in od2 and od2['member_status'] == 0
    gold = helpers.golden_tables(name, 'tight')
    for sc in gold['R']:
        assert df_R[sc].index.equals(met.index[cut:])
        for c in gold['R'][sc].columns:
            assert helpers.max_rel_err(df_R[sc][c].values, gold['R'][sc][c].values[cut:], floor=1e-300) < 1e-6, (sc, c)
        for c in gold['TC'][sc].columns:
            tol = 2e-5 if c in ('QsA', 'QsS', 'QsNC') else 1e-6
            assert helpers.max_rel_err(df_TC[sc][c].values, gold['TC'][sc][c].values[cut:], floor=1e-9) < tol, (sc, c)
    with pytest.raises(ValueError, match='must start on'):
        sp.run_simply_p(met.iloc[cut + 1:], p_struc, p_SU, p_LU, p_SC, p, dyn, initial_state=st)


# ---- 9. one-shot semantics ----
def test_the_arm_is_one_shot(engine0):
    import torch
    E = 70
    m = perturb(helpers.marshal_scenario('tarland_2004_dynamic', E=E, out_mask=marshal.MASK_REACH5), E)
    a, b = days(m, 0, 200), days(m, 200, 366)
    cold = run(engine0, b)
    first = run(engine0, a)
    warm = run(engine0, b, state_in=first['state'])
    assert not np.array_equal(warm['out'], cold['out'])

    L, h = engine.lib(), engine0._h
    poison = torch.full((1, 16, E), float('nan'), dtype=torch.float64, device=engine0.tdev)
    sink = torch.zeros((1, 16, E), dtype=torch.float64, device=engine0.tdev)

    def arm(si, so):
        assert L.simplyp_set_state(h, None if si is None else ctypes.c_void_p(si.data_ptr()),
                                   None if so is None else ctypes.c_void_p(so.data_ptr())) == 0

    def plain_run(p):
        """eng.run's own call sequence minus its simplyp_set_state: what a C caller that never arms does"""
        f, dy = engine0.to_device(p['forcing'], torch.float64), engine0.to_device(p['doy'], torch.int32)
        mp, rp = engine0.to_device(p['member_params'], torch.float64), engine0.to_device(p['reach_params'], torch.float64)
        D = f.shape[2]
        out = torch.empty((5, D, 1, E), dtype=torch.float64, device=engine0.tdev)
        status = torch.empty(E, dtype=torch.int32, device=engine0.tdev)
        dims, stats = abi.Dims(E, 1, D, 1), abi.Stats()
        up = np.zeros(2, dtype=np.int32)
        torch.cuda.synchronize()
        rc = L.simplyp_run(h, ctypes.byref(dims), ctypes.byref(p['opts']), f.data_ptr(), dy.data_ptr(), None, None, mp.data_ptr(),
                           rp.data_ptr(), up.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), None, None, 0, out.data_ptr(),
                           status.data_ptr(), None, None, ctypes.byref(stats))
        return rc, out.cpu().numpy()

    assert L.simplyp_ctx_set_stream(h, None) == 0
    # a refused run consumes the arm: the plain run that follows starts cold and writes no state
    arm(poison, sink)
    bad = copy_opts(b['opts'])
    bad.integrator = 99
    rc, _ = plain_run(dict(b, opts=bad))
    assert rc == -1
    rc, out = plain_run(b)
    assert rc == 0 and np.array_equal(out, cold['out']) and float(sink.abs().sum()) == 0.0
    # (NULL, NULL) disarms
    arm(poison, sink)
    arm(None, None)
    rc, out = plain_run(b)
    assert rc == 0 and np.array_equal(out, cold['out']) and float(sink.abs().sum()) == 0.0
    # and an arm that is left alone fires once
    arm(first['state'], sink)
    rc, out = plain_run(b)
    assert rc == 0 and np.array_equal(out, warm['out']) and torch.equal(sink, warm['state'])
    rc, out = plain_run(b)
    assert rc == 0 and np.array_equal(out, cold['out'])


def test_state_is_valid_after_sync_of_a_deferred_run(engine0):
    import torch
    E = 70
    m = perturb(helpers.marshal_scenario('tarland_2004_dynamic', E=E, out_mask=marshal.MASK_REACH5), E)
    first = run(engine0, days(m, 0, 200))
    warm = run(engine0, days(m, 200, 366), state_in=first['state'])
    b = days(m, 200, 366)
    s = torch.cuda.Stream(device=engine0.tdev)
    with torch.cuda.stream(s):
        out, status, stats = engine0.run(b['forcing'], b['doy'], b['member_params'], b['reach_params'], b['up_ptr'], b['up_idx'], b['opts'],
                                         state_in=first['state'], state_out=True, defer_sync=True)
        state = stats['state']
        stats.update(stats.pop('finish')())
    s.synchronize()
    assert np.array_equal(out.cpu().numpy(), warm['out']) and torch.equal(state, warm['state'])
    assert stats['rhs_evals'] == warm['stats']['rhs_evals']


# ---- 10. the Python layer ----
def test_annual_windows_of_an_ensemble(engine0):
    """run_simply_p_ensemble_windows(window='annual') over 1981-1985, 2 000 members: the windows' tables laid end to end are the
    single call's table; goodness of fit and percentile bands per window; two contexts on one GPU; tables left on the device."""
    import torch
    from simplyp_amd import synthetic
    E = 2000
    met_df, p_struc, p_SU, p_LU, p_SC, p, dyn = synthetic.tarland_inputs('1981-01-01', '1985-12-31', dynamic_epc0='y', dynamic_erod='n')
    over = synthetic.monte_carlo_overrides(p, p_LU, E, seed=synthetic.C3_SEED)
    args = lambda: (met_df, p_struc, copy.deepcopy(p_SU), p_LU.copy(), p_SC.copy(), p.copy(), dyn)
    one = sp.run_simply_p_ensemble(*args(), overrides=over, return_state=True)
    assert one['data'].shape == (5, len(met_df), 1, E) and one['state']['data'].shape == (1, 16, E)
    assert one['state']['end'] == met_df.index[-1] and one['state']['reaches'] == [1]

    def collect(**kw):
        items = []
        for w in sp.run_simply_p_ensemble_windows(*args(), window='annual', overrides=over, **kw):
            items.append(w)
        return items

    # plain: host tables
    items = collect()
    assert [w['window'][0].year for w in items] == [1981, 1982, 1983, 1984, 1985]
    assert [w['data'].shape[1] for w in items] == [365, 365, 365, 366, 365]
    assert np.array_equal(np.concatenate([w['data'] for w in items], axis=1), one['data'], equal_nan=True)
    assert np.array_equal(np.bitwise_or.reduce([w['status'] for w in items]), one['status'])
    for k in ('rhs_evals', 'steps', 'rejected'):
        assert sum(w['stats'][k] for w in items) == one['stats'][k]
    assert torch.is_tensor(items[-1]['state']['data'])
    assert np.array_equal(items[-1]['state']['data'].cpu().numpy(), one['state']['data'], equal_nan=True)
    # a later call continues from the last window's state; the date check holds
    with pytest.raises(ValueError, match='must start on'):
        sp.run_simply_p_ensemble(*args(), overrides=over, initial_state=items[-2]['state'])

    # goodness of fit and percentile bands per window, tables left on the device
    # (the shipped observations start in 2004: member 3's own flow on every fifth day stands in for them)
    A_catch = float(p_SC.loc['A_catch', 1])
    q3 = pd.Series(one['data'][one['columns'].index('Qr'), :, 0, 3] * A_catch * 1000 / 86400, index=met_df.index)
    obs = {1: pd.DataFrame({'Q': q3.iloc[::5]})}
    qs = [0.025, 0.5, 0.975]
    items = collect(obs_dict=obs, quantiles=qs, to_host=False)
    lo = 0
    ok = (one['status'] & abi.STATUS_NONFINITE) == 0
    for w in items:
        n = w['data'].shape[1]
        assert torch.is_tensor(w['data']) and np.array_equal(w['data'].cpu().numpy(), one['data'][:, lo:lo + n], equal_nan=True)
        gof = w['gof']['data'].cpu().numpy()
        assert gof.shape[-1] == E
        assert (gof[abi.GOF_STATS.index('N obs'), 0, 0] == len(range(lo + (-lo) % 5, lo + n, 5))).all()
        assert abs(gof[abi.GOF_STATS.index('NSE'), 0, 0, 3] - 1.0) < 1e-9 and gof[abi.GOF_STATS.index('NSE'), 0, 0, 4] < 1.0
        assert w['quantiles']['data'].shape == (3, 5, n, 1) and w['quantiles']['n_members'] == int(ok.sum())
        band = np.quantile(one['data'][:, lo:lo + n][..., ok], qs, axis=-1)
        assert helpers.max_rel_err(w['quantiles']['data'], band, floor=1e-300) < 1e-12
        lo += n

    # two contexts on one GPU
    items = collect(devices=[0, 0])
    assert np.array_equal(np.concatenate([w['data'] for w in items], axis=1), one['data'], equal_nan=True)
    assert items[0]['stats']['bounds'] == [[0, 1000], [1000, 2000]] and len(items[0]['state']['data']) == 2
    assert np.array_equal(np.concatenate([t.cpu().numpy() for t in items[-1]['state']['data']], axis=-1), one['state']['data'])

    # annual sums per window
    ann = sp.run_simply_p_ensemble(*args(), overrides=over, reduce='annual')
    items = collect(reduce='annual')
    assert np.array_equal(np.concatenate([w['data'] for w in items], axis=1), ann['data'], equal_nan=True)


def test_c_program_resumes_bit_for_bit(tmp_path, engine0):
    engine.build()
    root = os.path.dirname(engine.HERE)
    exe = str(tmp_path / 'resume_from_c')
    subprocess.check_call(['gcc', '-O2', '-Wall', '-Wextra', '-Werror', '-I' + os.path.join(root, 'include'),
                           os.path.join(root, 'examples', 'resume_from_c.c'), '-o', exe, '-L' + engine.CSRC, '-lsimplyp_hip',
                           '-Wl,-rpath,' + engine.CSRC, '-lm'])
    p = subprocess.run([exe, '130', '700', '333'], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr + p.stdout
    assert 'table identical, state identical, status identical, rhs_evals identical' in p.stdout
    tail = re.search(r'E=130 D=700 cut=333 flagged=0 rhs_evals=(\d+) = (\d+) \+ (\d+)', p.stdout)
    assert tail and int(tail.group(1)) == int(tail.group(2)) + int(tail.group(3))
