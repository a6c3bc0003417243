"""Shared test helpers: rebuild the reference-shaped pandas inputs of a golden scenario,
and compare result tables."""

import json
import os

import numpy as np
import pandas as pd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'data')      # the reference's shipped data files (workbook, met series, observations, example outputs)
_meta = None


def meta():
    global _meta
    if _meta is None:
        with open(os.path.join(GOLDEN, 'series_meta.json')) as fh:
            _meta = json.load(fh)
    return _meta


def _nan(v):
    return np.nan if v is None else v


def scenario_inputs(name):
    """(met_df, p_struc, p_SU, p_LU, p_SC, p, dynamic_options) exactly as the golden run got them."""
    info = meta()[name]['inputs']
    z = np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False)
    met = pd.DataFrame(z['met/values'], columns=[str(c) for c in z['met/columns']],
                       index=pd.to_datetime([str(d) for d in z['met/index']]))
    met.index.name = 'Date'
    p_SU = pd.Series({k: _nan(v) for k, v in info['p_SU'].items()}, dtype=object)
    pd_ = {k: _nan(v) for k, v in info['p'].items()}
    pd_['SC_list'] = np.asarray(pd_['SC_list'])
    p = pd.Series(pd_, dtype=object)
    p_LU = pd.DataFrame({c: {k: _nan(v) for k, v in col.items()} for c, col in info['p_LU'].items()}, dtype=float)
    p_LU = p_LU[['A', 'S', 'IG', 'NC']]
    p_SC = pd.DataFrame({int(c): {k: _nan(v) for k, v in col.items()} for c, col in info['p_SC'].items()}, dtype=float)
    rows = {int(i): {k: _nan(v) for k, v in row.items()} for i, row in info['p_struc'].items()}
    p_struc = pd.DataFrame.from_dict(rows, orient='index')
    p_struc['Upstream_SCs'] = p_struc['Upstream_SCs'].astype(object)
    p_struc.index.name = 'Reach'
    dyn = pd.Series(dict(info['dyn'], Dynamic_effluent_inputs='n', Dynamic_terrestrialP_inputs='n'))
    return met, p_struc, p_SU, p_LU, p_SC, p, dyn


def golden_tables(name, label):
    """{'R': {SC: DataFrame}, 'TC': {SC: DataFrame}} of the golden run `label` ('tight' | 'shipped')."""
    z = np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False)
    idx = pd.to_datetime([str(d) for d in z['met/index']])
    out = {'R': {}, 'TC': {}}
    for key in z.files:
        parts = key.split('/')
        if parts[0] != label or len(parts) != 2:
            continue
        kind = 'R' if parts[1].startswith('R') else 'TC'
        sc = int(parts[1][len(kind):])
        out[kind][sc] = pd.DataFrame(z[key], columns=[str(c) for c in z[key + '/columns']], index=idx)
    return out


def max_rel_err(a, b, floor=0.0):
    """max over elements of |a-b| / max(|b|, floor); NaN-in-both counts as equal."""
    a = np.asarray(a, dtype=float); b = np.asarray(b, dtype=float)
    both_nan = np.isnan(a) & np.isnan(b)
    denom = np.maximum(np.abs(b), floor)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.abs(a - b) / denom
    r = np.where((a == b) | both_nan, 0.0, r)
    return float(np.nanmax(r)) if r.size else 0.0


def marshal_scenario(name, E=1, out_mask=None, solver=None, snow=False):
    """Arrays + opts for engine/oracle `run` from a golden scenario (base parameters replicated E times)."""
    from simplyp_amd import marshal, abi
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = scenario_inputs(name)
    marshal.prologue(p_SU, p_LU, p_SC, p)
    up_ptr, up_idx, _ = marshal.topology(p_struc, p)
    mp = marshal.member_params(p, p_LU, E)
    rp = marshal.reach_params(p_SC, p, E)
    forcing, doy = marshal.forcing_arrays(met, snow=snow)
    scs = marshal.sc_list(p)
    opts = abi.make_opts(solver, dynamic_epc0=dyn['Dynamic_EPC0'] == 'y', dynamic_erod=dyn['Dynamic_erodibility'] == 'y',
                         run_mode_cal=p_SU.run_mode == 'cal', sc_qr0=scs.index(int(p['SC_Qr0'])),
                         out_mask=marshal.MASK_ALL if out_mask is None else out_mask, snow=snow)
    return dict(forcing=forcing, doy=doy, member_params=mp, reach_params=rp, up_ptr=up_ptr, up_idx=up_idx, opts=opts,
                scs=scs, met=met)


def observations(st_dt, end_dt):
    """obs_dict of the shipped Tarland observation workbooks (data/ at the repository root), truncated to the run
    period the way the reference's read_input_data does (inputs.py:118-152)."""
    from simplyp_amd import xlsx
    df_li = []
    for f in ('Coull_DailyMeanQ.xlsx', 'Coull_ChemObs.xlsx'):
        wb = xlsx.Workbook(os.path.join(DATA, f))
        df = xlsx.read_excel(wb, '1', index_col=0)
        df.index = pd.to_datetime(df.index)
        df_li.append(df.sort_index().truncate(before=st_dt, after=end_dt))
    return {1: pd.concat(df_li, axis=1)}


def gof_golden():
    with open(os.path.join(GOLDEN, 'gof_golden.json')) as fh:
        return json.load(fh)


def gof_case_factors(index):
    """The deterministic multiplicative perturbations of tests/golden/make_gof_golden.py (case -> Q and concentration factors)."""
    t = np.arange(len(index)) / 365.25
    return {'base': dict(Q=1.0, C=1.0),
            'wet': dict(Q=1.25 + 0.1 * np.sin(2 * np.pi * t), C=0.8),
            'dry': dict(Q=0.7, C=1.4 + 0.3 * np.cos(2 * np.pi * t / 3.0)),
            # one NEGATIVE observation of Q and of SS (the k-th of each): np.log of it is NaN, which the reference's sums skip
            'negobs': dict(Q=1.0, C=1.0, negate=dict(Q=17, SS=9))}


def gof_case_observations(obs, factors):
    """The observations of a case of gof_case_factors: a copy of obs_dict with the case's edits applied."""
    out = {k: df.copy() for k, df in obs.items()}
    for v, k in factors.get('negate', {}).items():
        day = out[1][v].dropna().index[k]
        out[1].loc[day, v] = -out[1].loc[day, v]
    return out


# Two valid integrations at the default solver's working tolerance (kernel and oracle mirror the same step rule, but an
# accept/reject decision may flip on rounding) agree to about ten times that tolerance.
def _working_tolerance():
    from simplyp_amd import abi
    return 10.0 * abi.DEFAULT_SOLVER['rtol']


TOL_WORKING = _working_tolerance()


def member_fixture_problem(fname, solver=None):
    """Arrays + opts for the members of a per-member reference fixture (tests/golden/knee_members.npz, heldout_members.npz, wide_members.npz:
    members of a C3-distribution draw run one by one through the unmodified reference at rtol=atol=1e-12 by
    tests/golden/make_golden.py) and their reference tables: (problem dict, [table[D, 9 reach columns] per member]).
    The parameter values are regenerated from the recorded seed and checked against what the fixture recorded."""
    from simplyp_amd import synthetic, marshal, abi
    z = np.load(os.path.join(GOLDEN, fname), allow_pickle=False)
    members = [int(m) for m in z['members']]
    years = [str(y) for y in z['years']]
    met_df, p_struc, p_SU, p_LU, p_SC, p, dyn = synthetic.tarland_inputs(years[0], years[1], dynamic_epc0='y', dynamic_erod='n')
    over_all = synthetic.monte_carlo_overrides(p, p_LU, int(z['n_draw']), seed=int(z['seed']))
    if 'wide' in z.files:          # wide_members.npz: the draw's time constants and rates widened (synthetic.widen_overrides)
        over_all = synthetic.widen_overrides(over_all, p, p_LU, int(z['n_draw']), int(z['seed']), float(z['wide']))
    over = {k: v[members] for k, v in over_all.items()}
    for k, nm in enumerate(str(n) for n in z['names']):                # the generator still draws what the fixture recorded
        np.testing.assert_array_equal(over[nm], z['values'][k])
    marshal.prologue(p_SU, p_LU, p_SC, p)
    up_ptr, up_idx, _ = marshal.topology(p_struc, p)
    n = len(members)
    mp = marshal.member_params(p, p_LU, n, over)
    rp = marshal.reach_params(p_SC, p, n)
    forcing, doy = marshal.forcing_arrays(met_df)
    opts = abi.make_opts(solver, dynamic_epc0=True, run_mode_cal=True)
    assert [str(c) for c in z['columns']] == ['Vr', 'Qr_EndOfDay', 'Qr', 'Msus_EndOfDay', 'Msus_kg/day', 'TDPr_EndOfDay',
                                              'TDP_kg/day', 'PPr_EndOfDay', 'PP_kg/day']
    tables = [z['R/%d' % m] for m in members]
    return dict(forcing=forcing, doy=doy, member_params=mp, reach_params=rp, up_ptr=up_ptr, up_idx=up_idx, opts=opts,
                members=members, met=met_df), tables


def dry_fixture_problem(solver=None):
    """Arrays + opts for the ten members of tests/golden/dry_members.npz -- the dry-reach regime: members of two 100 000-member draws
    (one with the time constants widened x/÷ 2) with Qg_min ~ 0 on a climate with 0.6 x Tarland's precipitation and 1/0.6 x its PET,
    each run through the unmodified reference at rtol=atol=1e-12 from 1981-01-01 to a year past its worst day
    (tests/golden/make_golden.py --only dry) -- and what to compare: (problem dict over the days [0, max window end),
    [(lo, hi, table[hi - lo, 9 reach columns]) per member]).  Parameter values are regenerated from the recorded seeds and checked."""
    from simplyp_amd import synthetic, marshal, abi
    z = np.load(os.path.join(GOLDEN, 'dry_members.npz'), allow_pickle=False)
    members = [int(m) for m in z['members']]
    windows = [(int(lo), int(hi)) for lo, hi in z['window']]
    n_days = max(hi for _, hi in windows)
    days = pd.date_range('1981-01-01', periods=n_days)
    met_df, p_struc, p_SU, p_LU, p_SC, p, dyn = synthetic.tarland_inputs('1981-01-01', days[-1].strftime('%Y-%m-%d'), dynamic_epc0='y',
                                                                         dynamic_erod='n')
    names = [str(n) for n in z['names']]
    over = {nm: np.empty(len(members)) for nm in names}
    draws = {}
    for k, (m, dseed, wide) in enumerate(zip(members, z['seed_offset'], z['wide'])):
        key = (int(dseed), float(wide))
        if key not in draws:
            seed = synthetic.C3_SEED + int(dseed)
            o = synthetic.monte_carlo_overrides(p, p_LU, int(z['n_draw']), seed=seed)
            draws[key] = o if wide == 1.0 else synthetic.widen_overrides(o, p, p_LU, int(z['n_draw']), seed, float(wide))
        for nm in names:
            over[nm][k] = draws[key][nm][m]
    for k, nm in enumerate(names):                                     # the generators still draw what the fixture recorded
        np.testing.assert_array_equal(over[nm], z['values'][k])
    marshal.prologue(p_SU, p_LU, p_SC, p)
    up_ptr, up_idx, _ = marshal.topology(p_struc, p)
    n = len(members)
    mp = marshal.member_params(p, p_LU, n, over)
    rp = marshal.reach_params(p_SC, p, n)
    forcing, doy = marshal.forcing_arrays(met_df)
    forcing = forcing.copy()
    forcing[:, 0] *= float(z['pscale'])                                # the hydrological input x 0.6, PET / 0.6 (make_golden.run_reference)
    forcing[:, 1] /= float(z['pscale'])
    opts = abi.make_opts(solver, dynamic_epc0=True, run_mode_cal=True)
    assert [str(c) for c in z['columns']] == ['Vr', 'Qr_EndOfDay', 'Qr', 'Msus_EndOfDay', 'Msus_kg/day', 'TDPr_EndOfDay',
                                              'TDP_kg/day', 'PPr_EndOfDay', 'PP_kg/day']
    tables = [(lo, hi, z['R/%d' % k]) for k, (lo, hi) in enumerate(windows)]
    return dict(forcing=forcing, doy=doy, member_params=mp, reach_params=rp, up_ptr=up_ptr, up_idx=up_idx, opts=opts,
                members=members, met=met_df), tables


def dry_worst_per_member(got, tables, columns):
    """max relative error of every fixture member over its window and the 9 reach columns; got [n_cols, D, 1, E] with `columns`."""
    cols = ['Vr', 'Qr_EndOfDay', 'Qr', 'Msus_EndOfDay', 'Msus_kg/day', 'TDPr_EndOfDay', 'TDP_kg/day', 'PPr_EndOfDay', 'PP_kg/day']
    return [max(max_rel_err(got[columns.index(c), lo:hi, 0, k], tab[:, j], floor=1e-300) for j, c in enumerate(cols))
            for k, (lo, hi, tab) in enumerate(tables)]


def c4_members_problem(solver=None, fname='c4_members.npz'):
    """Arrays + opts for tests/golden/c4_members.npz -- 4 members of BASELINE config C4's own distribution on the upper 16 reaches of
    its chain, 1981, run through the unmodified reference at rtol=atol=1e-12 (tests/golden/make_golden.py --only c4mc) -- and the
    reference tables: (problem dict with all 25 columns of the kept reaches, {(member, position among the kept reaches): table[366, 9]}).
    fname='c4_deep.npz': 2 members on the whole 256-reach chain, reaches 32, 64, 128, 192 and the outlet kept (--only c4deep)."""
    from simplyp_amd import synthetic, marshal
    z = np.load(os.path.join(GOLDEN, fname), allow_pickle=False)
    S, E = int(z['n_reaches']), int(z['n_members'])
    keep = [int(r) for r in z['reaches']]
    pr = synthetic.c4_problem(E, n_reaches=S, n_days=365, solver=solver, out_mask=marshal.MASK_ALL, out_reaches=[r - 1 for r in keep])
    for k, nm in enumerate(str(n) for n in z['names']):                 # the generator still draws what the fixture recorded
        np.testing.assert_array_equal(pr['member_params'][marshal.PM_NAMES.index(nm)], z['values'][k])
    tables = {(m, j): z['R/%d/%d' % (m, r)] for m in range(E) for j, r in enumerate(keep)}
    assert all(t.shape == (365, 9) for t in tables.values())
    return pr, tables


def c4_members_worst(got, tables):
    """max relative error over the 9 reach columns, per (member, kept reach); got [25, 365, n_kept, E]"""
    from simplyp_amd import marshal
    cols = ['Vr', 'Qr_EndOfDay', 'Qr', 'Msus_EndOfDay', 'Msus_kg/day', 'TDPr_EndOfDay', 'TDP_kg/day', 'PPr_EndOfDay', 'PP_kg/day']
    return {key: max(max_rel_err(got[marshal.OUT_COLUMNS.index(c), :, key[1], key[0]], tab[:, j], floor=1e-300) for j, c in enumerate(cols))
            for key, tab in tables.items()}


REACH_COLS = ['Vr', 'Qr_EndOfDay', 'Qr', 'Msus_EndOfDay', 'Msus_kg/day', 'TDPr_EndOfDay', 'TDP_kg/day', 'PPr_EndOfDay', 'PP_kg/day']


def dry_network_inputs(n_draw, n_reaches, st_dt, end_dt, pscale=0.6, solver=None, out_mask=None, out_reaches=None):
    """Config C4's chain (its upper `n_reaches` reaches), every member of an `n_draw`-member draw of C4's distribution (C4_SEED, both
    dynamic options on), Tarland's forcing over [st_dt, end_dt] with the hydrological input x pscale and PET / pscale -- the dry
    network of tests/golden/dry_network.npz and of tools/sweep_dry_network.py.  The run starts at st_dt: initial conditions come from
    the parameters, as in the reference."""
    from simplyp_amd import synthetic, marshal, abi
    met_df, p_struc, p_SU, p_LU, p_SC, p, dyn = synthetic.c4_inputs(n_reaches, synthetic.C4_SEED, st_dt, end_dt)
    marshal.prologue(p_SU, p_LU, p_SC, p)
    up_ptr, up_idx, _ = marshal.topology(p_struc, p)
    over = synthetic.monte_carlo_overrides(p, p_LU, n_draw, synthetic.C4_SEED)
    mp = marshal.member_params(p, p_LU, n_draw, over)
    rp = marshal.reach_params(p_SC, p, n_draw)
    forcing, doy = marshal.forcing_arrays(met_df)
    forcing = forcing.copy()
    forcing[:, 0] *= pscale                                            # as make_golden.run_reference applies `pscale`
    forcing[:, 1] /= pscale
    opts = abi.make_opts(solver, dynamic_epc0=True, dynamic_erod=True, run_mode_cal=True, sc_qr0=int(n_reaches) - 1,
                         out_mask=marshal.MASK_ALL if out_mask is None else out_mask)
    return dict(forcing=forcing, doy=doy, member_params=mp, reach_params=rp, up_ptr=up_ptr, up_idx=up_idx, opts=opts,
                out_reaches=out_reaches, met=met_df)


def dry_network_problem(solver=None):
    """Arrays + opts for tests/golden/dry_network.npz -- members of config C4's draw on the upper reaches of its chain on the dry
    climate (0.6 x precipitation, PET / 0.6), two years, run through the unmodified reference at odeint (1e-12, 1e-15)
    (tests/golden/make_golden.py --only drynet) -- and the reference tables: (problem dict with all 25 columns of the kept reaches and
    only the fixture's members, {(position among the members, position among the kept reaches): table[D, 9]} for the (member, reach)
    pairs the fixture holds -- c4_members_worst compares against it).  The parameter values are regenerated from the recorded seed and
    checked against what the fixture recorded."""
    from simplyp_amd import marshal
    z = np.load(os.path.join(GOLDEN, 'dry_network.npz'), allow_pickle=False)
    members = [int(m) for m in z['members']]
    keep = [int(r) for r in z['reaches']]
    st_dt, end_dt = (str(y) for y in z['years'])
    pr = dry_network_inputs(int(z['n_draw']), int(z['n_reaches']), st_dt, end_dt, float(z['pscale']), solver=solver,
                            out_reaches=[r - 1 for r in keep])
    pr['member_params'] = np.ascontiguousarray(pr['member_params'][:, members])
    pr['reach_params'] = np.ascontiguousarray(pr['reach_params'][:, :, members])
    for k, nm in enumerate(str(n) for n in z['names']):                 # the generator still draws what the fixture recorded
        np.testing.assert_array_equal(pr['member_params'][marshal.PM_NAMES.index(nm)], z['values'][k])
    assert [str(c) for c in z['columns']] == REACH_COLS
    D = pr['forcing'].shape[2]
    tables = {(k, j): z['R/%d/%d' % (m, r)] for k, m in enumerate(members) for j, r in enumerate(keep) if 'R/%d/%d' % (m, r) in z.files}
    assert all(t.shape == (D, 9) for t in tables.values())
    pr['members'], pr['reaches'] = members, keep
    return pr, tables


def branch_network_inputs(n_draw, st_dt, end_dt, members=None, solver=None, out_mask=None, out_reaches=None, snow=False):
    """The branching reach network of simplyp_amd.synthetic.branch_inputs (22 sub-catchments, 13 levels, both dynamic options on) on
    Tarland's forcing over [st_dt, end_dt], with members of an `n_draw`-member draw of config C4's distribution (C4_SEED): all of them,
    or `members` -- positions in the draw, -1 for the workbook's own values -- in that order.  The network of
    tests/golden/branch_network.npz and of tools/sweep_dry_network.py --network branch.  snow=True: the raw met rows and the snow
    module in the kernel (opts.snow = 1), as marshal_scenario."""
    from simplyp_amd import synthetic, marshal, abi
    met_df, p_struc, p_SU, p_LU, p_SC, p, dyn = synthetic.branch_inputs(synthetic.BRANCH_SEED, st_dt, end_dt)
    marshal.prologue(p_SU, p_LU, p_SC, p)
    up_ptr, up_idx, _ = marshal.topology(p_struc, p)
    over = synthetic.monte_carlo_overrides(p, p_LU, n_draw, synthetic.C4_SEED)
    if members is not None:
        base = marshal.member_params(p, p_LU, 1)[:, 0]
        over = {nm: np.array([base[marshal.PM_NAMES.index(nm)] if m < 0 else v[m] for m in members]) for nm, v in over.items()}
    E = n_draw if members is None else len(members)
    mp = marshal.member_params(p, p_LU, E, over)
    rp = marshal.reach_params(p_SC, p, E)
    forcing, doy = marshal.forcing_arrays(met_df, snow=snow)
    opts = abi.make_opts(solver, dynamic_epc0=True, dynamic_erod=True, run_mode_cal=True, sc_qr0=len(marshal.sc_list(p)) - 1,
                         out_mask=marshal.MASK_ALL if out_mask is None else out_mask, snow=snow)
    return dict(forcing=forcing, doy=doy, member_params=mp, reach_params=rp, up_ptr=up_ptr, up_idx=up_idx, opts=opts,
                out_reaches=out_reaches, met=met_df)


def network_levels(up_ptr, up_idx):
    """(level[S] = longest path from a headwater, max_jump = the largest level difference between a reach and a reach directly upstream
    of it) of a reach graph in CSR form -- what the library's derive_topology computes to size the task queue's ring buffers
    (min(n_chunks, max_jump + 1) time chunks) and to cut the load balancer's pilot (PILOT_LEVELS)."""
    S = len(up_ptr) - 1
    level = [0] * S
    for s in range(S):
        for k in range(up_ptr[s], up_ptr[s + 1]):
            level[s] = max(level[s], level[up_idx[k]] + 1)
    jump = max([level[s] - level[up_idx[k]] for s in range(S) for k in range(up_ptr[s], up_ptr[s + 1])] or [0])
    return level, jump


def branch_network_problem(solver=None):
    """Arrays + opts for tests/golden/branch_network.npz -- the workbook member and three members of a 64-member draw of config C4's
    distribution on the branching network of synthetic.branch_inputs, 1981-1982, run through the unmodified reference at odeint
    rtol = atol = 1e-12 (tests/golden/make_golden.py --only branch) -- and the reference tables: (problem dict with all 25 columns of
    the kept reaches and the fixture's members, {(position among the members, position among the kept reaches): table[D, 9]} for the
    (member, reach) pairs the fixture holds -- c4_members_worst compares against it).  The parameter values are regenerated from the recorded seed and checked against what the
    fixture recorded, and so is the topology."""
    from simplyp_amd import marshal
    z = np.load(os.path.join(GOLDEN, 'branch_network.npz'), allow_pickle=False)
    members = [int(m) for m in z['members']]
    keep = [int(r) for r in z['reaches']]
    st_dt, end_dt = (str(y) for y in z['years'])
    pr = branch_network_inputs(int(z['n_draw']), st_dt, end_dt, members=members, solver=solver, out_reaches=[r - 1 for r in keep])
    for k, nm in enumerate(str(n) for n in z['names']):                 # the generator still draws what the fixture recorded
        np.testing.assert_array_equal(pr['member_params'][marshal.PM_NAMES.index(nm)], z['values'][k])
    np.testing.assert_array_equal(pr['up_ptr'], z['up_ptr'])
    np.testing.assert_array_equal(pr['up_idx'], z['up_idx'])
    assert [str(c) for c in z['columns']] == REACH_COLS
    D = pr['forcing'].shape[2]
    tables = {(k, j): z['R/%d/%d' % (m, r)] for k, m in enumerate(members) for j, r in enumerate(keep) if 'R/%d/%d' % (m, r) in z.files}
    assert all(t.shape == (D, 9) for t in tables.values())
    pr['members'], pr['reaches'] = members, keep
    return pr, tables


def random_network_problem(seed, E=40):
    """A random upstream graph: 12 reaches, 0-2 upstream reaches each, a reach may feed several downstream reaches; every reach one of
    confluence3_nc_2004's three (newly-converted land of either kind, or none) with its own area, length, slope and TDPeff (blank on
    about a third); `E` members with fc, T_g, a_Q and E_M perturbed.  One year, both dynamic options on; opts: the default solver."""
    from simplyp_amd import marshal, abi
    rng = np.random.default_rng(100 + seed)
    S = 12
    base = marshal_scenario('confluence3_nc_2004', E=E)
    rp0 = base['reach_params']                                   # [NP_R, 3, E]
    rp = np.empty((marshal.NP_R, S, E))
    for s in range(S):
        rp[:, s, :] = rp0[:, rng.integers(0, 3), :]
    ix = marshal.PR_NAMES.index
    rp[ix('A_catch')] = rng.uniform(5.0, 60.0, (S, 1))
    rp[ix('L_reach')] = rng.uniform(2000.0, 12000.0, (S, 1))
    rp[ix('S_reach')] = rng.uniform(0.3, 2.5, (S, 1))
    rp[ix('TDPeff')] = np.where(rng.random((S, 1)) < 0.3, np.nan, rng.uniform(0.0, 0.4, (S, 1)))
    up_ptr, up_idx = [0], []
    for s in range(S):
        k = 0 if s == 0 else int(rng.integers(0, 3))
        ups = sorted(rng.choice(s, size=min(k, s), replace=False).tolist()) if k else []
        up_idx += ups
        up_ptr.append(len(up_idx))
    mp = base['member_params'].copy()
    for pname, lo, hi in (('fc', 0.9, 1.1), ('T_g', 0.7, 1.4), ('a_Q', 0.7, 1.5), ('E_M', 0.5, 2.0)):
        mp[marshal.PM_NAMES.index(pname)] *= rng.uniform(lo, hi, E)
    opts = abi.make_opts(None, dynamic_epc0=True, dynamic_erod=True, run_mode_cal=True, sc_qr0=S - 1, out_mask=marshal.MASK_ALL)
    return dict(base, member_params=mp, reach_params=rp, up_ptr=np.asarray(up_ptr, dtype=np.int32), up_idx=np.asarray(up_idx, dtype=np.int32),
                opts=opts)


BUDGET_SCENARIOS = ['tarland_2004_dynamic', 'tarland_2004_dynamic+snow', 'chain4_val_2004', 'confluence3_nc_2004', 'stiff_chain12_2004',
                    'branch', 'random1', 'random2', 'random3',
                    'net5_static_2004', 'net5_static_erod_val_2004', 'net5_dynamic_leakA_2004', 'net5_dynamic_leaknone_2004']


def budget_problem(name, E, solver=None, step_len=1.0, closable=True, seed=7):
    """Arrays + opts of a scenario of BUDGET_SCENARIOS for the budgets of tests/budgets.py: a golden scenario ('+snow': the snow module
    in the kernel, with f_DDSM and D_snow_0 perturbed and the D_snow column in the table), the branching network ('branch', 1981,
    members of config C4's draw) or a random 12-reach graph ('randomN' = random_network_problem(N)), all 25 columns.  closable: alpha = 0
    and k_M = 1 for every member, and fc, T_g, a_Q, b_Q, beta, f_quick, E_M, T_s_A, T_s_S, Qg_min perturbed per member (member 0 keeps
    the scenario's values); else the members as the scenario has them.  m['columns'] names the table's columns."""
    from simplyp_amd import marshal, abi
    snow = name.endswith('+snow')
    if name == 'branch':
        m = branch_network_inputs(max(E, 2), '1981-01-01', '1981-12-31', members=[-1] + list(range(E - 1)), solver=solver)
    elif name.startswith('random'):
        m = random_network_problem(int(name[len('random'):]), E)
        o = abi.make_opts(solver, dynamic_epc0=True, dynamic_erod=True, run_mode_cal=True, sc_qr0=m['opts'].sc_qr0, out_mask=marshal.MASK_ALL)
        m['opts'] = o
    else:
        m = marshal_scenario(name.split('+')[0], E=E, solver=solver, snow=snow)
    m['opts'].step_len = float(step_len)
    m['columns'] = list(marshal.OUT_COLUMNS)
    mp = np.array(m['member_params'], dtype=np.float64)
    rng = np.random.default_rng(seed)
    if snow:
        m['opts'].out_mask = marshal.MASK_ALL | marshal.MASK_D_SNOW
        m['columns'] = list(marshal.ALL_COLUMNS)
        mp[marshal.PM_NAMES.index('f_DDSM'), 1:] *= rng.uniform(0.5, 2.0, E - 1)
        mp[marshal.PM_NAMES.index('D_snow_0'), 1:] = rng.uniform(0.0, 30.0, E - 1)
    if closable:
        mp[marshal.PM_NAMES.index('alpha')] = 0.0
        mp[marshal.PM_NAMES.index('k_M')] = 1.0
        for pname, lo, hi, cap in (('fc', 0.85, 1.15, None), ('T_g', 0.6, 1.6, None), ('a_Q', 0.6, 1.6, None), ('b_Q', 0.9, 1.1, 0.95),
                                   ('beta', 0.8, 1.2, 0.95), ('f_quick', 0.3, 3.0, 0.5), ('E_M', 0.5, 2.0, None), ('T_s_A', 0.5, 2.0, None),
                                   ('T_s_S', 0.5, 2.0, None), ('Qg_min', 0.2, 3.0, None)):
            row = mp[marshal.PM_NAMES.index(pname)]
            row[1:] *= rng.uniform(lo, hi, E - 1)
            if cap is not None:
                np.minimum(row, cap, out=row)
    m['member_params'] = np.ascontiguousarray(mp)
    m.setdefault('out_reaches', None)
    return m


def steplen_cases():
    """[(scenario name, step_len)] of tests/golden/step_len.npz (tests/golden/make_golden.py --only steplen)."""
    z = np.load(os.path.join(GOLDEN, 'step_len.npz'), allow_pickle=False)
    return [(str(n), float(s)) for n, s in zip(z['names'], z['step_len'])]


def steplen_problem(case, E=1, solver=None):
    """Arrays + opts of case `case` of tests/golden/step_len.npz -- a golden scenario (marshal_scenario) run by the unmodified reference
    with run_simply_p(..., step_len=s) at rtol = atol = 1e-12 -- and its tables: (problem dict with opts.step_len = s,
    {SC: {column: series}} with the 9 reach columns of every reach and, where stored, the terrestrial columns)."""
    z = np.load(os.path.join(GOLDEN, 'step_len.npz'), allow_pickle=False)
    name, step_len = str(z['names'][case]), float(z['step_len'][case])
    m = marshal_scenario(name, E=E, solver=solver)
    m['opts'].step_len = step_len
    tables = {}
    for sc in m['scs']:
        t = dict(zip(REACH_COLS, z['R/%d/%d' % (case, sc)].T))
        if 'TC/%d/%d' % (case, sc) in z.files:
            t.update(zip((str(c) for c in z['TC/%d/%d/columns' % (case, sc)]), z['TC/%d/%d' % (case, sc)].T))
        tables[sc] = t
    m['name'], m['step_len'] = name, step_len
    return m, tables


def steplen_errors(out, scs, tables, columns, member=0):
    """{column: max relative error over the reaches} of out[n_cols, D, S, E] (columns = `columns`) against steplen_problem's tables,
    over every column the fixture holds."""
    errs = {}
    for j, sc in enumerate(scs):
        for c, ref in tables[sc].items():
            errs[c] = max(errs.get(c, 0.0), max_rel_err(out[columns.index(c), :, j, member], ref, floor=1e-300))
    return errs
