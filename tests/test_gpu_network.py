"""The network paths of the HIP engine that only a deep, branching reach graph reaches: the task-queue kernel's ring buffers of the
routing series when they wrap across a level jump (a reach reads an upstream reach several levels above it, and a ring holds
min(n_chunks, max_jump + 1) time chunks, so a row is overwritten while a reader further down may still need it), a reach read at two
different lags (fan-out), the load balancer's pilot cut at PILOT_LEVELS on a branching schedule, and the other options of a run
(four lanes per member, slot order, selected reaches, streamed output, per-period sums, the snow module) on such a graph.

Each test first asserts, from up_ptr / up_idx and the run's stats, that it reaches the path it is named for.  The reference-made
tables of the branching network are tests/golden/branch_network.npz (tests/golden/make_golden.py --only branch)."""

import numpy as np
import pytest

import helpers
from simplyp_amd import abi, engine, marshal

pytestmark = pytest.mark.gpu

PILOT_LEVELS = 8                    # simplyp_hip.hip: the load balancer's pilot runs the reaches above this level
FLOOR = 1e-12
YEARS = ('1981-01-01', '1982-12-31')


def gpu_run(eng, m, **kw):
    out, status, stats = eng.run(m['forcing'], m['doy'], m['member_params'], m['reach_params'], m['up_ptr'], m['up_idx'], m['opts'], **kw)
    return out.cpu().numpy(), status.cpu().numpy(), stats


def cpu_run(oracle_lib, m, **kw):
    return oracle_lib.run(m['forcing'], m['doy'], m['member_params'], m['reach_params'], m['up_ptr'], m['up_idx'], m['opts'], **kw)


def n_chunks(D, chunk_days):
    return -(-D // chunk_days)


def ring_wraps(m, chunk_days):
    """Does a run of m in chunks of `chunk_days` overwrite rows of its routing rings (min(n_chunks, max_jump + 1) < n_chunks)?"""
    _, jump = helpers.network_levels(m['up_ptr'], m['up_idx'])
    nc = n_chunks(m['forcing'].shape[2], chunk_days)
    return min(nc, jump + 1) < nc


def depth(m):
    return max(helpers.network_levels(m['up_ptr'], m['up_idx'])[0]) + 1


# ---- 1. the kernel against the reference on the branching network -----------------------------------------------------------

@pytest.mark.parametrize('lanes', [1, 4])
def test_kernel_on_the_branching_network_against_the_reference(engine0, oracle_lib, lanes):
    """tests/golden/branch_network.npz (the workbook member and three of C4's draw on synthetic.branch_inputs' 22-reach network,
    1981-1982, the unmodified reference at odeint rtol = atol = 1e-12), default solver, one and four lanes per member: the automatic
    kernel (at this size the task queue, 256-day chunks), the queue at 64-day chunks (the rings wrap) and the chain kernel meet
    north_star's bar on every kept value, are bit for bit the same run, and are within 10 x rtol of the oracle's run of the same
    scheme.  stiff_pair = -1 (Cash-Karp alone, the conservative switch) meets the bar too."""
    pr, tables = helpers.branch_network_problem(solver=dict(lanes_per_member=lanes))
    D = pr['forcing'].shape[2]
    assert depth(pr) > PILOT_LEVELS and ring_wraps(pr, 64) and not ring_wraps(pr, 256)
    auto, sa, st_a = gpu_run(engine0, pr, out_reaches=pr['out_reaches'])
    assert st_a['queued'] == 1 and st_a['lanes_per_member'] == lanes and st_a['stiff_pair'] == 1 and sa.max() == 0
    runs = {'auto': (auto, sa, st_a)}
    for key, chunk in (('queue64', 64), ('chain', -1)):
        pr['opts'].time_chunk_days = chunk
        runs[key] = gpu_run(engine0, pr, out_reaches=pr['out_reaches'])
        assert runs[key][2]['queued'] == (chunk > 0) and runs[key][2]['lanes_per_member'] == lanes and runs[key][2]['stiff_pair'] == 1
    assert n_chunks(D, 64) == 12
    for key, (got, status, stats) in runs.items():
        worst = helpers.c4_members_worst(got, tables)
        assert max(worst.values()) < 1e-6, (key, worst)
        assert np.array_equal(got, auto) and np.array_equal(status, sa) and stats['rhs_evals'] == st_a['rhs_evals'], key
    pr['opts'].time_chunk_days = 0
    ref, rs, _ = cpu_run(oracle_lib, pr, out_reaches=pr['out_reaches'], n_threads=4)
    assert rs.max() == 0 and helpers.max_rel_err(auto, ref, floor=FLOOR) < helpers.TOL_WORKING
    pr['opts'].stiff_pair = -1
    off, so, st_o = gpu_run(engine0, pr, out_reaches=pr['out_reaches'])
    assert st_o['stiff_pair'] == 0 and st_o['queued'] == 1 and so.max() == 0
    worst = helpers.c4_members_worst(off, tables)
    assert max(worst.values()) < 1e-6, worst


# ---- 2. every kernel path on the branching network is the same run --------------------------------------------------------

def test_every_kernel_path_on_the_branching_network_is_the_same_run(engine0):
    """150 members of C4's draw on the fixture's network over 1981-1982, one of them NaN-poisoned.  The baseline is the chain kernel, one
    lane per member, no balancing.  Bit for bit the same outputs, status words and per-member right-hand sides from: the queue at
    256-day chunks; the queue at 64-day chunks (12 chunks: the rings of max_jump + 1 = 10 chunks wrap); balance = 1 on both kernels (a
    pilot cut at PILOT_LEVELS on a schedule 13 levels deep); four lanes per member on both kernels; slot order mapped back; selected
    reaches; a streamed host table (equal to the device table).  Annual rows equal the host's sums of the daily rows."""
    import torch
    E, poisoned = 150, 77
    mask = marshal.mask_of_columns(helpers.REACH_COLS)
    base = helpers.branch_network_inputs(E, *YEARS, solver=dict(time_chunk_days=-1, balance=0, lanes_per_member=1), out_mask=mask)
    base['member_params'][marshal.PM_NAMES.index('T_s_S'), poisoned] = np.nan
    D, S = base['forcing'].shape[2], base['reach_params'].shape[1]
    assert depth(base) > PILOT_LEVELS and ring_wraps(base, 64) and not ring_wraps(base, 256) and n_chunks(D, 64) == 12
    w0 = torch.zeros(E, dtype=torch.int32, device='cuda')
    ref, sref, st0 = gpu_run(engine0, base, member_rhs=w0)
    assert st0['queued'] == 0 and st0['balanced'] == 0 and st0['lanes_per_member'] == 1 and st0['stiff_pair'] == 1
    assert sref[poisoned] & abi.STATUS_NONFINITE and (np.delete(sref, poisoned) == 0).all()

    def variant(**solver):
        return dict(base, opts=abi.make_opts(dict(dict(time_chunk_days=-1, balance=0, lanes_per_member=1), **solver), dynamic_epc0=True,
                                             dynamic_erod=True, run_mode_cal=True, sc_qr0=S - 1, out_mask=mask))

    def same(m, want, **kw):
        w = torch.zeros(E, dtype=torch.int32, device='cuda')
        got, status, st = gpu_run(engine0, m, member_rhs=w, **kw)
        for k, v in want.items():
            assert st[k] == v, (k, st[k], want)
        if m['opts'].out_slot_order:
            mos = st['member_of_slot'].cpu().numpy()
            assert sorted(mos) == list(range(E)) and not np.array_equal(mos, np.arange(E))
            unslot = np.empty_like(got)
            unslot[..., mos] = got
            got = unslot
        assert np.array_equal(got, ref, equal_nan=True), want
        assert np.array_equal(status, sref) and bool(torch.equal(w, w0)) and st['rhs_evals'] == st0['rhs_evals'], want
        return st

    same(variant(time_chunk_days=256), dict(queued=1, balanced=0))
    same(variant(time_chunk_days=64), dict(queued=1, balanced=0))
    same(variant(balance=1), dict(queued=0, balanced=1))
    same(variant(balance=1, time_chunk_days=64), dict(queued=1, balanced=1))
    same(variant(lanes_per_member=4), dict(queued=0, lanes_per_member=4))
    same(variant(lanes_per_member=4, time_chunk_days=64), dict(queued=1, lanes_per_member=4))
    same(variant(balance=1, out_slot_order=1, time_chunk_days=64), dict(queued=1, balanced=1))
    # selected reaches: the tributaries' ends, the confluence, where C and the lone headwater join, the outlet
    sel = [6, 11, 12, 16, 18, 21]
    m = variant(time_chunk_days=64)
    got, status, st = gpu_run(engine0, m, out_reaches=sel)
    assert st['queued'] == 1 and np.array_equal(got, ref[:, :, sel], equal_nan=True) and np.array_equal(status, sref)
    # a streamed host table: the queue in time chunks (auto: 256 days for a network; and 64 days, where the first of 12 chunks is
    # complete at all 13 levels long before the last one: its copy must have started while the kernel ran)
    host = engine.pinned_empty(tuple(ref.shape))
    for chunk in (0, 64):
        m = variant(time_chunk_days=chunk)
        host[...] = -7.0
        out, status, st = engine0.run(m['forcing'], m['doy'], m['member_params'], m['reach_params'], m['up_ptr'], m['up_idx'], m['opts'],
                                      host_out=host)
        nc = n_chunks(D, chunk or 256)
        assert st['queued'] == 1 and (1 if chunk else 0) <= st['streamed_chunks'] <= nc, (chunk, st['streamed_chunks'])
        assert np.array_equal(host, out.cpu().numpy(), equal_nan=True) and np.array_equal(host, ref, equal_nan=True)
        assert np.array_equal(status.cpu().numpy(), sref)
    # annual rows (opts.n_periods): the kernel's per-period sums against the host's sums of the daily rows, both kernels
    years = np.asarray(base['met'].index.year)
    uy = np.unique(years)
    pod = np.searchsorted(uy, years).astype(np.int32)
    ok = np.delete(np.arange(E), poisoned)
    want = np.stack([ref[:, years == y].sum(axis=1) for y in uy], axis=1)
    for chunk in (-1, 64):
        m = variant(time_chunk_days=chunk)
        m['opts'].n_periods = len(uy)
        red, status, st = gpu_run(engine0, m, period_of_day=pod)
        assert st['queued'] == (chunk > 0) and red.shape == (9, len(uy), S, E) and np.array_equal(status, sref)
        np.testing.assert_allclose(red[..., ok], want[..., ok], rtol=1e-12)


# ---- 3. level jumps and fan-out in the queue, on small graphs -----------------------------------------------------------------

def graph(ups):
    """CSR (up_ptr, up_idx) of a reach graph given as each reach's list of directly-upstream reaches (zero-based, ids ascending
    downstream)."""
    up_ptr, up_idx = [0], []
    for s, u in enumerate(ups):
        assert all(0 <= x < s for x in u)
        up_idx += sorted(u)
        up_ptr.append(len(up_idx))
    return np.asarray(up_ptr, dtype=np.int32), np.asarray(up_idx, dtype=np.int32)


def stem_with_side_headwaters():
    """A stem of 11 reaches; side headwaters (2, 6, 11) join it at levels 2, 5 and 9."""
    return graph([[], [0], [], [1, 2], [3], [4], [], [5, 6], [7], [8], [9], [], [10, 11], [12]])


def fan_out():
    """Headwater 0 is read by reach 1 (level 1) and by reach 8 (level 6): one ring row, two readers at different lags."""
    return graph([[], [0], [], [2], [3], [4], [5], [6], [7, 0], [8, 1]])


def random_dag(seed, S=40):
    """A random tree of S reaches (ids ascending downstream): each reach is a headwater or drains 1-2 of the reaches before it that
    nothing drains yet, picked among the 8 most recent; the first three reaches are headwaters kept out of that pool and forced into reaches at levels
    6-10 further down (long jumps)."""
    rng = np.random.default_rng(seed)
    ups, pool = [[], [], []], []
    for s in range(3, S):
        k = min(len(pool), int(rng.choice(3, p=(0.3, 0.35, 0.35))))
        pick = sorted(rng.choice(pool[-8:], size=k, replace=False).tolist()) if k else []
        pool = [r for r in pool if r not in pick] + [s]
        ups.append(pick)
    level, _ = helpers.network_levels(*graph(ups))
    deep = [s for s in range(S) if 6 <= level[s] <= 10]
    for h, s in zip(range(3), rng.choice(deep, size=3, replace=False)):
        ups[int(s)] = sorted(set(ups[int(s)]) | {h})
    return graph(ups)


TOPOLOGIES = {'stem': stem_with_side_headwaters, 'fan_out': fan_out,
              'random1': lambda: random_dag(1), 'random2': lambda: random_dag(2), 'random3': lambda: random_dag(3)}


def topology_problem(up_ptr, up_idx, E=16, seed=7, years=4):
    """confluence3_nc_2004's reaches spread over the graph with varied areas / lengths / slopes (at least 20 km2 of their own, so that
    no reach is stiffer than RK4 at 128 substeps can take) and newly-converted land, 2004's forcing tiled `years` times, E perturbed
    members."""
    rng = np.random.default_rng(seed)
    S = len(up_ptr) - 1
    base = helpers.marshal_scenario('confluence3_nc_2004', E=E)
    rp0 = base['reach_params']
    rp = np.empty((marshal.NP_R, S, E))
    for s in range(S):
        rp[:, s, :] = rp0[:, rng.integers(0, 3), :]
    ix = marshal.PR_NAMES.index
    rp[ix('A_catch')] = rng.uniform(20.0, 60.0, (S, 1))
    rp[ix('L_reach')] = rng.uniform(2000.0, 12000.0, (S, 1))
    rp[ix('S_reach')] = rng.uniform(0.3, 2.5, (S, 1))
    mp = base['member_params'].copy()
    for pname, lo, hi in (('fc', 0.9, 1.1), ('T_g', 0.7, 1.4), ('a_Q', 0.7, 1.5), ('E_M', 0.5, 2.0)):
        mp[marshal.PM_NAMES.index(pname)] *= rng.uniform(lo, hi, E)
    forcing = np.ascontiguousarray(np.tile(base['forcing'], (1, 1, years)))
    doy = np.ascontiguousarray(np.tile(base['doy'], years))
    return dict(base, forcing=forcing, doy=doy, member_params=mp, reach_params=np.ascontiguousarray(rp), up_ptr=up_ptr, up_idx=up_idx)


@pytest.mark.parametrize('name', list(TOPOLOGIES))
def test_level_jumps_and_fan_out_in_the_queue(engine0, oracle_lib, name):
    """Small graphs built for the paths: a stem with side headwaters joining at levels 2, 5 and 9; a headwater read by reaches at levels
    1 and 6; random trees of 40 reaches with headwaters forced into reaches 6-10 levels down (their own jumps reach 15-21 levels).
    Four years (1464 days), so that the rings wrap at 64-day chunks (23), and at 128-day chunks (12) on the two small graphs.  RK4 (chain kernel only) within 1e-9 of the oracle; the default
    solver within 10 x rtol of the oracle on the chain kernel, and the queue at 64, 128 and 256 days bit for bit the chain kernel."""
    up_ptr, up_idx = TOPOLOGIES[name]()
    m = topology_problem(up_ptr, up_idx)
    S, D = len(up_ptr) - 1, m['forcing'].shape[2]
    level, jump = helpers.network_levels(up_ptr, up_idx)
    assert jump >= 6 and ring_wraps(m, 64), (name, jump)
    assert ring_wraps(m, 128) == (name in ('stem', 'fan_out')), (name, jump)        # the random trees' jumps are 15-21 levels
    n_down = np.bincount(up_idx, minlength=S)
    if name == 'fan_out':
        assert n_down[0] == 2 and level[1] == 1 and level[8] == 6
    if name == 'stem':
        assert sorted(level[s] for s in range(S) if up_ptr[s + 1] - up_ptr[s] == 2) == [2, 5, 9]
    opts = lambda solver: abi.make_opts(solver, dynamic_epc0=True, dynamic_erod=True, run_mode_cal=True, sc_qr0=S - 1,
                                        out_mask=marshal.MASK_ALL)
    m['opts'] = opts(dict(integrator='rk4', substeps=128))
    ref, rs, _ = cpu_run(oracle_lib, m, n_threads=8)
    got, gs, st = gpu_run(engine0, m)
    assert st['queued'] == 0 and rs.max() == 0 and gs.max() == 0
    assert helpers.max_rel_err(got, ref, floor=FLOOR) < 1e-9, name
    m['opts'] = opts(dict(time_chunk_days=-1, balance=0))
    ref, rs, _ = cpu_run(oracle_lib, m, n_threads=8)
    chain, cs, cst = gpu_run(engine0, m)
    assert cst['queued'] == 0 and cst['stiff_pair'] == 1 and rs.max() == 0 and cs.max() == 0
    assert helpers.max_rel_err(chain, ref, floor=FLOOR) < helpers.TOL_WORKING, name
    for chunk in (64, 128, 256):
        m['opts'].time_chunk_days = chunk
        queue, qs, qst = gpu_run(engine0, m)
        assert qst['queued'] == 1, (name, chunk)
        assert np.array_equal(queue, chain) and np.array_equal(qs, cs) and qst['rhs_evals'] == cst['rhs_evals'], (name, chunk)


# ---- 4. the snow module on the branching network --------------------------------------------------------------------------

def test_snow_in_kernel_on_the_branching_network(engine0):
    """opts.snow = 1 (each member's own degree-day snow module in the kernel) on the fixture's network through the task queue at 64-day
    chunks (the rings wrap) with four lanes per member: bit for bit the run fed the host snow function's P series per member."""
    from test_snow_in_kernel import per_member_forcing, snow_members
    import torch
    E = 40
    solver = dict(time_chunk_days=64, lanes_per_member=4)
    m1 = helpers.branch_network_inputs(E, *YEARS, solver=solver, out_mask=marshal.MASK_REACH5, snow=True)
    m0 = helpers.branch_network_inputs(E, *YEARS, solver=solver, out_mask=marshal.MASK_REACH5)
    assert ring_wraps(m1, 64)
    f_ddsm, d0 = snow_members(E)
    m1['member_params'][marshal.PM_NAMES.index('f_DDSM')] = f_ddsm
    m1['member_params'][marshal.PM_NAMES.index('D_snow_0')] = d0
    m0['forcing'] = per_member_forcing(m0['met'], f_ddsm, d0)
    a, sa, st1 = engine0.run(m1['forcing'], m1['doy'], m1['member_params'], m1['reach_params'], m1['up_ptr'], m1['up_idx'], m1['opts'])
    b, sb, st0 = engine0.run(m0['forcing'], m0['doy'], m0['member_params'], m0['reach_params'], m0['up_ptr'], m0['up_idx'], m0['opts'],
                             forcing_of_member=np.arange(E, dtype=np.int32))
    for st in (st0, st1):
        assert st['queued'] == 1 and st['lanes_per_member'] == 4 and st['stiff_pair'] == 1
    assert bool(torch.equal(a, b)) and bool(torch.equal(sa, sb)) and int(sa.max()) == 0 and bool(torch.isfinite(a).all())
    assert not bool(torch.equal(a[..., 0], a[..., 1]))          # the snow parameters matter
