"""NSGA-II on the device (simplyp_nsga2_init / _crowding / _select / _offspring, include/simplyp_nsga2.h) against its NumPy
statement (simplyp_amd/nsga2.py), and find_pareto end to end.

Crowding, positions and survivors are selections and integer counts; the variation is + - * / sqrt and comparisons in fp64 in one
order on both sides (the library is built without contraction): everything is compared bit for bit or as integers, with no
margin.  The one bound is the public call's objectives against an independent ensemble run at the same points:
1e-9 max(1, |want|), the project's device-gof bar (same kernels, independent members; the goodness-of-fit sums may be chunked
differently for a different ensemble size)."""

import ctypes as C

import numpy as np
import pytest
import torch

import helpers
import nsga2_cases as nc
import simplyp_amd as sp
from simplyp_amd import abi, engine, marshal, nsga2, pareto

pytestmark = pytest.mark.gpu

SHAPES = [(4, 1, 1), (64, 3, 2), (130, 5, 3), (514, 16, 8)]      # a partial wave, a full one, a second block of pairs; both ends of n_dim and M
NAME = 'tarland_2004_dynamic'
SENTINEL = -777.25


def dev(eng, a, dtype=torch.float64):
    return eng.to_device(np.ascontiguousarray(a), dtype)


def box(n_dim):
    lo = -1.0 - np.arange(n_dim) * 0.125
    hi = 1.5 + np.arange(n_dim) * 0.25
    target = np.array([2, abi.MCMC_TARGET_F_TDP, abi.MCMC_TARGET_NONE] + list(range(5, 5 + n_dim)), dtype=np.int32)[:n_dim]
    return lo, hi, target


def scattered(mp, ft, theta, target, what):
    """The run's arrays hold theta's rows where target says so and the sentinel everywhere else."""
    mp, ft = mp.cpu().numpy(), ft.cpu().numpy()
    rows = set()
    for d, tg in enumerate(target):
        if tg >= 0:
            nc.same_bits(mp[tg], theta[d], (what, 'member_params', d))
            rows.add(int(tg))
        elif tg == abi.MCMC_TARGET_F_TDP:
            nc.same_bits(ft, theta[d], (what, 'f_tdp'))
    assert (np.delete(mp, sorted(rows), axis=0) == SENTINEL).all(), what
    if abi.MCMC_TARGET_F_TDP not in list(target):
        assert (ft == SENTINEL).all(), what


# ---- the four entries against the mirror --------------------------------------------------------------------------------------

@pytest.mark.parametrize('N, n_dim, M', SHAPES)
def test_init_and_offspring_match_the_mirror_bit_for_bit(engine0, N, n_dim, M):
    f64 = dict(dtype=torch.float64, device=engine0.tdev)
    lo, hi, target = box(n_dim)
    rng = np.random.default_rng(100 * N + n_dim)
    for seed in (0, (1 << 64) - 3):
        theta = torch.full((n_dim, N), SENTINEL, **f64)
        mp, ft = torch.full((marshal.NP_M, N), SENTINEL, **f64), torch.full((N,), SENTINEL, **f64)
        info = engine0.nsga2_init(theta, lo, hi, target, mp, ft, seed=seed)
        want = nsga2.initial_population(N, lo, hi, seed)
        nc.same_bits(theta.cpu().numpy(), want, 'init')
        scattered(mp, ft, want, target, 'init')
        assert info['n_inside'] == N and info['n_accepted'] == 0 and info['n_nan'] == 0 and info['kernel_ms'] > 0.0
        assert ((want >= lo[:, None]) & (want <= hi[:, None])).all()
    # parents on the box's faces, equal to each other, and anywhere; ranks with ties and invalid members; crowding with ties and inf
    parents = want.copy()
    parents[:, rng.integers(0, N, max(1, N // 8))] = lo[:, None]
    parents[:, rng.integers(0, N, max(1, N // 8))] = hi[:, None]
    parents[:, N // 2:N // 2 + max(1, N // 8)] = parents[:, :max(1, N // 8)]
    rank = rng.integers(-1, 3, N).astype(np.int32)
    crowd = np.where(rank < 0, 0.0, rng.choice([0.0, 0.25, 0.25, 1.5, np.inf], N))
    theta_d, rank_d, crowd_d = dev(engine0, parents), dev(engine0, rank, torch.int32), dev(engine0, crowd)
    settings = [dict(t=1), dict(t=(1 << 32) - 1, eta_c=1, eta_m=31, p_cross=1.0, p_mut=1.0), dict(t=7, eta_c=31, eta_m=1, p_cross=0.5, p_mut=0.3),
                dict(t=2, eta_c=3, eta_m=7, p_cross=0.0, p_mut=0.0), dict(t=3, eta_c=7, eta_m=3, p_cross=1.0, p_mut=0.0)]
    for kw in settings:
        child = torch.full((n_dim, N), SENTINEL, **f64)
        par = torch.full((2, N), -9, dtype=torch.int32, device=engine0.tdev)
        mp, ft = torch.full((marshal.NP_M, N), SENTINEL, **f64), torch.full((N,), SENTINEL, **f64)
        want = nsga2.offspring(parents, rank, crowd, kw['t'], lo, hi, kw.get('eta_c', 15), kw.get('eta_m', 15), kw.get('p_cross', 0.9),
                               kw.get('p_mut'), seed=5)
        info = engine0.nsga2_offspring(theta_d, rank_d, crowd_d, kw['t'], lo, hi, target, child, parents=par, member_params=mp, f_tdp=ft,
                                       k_c=nsga2.k_of_eta(kw.get('eta_c', 15)), k_m=nsga2.k_of_eta(kw.get('eta_m', 15)),
                                       p_cross=kw.get('p_cross', 0.9), p_mut=kw.get('p_mut'), seed=5)
        nc.same_bits(child.cpu().numpy(), want['child'], ('child', kw))
        assert np.array_equal(par.cpu().numpy(), want['parents']), kw
        scattered(mp, ft, want['child'], target, ('offspring', kw))
        assert info['n_inside'] == N and info['n_accepted'] == int(want['crossed'].sum()) and info['n_nan'] == 0
        assert ((want['child'] >= lo[:, None]) & (want['child'] <= hi[:, None])).all()
        if kw.get('p_cross') == 0.0 and kw.get('p_mut') == 0.0:
            assert np.array_equal(want['child'][:, :N // 2], parents[:, want['parents'][0, :N // 2]])
    assert torch.equal(theta_d, dev(engine0, parents))                       # the parents are read only
    # without the optional outputs
    child = torch.full((n_dim, N), SENTINEL, **f64)
    engine0.nsga2_offspring(theta_d, rank_d, crowd_d, 1, lo, hi, np.full(n_dim, abi.MCMC_TARGET_NONE), child, seed=5)
    nc.same_bits(child.cpu().numpy(), nsga2.offspring(parents, rank, crowd, 1, lo, hi, seed=5)['child'], 'no optional outputs')


@pytest.mark.parametrize('n, M', [(2 * N, M) for N, _, M in SHAPES] + [(4100, 3)])     # 4100: 2 full j splits and one of 4, 9 LDS tiles
def test_crowding_and_select_match_the_mirror_bit_for_bit(engine0, n, M):
    rng = np.random.default_rng(31 * n + M)
    N = n // 2
    for name, obj, sense, rank in nc.planted(rng, n, M):
        obj_d, rank_d = dev(engine0, obj), dev(engine0, rank, torch.int32)
        crowd_d, info = engine0.nsga2_crowding(obj_d, sense, rank_d)
        want = nsga2.crowding(obj, sense, rank)
        nc.same_bits(crowd_d.cpu().numpy(), want, (name, n, M))
        assert info['n_used'] == int((rank >= 0).sum()) and info['pair_tests'] == n * n and info['n_fronts'] == 0
        rows = rng.standard_normal((5, n))
        got = engine0.nsga2_select(N, rank_d, crowd_d, rows=dev(engine0, rows))
        pos, survivor = nsga2.select(N, rank, want)
        assert np.array_equal(got['position'].cpu().numpy(), pos), (name, n, M)
        assert np.array_equal(got['survivor'].cpu().numpy(), survivor), (name, n, M)
        assert np.array_equal(got['rank'].cpu().numpy(), rank[survivor]), name
        nc.same_bits(got['crowd'].cpu().numpy(), want[survivor], name)
        nc.same_bits(got['rows'].cpu().numpy(), rows[:, survivor], name)
        assert got['n_used'] == N and got['pair_tests'] == n * n
        assert int((rank[survivor] < 0).sum()) == max(0, N - int((rank >= 0).sum())), name
    # a population sorted in place: n = N, and without rows
    got = engine0.nsga2_select(n, rank_d, crowd_d)
    assert np.array_equal(got['survivor'].cpu().numpy(), nsga2.select(n, rank, want)[1]) and got['rows'] is None


def test_a_whole_search_through_the_abi(engine0):
    """ZDT1 with the objectives computed on the host from the downloaded children: the population, ranks and crowding after every
    generation are the mirror's."""
    N, n_dim, n_gen, seed = 64, 8, 20, 3
    lo, hi, sense = np.zeros(n_dim), np.ones(n_dim), [-1, -1]
    target = np.full(n_dim, abi.MCMC_TARGET_NONE, dtype=np.int32)
    f64 = dict(dtype=torch.float64, device=engine0.tdev)
    _, records = nsga2.run(lambda x: nc.zdt1(x)[0], N, n_gen, sense, lo, hi, seed=seed)
    child = torch.empty((n_dim, N), **f64)
    engine0.nsga2_init(child, lo, hi, target, seed=seed)
    theta = obj = rank = crowd = None
    for t in range(n_gen + 1):
        if t:
            engine0.nsga2_offspring(theta, rank, crowd, t, lo, hi, target, child, seed=seed)
        cobj = dev(engine0, nc.zdt1(child.cpu().numpy())[0])
        pool = torch.cat([child, cobj]) if t == 0 else torch.cat([torch.cat([theta, child], dim=1), torch.cat([obj, cobj], dim=1)])
        all_obj = pool[n_dim:].contiguous()
        pr = engine0.pareto(all_obj, sense, counts=False)
        crowd_all, _ = engine0.nsga2_crowding(all_obj, sense, pr['rank'])
        sel = engine0.nsga2_select(N, pr['rank'], crowd_all, rows=pool.contiguous())
        theta, obj, rank, crowd = sel['rows'][:n_dim].contiguous(), sel['rows'][n_dim:].contiguous(), sel['rank'], sel['crowd']
        rec = records[t]
        nc.same_bits(child.cpu().numpy(), rec['child'], ('child', t))
        assert np.array_equal(sel['survivor'].cpu().numpy(), rec['survivor']), t
        nc.same_bits(theta.cpu().numpy(), rec['theta'], ('theta', t))
        assert np.array_equal(rank.cpu().numpy(), rec['rank']), t
        nc.same_bits(crowd.cpu().numpy(), rec['crowd'], ('crowd', t))
        assert pr['n_fronts'] == rec['n_fronts'] and pr['n_front0'] == rec['n_front0']
    assert np.median(nc.zdt1(theta.cpu().numpy())[1]) < np.median(nc.zdt1(records[0]['child'])[1])


# ---- refusals -----------------------------------------------------------------------------------------------------------------

def refused(engine0, entry, args, info_class):
    """(rc, message, the info's bytes) of a raw call with the info filled with 0xA5."""
    info = info_class()
    C.memset(C.byref(info), 0xA5, C.sizeof(info))
    rc = getattr(engine.lib(), entry)(*(args + (C.byref(info),)))
    return int(rc), engine.lib().simplyp_last_error(engine0._h).decode(), bytes(info)


def raw_calls(engine0, p):
    """name -> (a function of overrides that builds the raw argument tuple, the info class); the device arrays are 8 KiB regions
    of the buffer at ``p``, one per argument."""
    dbl, i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    keep = []
    a0, a1, a2, a3, a4, a5, a6, a7, a8 = (p + 8192 * k for k in range(9))

    def host(a, dtype):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dtype)
        keep.append(a)
        return a.ctypes.data_as(dbl if dtype == np.float64 else i32)

    def vary(with_t):
        def build(N=8, n_dim=2, seed=1, t=1, k_c=4, k_m=4, p_cross=0.9, p_mut=0.5, lo=(0.0, 0.0), hi=(1.0, 1.0), target=(2, -1), theta=a0, rank=a1,
                  crowd=a2, child=a3, parents=a4, mp=a5, ft=a6):
            head = (engine0._h, N, n_dim, C.c_uint64(seed))
            boxed = (host(lo, np.float64), host(hi, np.float64), host(target, np.int32))
            if with_t:
                return head + (C.c_uint32(t), k_c, k_m, C.c_double(p_cross), C.c_double(p_mut)) + boxed + (theta, rank, crowd, child, parents, mp, ft)
            return head + boxed + (theta, mp, ft)
        return build

    def crowding(n=8, M=2, obj=a0, sense=(1, -1), rank=a1, crowd=a2):
        return (engine0._h, n, M, obj, host(sense, np.int32), rank, crowd)

    def select(n=8, N=4, rank=a0, crowd=a1, position=a2, survivor=a3, n_rows=2, rows_in=a4, rows_out=a5, rank_out=a6, crowd_out=a7):
        return (engine0._h, n, N, rank, crowd, position, survivor, n_rows, rows_in, rows_out, rank_out, crowd_out)

    return {'simplyp_nsga2_init': (vary(False), abi.McmcInfo), 'simplyp_nsga2_offspring': (vary(True), abi.McmcInfo),
            'simplyp_nsga2_crowding': (crowding, abi.ParetoInfo), 'simplyp_nsga2_select': (select, abi.ParetoInfo)}, keep


NAN = float('nan')
BOX_REFUSALS = [dict(lo=(0.0, 1.0), hi=(1.0, 1.0)), dict(lo=(0.0, 2.0)), dict(lo=(NAN, 0.0)), dict(hi=(1.0, NAN)), dict(lo=None), dict(hi=None),
                dict(target=None), dict(target=(2, -3)), dict(target=(marshal.NP_M, 0)), dict(target=(4, 4)), dict(target=(-1, -1)),
                dict(mp=None), dict(ft=None), dict(N=7), dict(N=2), dict(N=0), dict(N=65538), dict(n_dim=0), dict(n_dim=17)]
REFUSALS = {
    'simplyp_nsga2_init': BOX_REFUSALS + [dict(theta=None)],
    'simplyp_nsga2_offspring': BOX_REFUSALS + [dict(theta=None), dict(rank=None), dict(crowd=None), dict(child=None), dict(k_c=0), dict(k_c=6),
                                               dict(k_m=0), dict(k_m=6), dict(p_cross=-0.5), dict(p_cross=1.5), dict(p_cross=NAN), dict(p_mut=-0.5),
                                               dict(p_mut=1.5), dict(p_mut=NAN)],
    'simplyp_nsga2_crowding': [dict(n=0), dict(n=131073), dict(M=0), dict(M=9), dict(obj=None), dict(sense=None), dict(rank=None), dict(crowd=None),
                               dict(sense=(1, 0)), dict(sense=(2, 1))],
    'simplyp_nsga2_select': [dict(N=5), dict(N=2), dict(n=3), dict(n=9), dict(N=65538, n=65538), dict(rank=None), dict(crowd=None), dict(position=None),
                             dict(survivor=None), dict(n_rows=-1), dict(n_rows=65), dict(rows_in=None), dict(rows_out=None)],
}


def test_every_refusal_launches_nothing_and_leaves_the_info(engine0):
    scratch = torch.zeros(1 << 16, dtype=torch.float64, device=engine0.tdev)            # room for any of the valid calls below
    calls, keep = raw_calls(engine0, scratch.data_ptr())
    for entry, cases in REFUSALS.items():
        build, info_class = calls[entry]
        for kw in cases:
            rc, msg, info = refused(engine0, entry, build(**kw), info_class)
            assert rc == -1 and msg.startswith(entry + ': '), (entry, kw, rc, msg)
            assert set(info) == {0xA5}, (entry, kw)
        null_ctx = (None,) + build()[1:]
        assert refused(engine0, entry, null_ctx, info_class)[0] == -1
    torch.cuda.synchronize()
    assert not bool(scratch.any())
    # a valid call afterwards works and writes every field of the info
    for entry in calls:
        build, info_class = calls[entry]
        rc, msg, info = refused(engine0, entry, build(), info_class)
        got = info_class.from_buffer_copy(info).as_dict()
        assert rc == 0 and got['kernel_ms'] > 0.0, (entry, msg)
        if info_class is abi.McmcInfo:
            assert (got['n_inside'], got['n_nan']) == (8, 0) and 0 <= got['n_accepted'] <= 4, (entry, got)
        else:
            assert (got['pair_tests'], got['n_fronts'], got['n_front0'], got['n_unranked']) == (64, 0, 0, 0) and got['n_used'] in (4, 8), (entry, got)
    del keep


def test_the_entries_refuse_while_a_run_is_pending(engine0):
    """As every analysis entry does: between Engine.run(defer_sync=True) and its finish() the four entries return SIMPLYP_ERR_ARG
    with the entry frame's text, launch nothing and leave the info they were handed as it was."""
    m = helpers.marshal_scenario('tarland_2004_static', E=64)
    args = (m['forcing'], m['doy'], m['member_params'], m['reach_params'], m['up_ptr'], m['up_idx'], m['opts'])
    ref, _, _ = engine0.run(*args)
    scratch = torch.zeros(1 << 16, dtype=torch.float64, device=engine0.tdev)
    calls, keep = raw_calls(engine0, scratch.data_ptr())
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out, status, st = engine0.run(*args, defer_sync=True)
        for entry, (build, info_class) in calls.items():
            rc, msg, info = refused(engine0, entry, build(), info_class)
            assert (rc, msg) == (-1, '%s: a run is pending on this context; call simplyp_sync first' % entry)
            assert set(info) == {0xA5}, entry
        st.update(st.pop('finish')())
    s.synchronize()
    assert not bool(scratch.any()) and bool(torch.equal(out, ref))
    del keep


# ---- the public call: Tarland 2004 --------------------------------------------------------------------------------------------

N_PUB, GEN_PUB, SEED_PUB = 64, 4, 11
OBJECTIVES = [('NSE', 'Q'), ('NSE', 'TP'), ('Bias (%)', 'Q')]


def public(**kw):
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
    obs_dict = helpers.observations(p_SU['st_dt'], p_SU['end_dt'])
    priors = {nm_: (0.7 * float(p[nm_]), 1.3 * float(p[nm_])) for nm_ in ('fc', 'T_g', 'E_M')}
    args = dict(priors=priors, objectives=OBJECTIVES, n_pop=N_PUB, n_gen=GEN_PUB, seed=SEED_PUB, record_children=True)
    args.update(kw)
    return sp.find_pareto(met, p_struc, p_SU, p_LU, p_SC, p, dyn, obs_dict, **args), args['priors'], obs_dict


@pytest.fixture(scope='module')
def res4(engine0):
    return public()


def table_rows(gof, objectives=OBJECTIVES):
    data = np.asarray(gof['data'])
    return np.stack([data[abi.GOF_STATS.index(s), abi.GOF_VARS.index(v), 0] for s, v in objectives])


def test_public_objectives_equal_an_independent_ensemble_run(engine0, res4):
    res, priors, obs_dict = res4
    assert res['names'] == ['fc', 'T_g', 'E_M'] and res['labels'] == ['NSE(Q)', 'NSE(TP)', '|Bias (%)|(Q)'] and res['sense'] == [1, 1, -1]
    assert res['x'].shape == (3, N_PUB) and res['objectives'].shape == (3, N_PUB) and res['children'].shape == (GEN_PUB + 1, 3, N_PUB)
    assert res['children_objectives'].shape == (GEN_PUB + 1, 3, N_PUB) and res['children_valid'].all()
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
    points = np.concatenate([res['x']] + list(res['children']), axis=1)
    ens = sp.run_simply_p_ensemble(met, p_struc, p_SU, p_LU, p_SC, p, dyn, overrides={n: points[d] for d, n in enumerate(res['names'])},
                                   obs_dict=obs_dict, keep_daily=False)
    assert int(ens['status'].max()) == 0
    want = table_rows(ens['gof'])
    got = np.concatenate([res['objectives']] + list(res['children_objectives']), axis=1)
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print('objectives against an independent run: worst %.3g' % err.max())
    assert np.isfinite(want).all() and (err <= 1e-9).all(), err.max()
    # (c) every position is inside its closed box; (d) the front is rank 0 and the result is sorted by (rank, -crowding)
    for d, n in enumerate(res['names']):
        assert (points[d] >= priors[n][0]).all() and (points[d] <= priors[n][1]).all()
    assert (res['rank'][res['front']] == 0).all() and np.array_equal(res['front'], np.flatnonzero(res['rank'] == 0)) and res['front'].size
    assert (np.diff(res['rank']) >= 0).all()
    assert all(res['crowding'][i] >= res['crowding'][i + 1] for i in range(N_PUB - 1) if res['rank'][i] == res['rank'][i + 1])
    assert sorted(res['overrides']) == ['E_M', 'T_g', 'fc'] and np.array_equal(res['overrides']['fc'], res['x'][0])
    # the result goes straight back into the ensemble call
    one = sp.run_simply_p_ensemble(met, p_struc, p_SU, p_LU, p_SC, p, dyn, overrides=res['overrides'], obs_dict=obs_dict, keep_daily=False)
    again = table_rows(one['gof'])
    assert (np.abs(again - res['objectives']) <= 1e-9 * np.maximum(1.0, np.abs(again))).all()
    h = res['history']
    assert len(h['n_front0']) == len(h['n_fronts']) == len(h['n_invalid']) == GEN_PUB + 1 and h['best'].shape == (GEN_PUB + 1, 3)
    assert h['n_invalid'] == [0] * (GEN_PUB + 1) and min(h['n_front0'][-1], N_PUB) == res['front'].size
    ranked = np.where(res['absolute'][:, None], np.abs(res['objectives']), res['objectives'])
    assert np.array_equal(h['best'][-1], [ranked[0].max(), ranked[1].max(), ranked[2].min()])
    assert (np.diff(h['best'][:, 0]) >= 0).all() and (np.diff(h['best'][:, 2]) <= 0).all()        # elitism: an objective's best never worsens
    st = res['stats']
    assert all(len(st[k]) == GEN_PUB + 1 for k in st) and min(st['run_kernel_ms']) > 0.0 and min(st['crowding_ms']) > 0.0


def test_public_path_is_the_mirrors_replay_of_the_recorded_objectives(engine0, res4):
    res, priors, _ = res4
    lo = np.array([priors[n][0] for n in res['names']]); hi = np.array([priors[n][1] for n in res['names']])
    gens = iter(range(GEN_PUB + 1))
    seen = []

    def recorded(points):
        g = next(gens)
        nc.same_bits(points, res['children'][g], ('children', g))             # the mirror asks for the points the device ran
        seen.append(g)
        obj = res['children_objectives'][g]
        return np.where(res['absolute'][:, None], np.abs(obj), obj), res['children_valid'][g]

    nc.same_bits(res['children'][0], nsga2.initial_population(N_PUB, lo, hi, SEED_PUB), 'the initial population')
    state, records = nsga2.run(recorded, N_PUB, GEN_PUB, res['sense'], lo, hi, seed=SEED_PUB)
    assert seen == list(range(GEN_PUB + 1))
    for g, rec in enumerate(records):
        assert np.array_equal(res['survivors'][g], rec['survivor']), g
        assert np.array_equal(res['ranks'][g], rec['rank']), g
        nc.same_bits(res['crowdings'][g], rec['crowd'], ('crowding', g))
        assert res['history']['n_fronts'][g] == rec['n_fronts'] and res['history']['n_front0'][g] == rec['n_front0']
    nc.same_bits(res['x'], state['theta'], 'x')
    assert np.array_equal(res['rank'], state['rank']) and res['state']['t'] == state['t'] == GEN_PUB
    nc.same_bits(res['crowding'], state['crowd'], 'crowding')
    nc.same_bits(np.where(res['absolute'][:, None], np.abs(res['objectives']), res['objectives']), state['obj'], 'objectives')


def test_public_continuation_and_determinism(engine0, res4):
    res = res4[0]
    first, _, _ = public(n_gen=2)
    second, _, _ = public(n_gen=2, state=first['state'])
    twice, _, _ = public()
    for other in (second, twice):
        for k in ('x', 'objectives', 'crowding'):
            nc.same_bits(other[k], res[k], k)
        assert np.array_equal(other['rank'], res['rank']) and other['state']['t'] == GEN_PUB
    nc.same_bits(np.concatenate([first['children'], second['children']]), res['children'], 'children')
    nc.same_bits(twice['children_objectives'], res['children_objectives'], 'children_objectives')
    assert second['children'].shape[0] == 2 and first['history']['n_fronts'] + second['history']['n_fronts'] == res['history']['n_fronts']


def test_planted_invalid_members_never_win_and_leave(engine0):
    """A start with members at a corner of the closed box where the model goes non-finite (a groundwater time constant of zero):
    they are invalid after generation 0, sorted last, lose every tournament against a valid member, and are gone after the first
    selection."""
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
    priors = {'fc': (0.7 * float(p['fc']), 1.3 * float(p['fc'])), 'T_g': (0.0, 1.3 * float(p['T_g']))}
    lo = np.array([priors[n][0] for n in priors]); hi = np.array([priors[n][1] for n in priors])
    N, planted = 16, [1, 6, 11]
    start = nsga2.initial_population(N, lo, hi, 2)
    start[1] = np.maximum(start[1], 0.5 * hi[1])
    start[1, planted] = 0.0
    res, _, _ = public(priors=priors, n_pop=N, n_gen=1, start=start, seed=2)
    nc.same_bits(res['children'][0], start, 'the start')
    assert np.array_equal(np.flatnonzero(~res['children_valid'][0]), planted) and res['children_valid'][1].all()
    assert res['history']['n_invalid'] == [3, 3]                    # generation 1 ranks the three as parents once more, for the last time
    assert (res['ranks'][0][-3:] == -1).all() and (res['ranks'][0][:-3] >= 0).all() and (res['crowdings'][0][-3:] == 0.0).all()
    assert sorted(res['survivors'][0][-3:]) == planted
    # generation 1's tournaments, replayed: wherever a valid member met an invalid one, the valid one became the parent
    x = nsga2._draw(2, np.arange(N // 2), 1, nsga2.TOURNAMENT)
    cand = [((w.astype(np.uint64) * np.uint64(N)) >> np.uint64(32)).astype(int) for w in x]
    par = nsga2.mating(N, 1, res['ranks'][0], res['crowdings'][0], seed=2)
    for k, (a, b) in enumerate(((cand[0], cand[1]), (cand[2], cand[3]))):
        mixed = (a >= N - 3) != (b >= N - 3)
        assert (par[k][mixed] < N - 3).all()
    assert (res['rank'] >= 0).all() and np.isfinite(res['objectives']).all() and res['children_valid'][1].all()
    assert (res['x'][1] > 0.0).all()
