"""Weighted bands on the device (simplyp_weighted_quantiles, simplyp_predictive_bands_weighted) against the Python-integer
statement of the rule (simplyp_amd/weighted.py).  Every comparison is bit for bit, -0.0 and +0.0 counting as equal: the rule
is integer arithmetic, there is no tolerance anywhere.

Sizes are where the kernels can go wrong: E around the wavefront (63, 64, 65), around the LDS sort's longest row (2048, 2049)
and the unweighted sort's (4096, 4097), rows the radix select sweeps in one, two and three trips of 4096 members with a ragged
tail (4097, 9000); 1, 3 and 17 rows pack a sort workgroup fully, partly and leave a partial last workgroup.  Rows whose wanted
buckets hold exactly 32 or 33 weighted members, and 65536 + 36 rows (more than the select's grid has workgroups), also pin
n_passes to the count of tests/selection_model.py."""

import ctypes as C
import os

import numpy as np
import pytest

import helpers
import simplyp_amd as sp
from simplyp_amd import abi, engine, marshal, weighted

import selection_cases as sc
import selection_model as sm
import weighted_cases as wc

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 1000, 2048, 2049, 4096, 4097, 9000]
ERR_ARG = -1
PATTERN = -123.456


def dev(eng, a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(eng.tdev)


def dev_weights(eng, q):
    return dev(eng, np.asarray(q).astype(np.int64))


def check(eng, table, q, probs, include=None, member_of_slot=None, mirror=None, what=None):
    """One call against the mirror; returns (values, info)."""
    got, info = eng.weighted_quantiles(dev(eng, table), probs, q, include=include, member_of_slot=member_of_slot)
    want = weighted.quantiles(table, q, probs, include=include) if mirror is None else mirror
    got = got.cpu().numpy()
    assert got.shape == want.shape == (len(probs),) + table.shape[:-1]
    assert wc.same_bits(got, want), (what, np.argwhere(got.view(np.uint64) != want.view(np.uint64))[:5])
    return got, info


@pytest.mark.parametrize('E', SIZES)
def test_made_up_tables_equal_the_mirror(engine0, E):
    rng = np.random.default_rng(100 + E)
    extra = [float(p) for p in rng.uniform(0, 1, 11)]
    n = 0
    for n_rows in (1, 3, 17):
        for vp in wc.VALUE_PATTERNS:
            table = wc.values(vp, (n_rows, E), rng)
            for wp in wc.WEIGHT_PATTERNS:
                q = wc.weights(wp, E, rng)
                for probs in ([wc.PROBS[(n_rows + n) % 5]], wc.PROBS + extra):          # K = 1 and K = 16
                    got, info = check(engine0, table, q, probs, what=(E, n_rows, vp, wp, len(probs)))
                    T = sum(int(v) for v in q)
                    assert info['T'] == T and info['n_used'] == int((q > 0).sum())
                    assert info['bytes_table'] == n_rows * E * 8
                    if T == 0:
                        assert np.isnan(got).all() and info['n_passes'] == 0
                    else:
                        assert 1 <= info['n_passes'] <= 8
                    n += 1
    assert n == 3 * 3 * 6 * 2


@pytest.mark.parametrize('E', SIZES[1:])
def test_probabilities_on_a_running_sum_boundary(engine0, E):
    """T a power of two: p = C_i / T is a float, p T is an integer, and the first member with C_i >= t is member i itself; one ulp
    below still selects it, one ulp above the next member with a weight.  This is where >= against > shows."""
    rng = np.random.default_rng(200 + E)
    for vp in ('normals', 'ties'):
        table = wc.values(vp, (3, E), rng)
        q = wc.power_of_two_total(E, rng)
        probs = wc.boundary_probs(table[0], q, n=4, rng=rng) + [0.0, 0.5, 1.0, 2.0 ** -30]
        assert len(probs) == 16
        _, info = check(engine0, table, q, probs, what=(E, vp))
        assert info['T'] == 1 << 30 and info['n_used'] == E
        # the boundary itself selects the sorted row's member i, the next float up the member after it
        order = np.argsort(table[0], kind='stable')
        C = np.cumsum(q[order])
        for p in probs[:12]:
            t = weighted.threshold(p, 1 << 30)
            assert weighted.quantile_row(table[0], q, p) == table[0][order[int(np.searchsorted(C, t, side='left'))]]


@pytest.mark.parametrize('E', [1000, 2049, 4097, 9000])
def test_all_equal_rows_and_rows_over_600_binades(engine0, E):
    rng = np.random.default_rng(300 + E)
    q = wc.weights('zeros30', E, rng)
    flat = np.full((2, E), 3.25)
    flat[1, :] = -0.0
    _, info = check(engine0, flat, q, wc.PROBS, what=('flat', E))
    assert info['n_passes'] == (8 if E > 2048 else 1)                       # the select walks the whole key; the sort makes one sweep
    wide = np.ldexp(rng.uniform(1, 2, (3, E)), rng.integers(-300, 301, (3, E))) * rng.choice([-1.0, 1.0], (3, E))
    _, info = check(engine0, wide, q, wc.PROBS + [float(p) for p in rng.uniform(0, 1, 11)], what=('wide', E))
    assert 1 <= info['n_passes'] <= 8


def model_of(table, q, probs):
    """tests/selection_model.py on every row: (values [K, n_rows], the largest sweep count)."""
    T = sum(int(v) for v in q)
    got = [sm.member_select(row, [weighted.threshold(p, T) for p in probs], weights=q) for row in table]
    return np.stack([g[0] for g in got], axis=1), max(g[1] for g in got)


@pytest.mark.parametrize('case', sc.weighted_cases(), ids=lambda c: c[0])
@pytest.mark.parametrize('n_rows', [1, 3, 17])
def test_rows_on_the_list_limit(engine0, case, n_rows):
    """WQLIST = 32, the bucket size at which weighted_select_kernel collects -- counted in members that carry a weight (chist),
    not in weight (hist): rows of E = 2049 (the shortest the select takes) whose wanted buckets hold exactly 32 or 33 such
    members after the first digit, and one of 33 members of which one has weight 0, which counts as 32.  n_passes tells the
    path: 2 = first digit, collect; 3 = the 33 part in the second digit; 4 = in the third; two groups of 32 and 33: 3 with a
    threshold in the larger, 2 without.  tests/selection_cases.py derives the numbers."""
    rng = np.random.default_rng(100 * n_rows + len(case[0]))
    q = wc.weights('zeros30', sc.E_WSELECT, rng)
    table, probs, _ = sc.weighted_table(case, q, n_rows, rng)
    assert table.shape == (n_rows, sm.WQSORT_MAX + 1)
    _, info = check(engine0, table, q, probs, what=case[0])
    values, model_sweeps = model_of(table, q, probs)
    assert wc.same_bits(values, weighted.quantiles(table, q, probs))
    assert info['n_passes'] == model_sweeps == case[5]


@pytest.fixture(scope='module')
def capped(engine0):
    """65536 + 36 rows of 2049 members (1.07 GB), made on the device from six base rows and a power of two per row."""
    import torch
    rng = np.random.default_rng(65536)
    q = wc.weights('zeros30', sc.E_WSELECT, rng)
    base = sc.base_rows(sc.E_WSELECT, sm.WQLIST, rng, weights=q)
    kind, scale = sc.capped_rows(65536, len(base), rng)
    table = torch.from_numpy(base).to(engine0.tdev)[torch.from_numpy(kind).to(engine0.tdev)]
    table.mul_(torch.from_numpy(scale).to(engine0.tdev)[:, None])
    made = dict(q=q, base=base, kind=kind, scale=scale, table=table)
    del table
    yield made
    made.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize('K', [5, 16])
def test_rows_past_the_grid_cap(engine0, capped, K):
    """select_launch caps the grid at 65536 workgroups and radix_select<WQSelect> strides over the rows (r += gridDim.x),
    carrying collect, G, prefix, count and list_n in LDS from one row to the next behind one barrier.  Workgroup i < 36 selects
    row i and then row 65536 + i: every ordered pair of six kinds of row (distinct, ties, flat, specials, wanted bucket of 32, of
    33).  A power of two scales the values exactly and leaves their order alone, so the expected values are the base rows' times
    the row's scale.  The flat rows take all 8 digits at any scale, so n_passes is 8: the model's maximum over the kinds."""
    q, base, kind, scale, table = (capped[k] for k in ('q', 'base', 'kind', 'scale', 'table'))
    N = len(kind)
    assert N == 65536 + 36 and tuple(table.shape) == (N, 2049)
    assert {(int(kind[i]), int(kind[65536 + i])) for i in range(36)} == {(a, b) for a in range(6) for b in range(6)}
    probs = wc.PROBS + [float(p) for p in np.random.default_rng(K).uniform(0, 1, K - 5)]
    got, info = engine0.weighted_quantiles(table, probs, q)
    values, model_sweeps = model_of(base, q, probs)
    want = weighted.quantiles(base, q, probs)
    assert wc.same_bits(np.nan_to_num(values, nan=7.0), np.nan_to_num(want, nan=7.0))
    got, want = got.cpu().numpy(), want[:, kind] * scale
    assert got.shape == want.shape == (K, N)
    assert np.array_equal(got, want, equal_nan=True), np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5]
    assert info['n_passes'] == model_sweeps == 8 and info['T'] == sum(int(v) for v in q) and info['bytes_table'] == N * 2049 * 8


@pytest.mark.parametrize('E', [65, 2049, 4097])
def test_include_and_member_of_slot(engine0, E):
    rng = np.random.default_rng(400 + E)
    perm = rng.permutation(E).astype(np.int32)                              # slot j holds member perm[j]
    by_member = wc.values('special', (5, E), rng)
    by_slot = np.ascontiguousarray(by_member[:, perm])
    q = rng.integers(0, 1000, E).astype(np.uint64)
    q[int(rng.integers(0, E))] = 1 << 40
    inc = rng.random(E) < 0.8
    inc[int(np.argmax(q))] = False                                          # the mask removes the heaviest member
    probs = wc.PROBS
    want = weighted.quantiles(by_member, q, probs, include=inc)
    assert not wc.same_bits(want, weighted.quantiles(by_member, q, probs))  # ... which changes the band
    mos = dev(engine0, perm)
    _, info = check(engine0, by_slot, q, probs, include=inc, member_of_slot=mos, mirror=want, what=('slots', E))
    assert wc.same_bits(want, weighted.quantiles(by_slot, q[perm], probs, include=inc[perm]))
    assert info['T'] == sum(int(v) for v in q[inc]) and info['n_used'] == int(((q > 0) & inc).sum())
    _, info = check(engine0, by_member, q, probs, include=inc, what=('members', E))
    # nobody left: every output NaN, T = 0, the call succeeds
    for kw in (dict(include=np.zeros(E, dtype=bool)), dict()):
        qq = q if kw else np.zeros(E, dtype=np.uint64)
        got, info = engine0.weighted_quantiles(dev(engine0, by_slot), probs, qq, member_of_slot=mos, **kw)
        assert np.isnan(got.cpu().numpy()).all() and info['T'] == 0 and info['n_used'] == 0


@pytest.mark.parametrize('E', [64, 2048, 9000])
def test_the_same_call_twice_gives_the_same_bits(engine0, E):
    rng = np.random.default_rng(500 + E)
    table = dev(engine0, wc.values('ties', (17, E), rng))
    q = dev_weights(engine0, wc.weights('zeros30', E, rng))
    probs = wc.PROBS + [float(p) for p in rng.uniform(0, 1, 11)]
    a, ia = engine0.weighted_quantiles(table, probs, q)
    b, ib = engine0.weighted_quantiles(table, probs, q)
    assert np.array_equal(a.cpu().numpy().view(np.uint64), b.cpu().numpy().view(np.uint64))
    assert (ia['T'], ia['n_used'], ia['n_passes']) == (ib['T'], ib['n_used'], ib['n_passes'])


def raw_call(eng, E, n_rows, table, weights, probs, K, out):
    import torch
    L = engine.lib()
    qa = None if probs is None else np.ascontiguousarray(probs, dtype=np.float64)
    info = abi.WqInfo()
    with torch.cuda.device(eng.tdev):
        eng._bind_stream()
        rc = L.simplyp_weighted_quantiles(eng._h, E, n_rows, None if table is None else table.data_ptr(), None, None,
                                          None if weights is None else weights.data_ptr(),
                                          None if qa is None else qa.ctypes.data_as(C.POINTER(C.c_double)), K,
                                          None if out is None else out.data_ptr(), C.byref(info))
        torch.cuda.synchronize(eng.tdev)
    return rc, L.simplyp_last_error(eng._h).decode()


def test_refusals_write_nothing(engine0):
    import torch
    E, n_rows = 100, 4
    rng = np.random.default_rng(6)
    table = dev(engine0, wc.values('normals', (n_rows, E), rng))
    q = dev_weights(engine0, wc.weights('ones', E, rng))
    heavy = wc.weights('ones', E, rng)
    heavy[17] = (1 << 40) + 1
    out = torch.full((17, n_rows), PATTERN, dtype=torch.float64, device=engine0.tdev)
    cases = [(E, n_rows, table, q, [], 0), (E, n_rows, table, q, [0.5] * 17, 17), (E, n_rows, table, q, [1.5], 1),
             (E, n_rows, table, q, [0.5, float('nan')], 2), (E, n_rows, table, dev_weights(engine0, heavy), [0.5], 1),
             (E, n_rows, table, None, [0.5], 1), ((1 << 22) + 1, n_rows, table, q, [0.5], 1), (0, n_rows, table, q, [0.5], 1),
             (E, -1, table, q, [0.5], 1), (E, n_rows, None, q, [0.5], 1), (E, n_rows, table, q, None, 1)]
    for E_, rows_, t_, w_, probs, K in cases:
        rc, msg = raw_call(engine0, E_, rows_, t_, w_, probs, K, out)
        assert rc == ERR_ARG and msg.startswith('simplyp_weighted_quantiles: '), (rc, msg, E_, rows_, K)
        assert bool((out == PATTERN).all()), msg
    assert raw_call(engine0, E, n_rows, table, q, [0.5], 1, None)[0] == ERR_ARG
    assert raw_call(engine0, E, 0, table, q, [0.5], 1, out)[0] == 0 and bool((out == PATTERN).all())     # n_rows == 0 succeeds
    rc, msg = raw_call(engine0, E, n_rows, table, dev_weights(engine0, np.full(E, 1 << 40)), [0.5], 1, out)
    assert rc == 0 and bool((out[0] != PATTERN).all()) and bool((out[1:] == PATTERN).all())                # 2^40 itself is a weight
    with pytest.raises(engine.EngineError, match='exceed 2\\^40'):
        engine0.weighted_quantiles(table, [0.5], heavy)
    with pytest.raises(ValueError):
        engine0.weighted_quantiles(table, [0.5], np.ones(E))                                              # floats are not weights
    with pytest.raises(ValueError):
        engine0.weighted_quantiles(table, [0.5], np.ones(E + 1, dtype=np.int64))


# ---- predictive_bands(weights=) on a small run -----------------------------------------------------------------------------
NAME = 'tarland_2004_dynamic'
FLUX4 = ['Qr', 'Msus_kg/day', 'TDP_kg/day', 'PP_kg/day']
Q_ID = abi.TQ_DERIVED + abi.TQ_DERIVED_SERIES.index('Q_cumecs')
SEED = 77
_runs = {}


def small_run(E):
    """The 2004 scenario with E members (a_Q, T_g, E_M, fc scaled by seeded factors): the daily table on the device."""
    if E not in _runs:
        met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
        base = helpers.marshal_scenario(NAME, E=1)['member_params'][:, 0]
        rng = np.random.default_rng(E)
        over = {nm: base[marshal.PM_NAMES.index(nm)] * rng.uniform(lo, hi, E)
                for nm, lo, hi in (('a_Q', 0.6, 1.6), ('T_g', 0.7, 1.4), ('E_M', 0.5, 2.0), ('fc', 0.85, 1.15))}
        res = sp.run_simply_p_ensemble(met, p_struc, p_SU, p_LU, p_SC, p, dyn, overrides=over, outputs=FLUX4, to_host=False)
        rp = np.zeros((len(marshal.PR_NAMES), 1, E))
        rp[marshal.PR_NAMES.index('A_catch')] = float(p_SC.loc['A_catch', 1])
        _runs[E] = dict(out=res['data'], mask=marshal.mask_of_columns(res['columns']), kw=dict(f_tdp=float(p['f_TDP']), reach_params=rp))
    return _runs[E]


@pytest.mark.parametrize('E', [64, 5000])
@pytest.mark.parametrize('noisy', [False, True])
def test_predictive_bands_weighted(engine0, E, noisy):
    run = small_run(E)
    rng = np.random.default_rng(E + noisy)
    m = rng.uniform(0.05, 0.4, (1, E)) if noisy else None
    q = wc.weights('zeros30', E, rng)
    # p E is 1.6064 / 32 / 62.4064 and 125.5 / 2500 / 4875.5: away from the integers, or exactly on one with an exact p, so numpy's
    # fp64 product p * E below rounds to the same side as the exact one (0.025 * 5000 would not: it rounds DOWN onto 125)
    probs = [0.0251, 0.5, 0.9751]
    args = (run['out'], run['mask'], probs, [Q_ID])
    kw = dict(err_m=m, seed=SEED, day0=10, **run['kw'])
    series = engine0.predictive_series(run['out'], run['mask'], [Q_ID], err_m=m, seed=SEED, day0=10, **run['kw']).cpu().numpy()
    got, info = engine0.predictive_bands(*args, weights=q, **kw)
    got = got.cpu().numpy()
    want = weighted.quantiles(series, q, probs)
    assert got.shape == want.shape == (3, 1, 366, 1) and wc.same_bits(got, want)
    assert info['T'] == sum(int(v) for v in q) and info['n_used'] == int((q > 0).sum())
    # independent of the chunk length
    old = os.environ.get('SIMPLYP_PRED_CHUNK_DAYS')
    try:
        for days in ('7', '100'):
            os.environ['SIMPLYP_PRED_CHUNK_DAYS'] = days
            again, _ = engine0.predictive_bands(*args, weights=q, **kw)
            assert np.array_equal(again.cpu().numpy().view(np.uint64), got.view(np.uint64)), days
    finally:
        if old is None:
            os.environ.pop('SIMPLYP_PRED_CHUNK_DAYS', None)
        else:
            os.environ['SIMPLYP_PRED_CHUNK_DAYS'] = old
    # all weights equal: numpy's inverted_cdf band across the members
    for unit in (1, 1 << 40):
        flat, _ = engine0.predictive_bands(*args, weights=np.full(E, unit, dtype=np.uint64), **kw)
        assert wc.same_bits(flat.cpu().numpy(), np.quantile(series, probs, axis=-1, method='inverted_cdf'))
    # the unweighted entry is untouched by the new keyword's default
    lo, up, pinfo = engine0.predictive_bands(*args, **kw)
    assert lo.shape == (3, 1, 366, 1) and pinfo['n_used'] == E
