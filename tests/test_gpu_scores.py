"""Scores on the device (simplyp_scores, simplyp_predictive_scores) against the exact statement of the rule in Python integers and
fractions (simplyp_amd/score.py).

The counts are integers: compared with ==.  A and B are sums of non-negative terms of at most 8 roundings each, added as 1024
per-lane partials of at most 4096 terms and a tree of at most 22 levels: (8 + 4096 + 22) 2^-53 = 4.6e-13, so each must lie within
1e-12 of its exact value RELATIVE TO ITSELF (CRPS is never compared relative to itself: it cancels).  Equality between two device
results -- chunked against unchunked, the same call twice, no weights against unit weights, a row in another place of the table,
the predictive entry against the materialised series -- is bit for bit.

Sizes are where the kernels can go wrong: E around the wavefront (63, 64, 65), around the LDS tile (TILE - 1, TILE, TILE + 1: one
tile padded, full, and a second tile of one member), 2 TILE and 2 TILE + 1 (one merge pass without and with a run of one),
3 TILE + 5 (an odd run out in the merge tree) and 2^17 + 3 (33 tiles, six merge levels, 129 blocks of the gap pass); 1 and 7 rows,
and 5 rows in chunks of 2."""

import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

import helpers
import simplyp_amd as sp
from simplyp_amd import abi, engine, marshal, score

import weighted_cases as wc

pytestmark = pytest.mark.gpu

TILE = abi.SCORE_TILE
SIZES = [1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1, 3 * TILE + 5, (1 << 17) + 3]
assert SIZES[-1] >= 9 * TILE + 3
ERR_ARG = -1
PATTERN = -123.456
COUNT_PATTERN = 0x5A5A5A5A
REL = Fraction(1, 10 ** 12)


def dev(eng, a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(eng.tdev)


class chunk_rows:
    """SIMPLYP_SCORE_CHUNK_ROWS for the calls inside."""
    def __init__(self, n):
        self.n = n

    def __enter__(self):
        self.old = os.environ.get('SIMPLYP_SCORE_CHUNK_ROWS')
        os.environ['SIMPLYP_SCORE_CHUNK_ROWS'] = str(self.n)

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop('SIMPLYP_SCORE_CHUNK_ROWS', None)
        else:
            os.environ['SIMPLYP_SCORE_CHUNK_ROWS'] = self.old


def observations(table, rng, with_nan):
    """One observation per row: below all, above all, on a value of the row, +-0.0 or between two values; NaN interleaved."""
    y = np.empty(table.shape[0])
    for r, x in enumerate(table):
        fin = np.sort(x[np.isfinite(x)])
        if len(fin) == 0:
            fin = np.array([0.0])
        k = int(rng.integers(0, len(fin)))
        pick = int(rng.integers(0, 6))
        y[r] = [fin[0] - 1.5, fin[-1] + 2.25, fin[k], 0.0, -0.0, 0.5 * (fin[k] + fin[min(k + 1, len(fin) - 1)])][pick]
    if with_nan:
        y[1::3] = np.nan
    return y


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(np.uint64) == b.view(np.uint64)).all())


def call(eng, table, y, **kw):
    sums, counts, info = eng.scores(table if not isinstance(table, np.ndarray) else dev(eng, table), y, **kw)
    return sums.cpu().numpy(), counts.cpu().numpy(), info


def against_mirror(got, table, y, q, include=None, what=None):
    """Counts ==, A and B within 1e-12 of the exact values relative to themselves, NaN exactly where the rule says."""
    sums, counts, info = got
    want = score.scores(table, y, q, include)
    assert info['T'] == want['T'], what
    assert (counts[0] == want['below'].astype(np.int64)).all() and (counts[1] == want['at_or_below'].astype(np.int64)).all(), what
    worst = Fraction(0)
    for r in range(table.shape[0]):
        ex = want['exact'][r]
        if ex is None:
            assert np.isnan(sums[0, r]) and np.isnan(sums[1, r]), (what, r)
            continue
        for k in range(2):
            err = abs(Fraction(float(sums[k, r])) - ex[k])
            assert err <= REL * ex[k], (what, r, k, float(sums[k, r]), float(ex[k]))
            if ex[k] > 0:
                worst = max(worst, err / ex[k])
        # CRPS: within 1e-12 (A + B), never relative to itself
        assert abs(Fraction(float(sums[0, r])) - Fraction(float(sums[1, r])) - (ex[0] - ex[1])) <= REL * (ex[0] + ex[1])
    assert info['n_rows_scored'] == (int((~np.isnan(y)).sum()) if want['T'] > 0 else 0), what
    return float(worst)


@pytest.mark.parametrize('E', SIZES)
def test_made_up_tables_equal_the_mirror(engine0, E):
    rng = np.random.default_rng(700 + E)
    combos = [(vp, wp) for vp in wc.VALUE_PATTERNS for wp in wc.WEIGHT_PATTERNS]
    if E > 4 * TILE:                                    # every value and weight pattern once: the mirror is Python integers
        combos = [(wc.VALUE_PATTERNS[i % 3], wp) for i, wp in enumerate(wc.WEIGHT_PATTERNS)]
    worst = 0.0
    for c, (vp, wp) in enumerate(combos):
        n_rows = (1, 7, 5)[c % 3]
        table = wc.values(vp, (n_rows, E), rng)
        if vp == 'special':
            table[0, int(rng.integers(0, E))] = 0.0
        q = wc.weights(wp, E, rng)
        y = observations(table, rng, with_nan=n_rows > 1)
        d_table = dev(engine0, table)
        got = call(engine0, d_table, y, weights=q)
        worst = max(worst, against_mirror(got, table, y, q, what=(E, vp, wp, n_rows)))
        sums, counts, info = got
        T = sum(int(v) for v in q)
        assert info['n_used'] == int((q > 0).sum())
        if T == 0:                                      # nobody takes part: NaN and 0, and the call succeeds
            assert np.isnan(sums).all() and (counts == 0).all() and info['n_chunks'] == 0
        else:
            assert info['n_chunks'] == 1 and info['bytes_workspace'] == 32 * E * info['n_rows_scored']
        if vp == 'special' and T > 0:
            part = table[:, q > 0]
            bad = ~np.isfinite(part).all(axis=1) & ~np.isnan(y)
            assert np.isnan(sums[:, bad]).all() and (counts[1, bad] <= T).all()
            ok = np.isfinite(part).all(axis=1) & ~np.isnan(y)
            assert not np.isnan(sums[:, ok]).any()
        if n_rows == 5:                                 # the scored rows in chunks of 2: the same bits
            with chunk_rows(2):
                s2, c2, i2 = call(engine0, d_table, y, weights=q)
            assert same_bits(s2, sums) and same_bits(c2, counts), (E, vp, wp)
            assert i2['n_chunks'] == (-(-info['n_rows_scored'] // 2) if T > 0 else 0)
    print('E = %d: largest relative error of A or B %.3e' % (E, worst))


@pytest.mark.parametrize('E', [65, TILE + 1, 3 * TILE + 5])
def test_no_weights_are_unit_weights_and_place_does_not_matter(engine0, E):
    rng = np.random.default_rng(800 + E)
    table = wc.values('normals', (7, E), rng)
    table[3] = wc.values('ties', (E,), rng)
    y = observations(table, rng, with_nan=True)
    d_table = dev(engine0, table)
    none = call(engine0, d_table, y)
    ones = call(engine0, d_table, y, weights=np.ones(E, dtype=np.uint64))
    assert same_bits(none[0], ones[0]) and same_bits(none[1], ones[1]) and none[2]['T'] == E
    against_mirror(none, table, y, None, what=('no weights', E))
    again = call(engine0, d_table, y)                                       # the same call twice
    assert same_bits(again[0], none[0]) and same_bits(again[1], none[1])
    # the rows in reverse order, alone, and in chunks of 3: a row's outputs go with the row
    back = call(engine0, np.ascontiguousarray(table[::-1]), y[::-1].copy())
    assert same_bits(back[0][:, ::-1], none[0]) and same_bits(back[1][:, ::-1], none[1])
    alone = call(engine0, table[2:3].copy(), y[2:3].copy())
    assert same_bits(alone[0][:, 0], none[0][:, 2]) and same_bits(alone[1][:, 0], none[1][:, 2])
    with chunk_rows(3):
        parts = call(engine0, d_table, y)
    assert same_bits(parts[0], none[0]) and same_bits(parts[1], none[1]) and parts[2]['n_chunks'] == 2
    # a higher-rank table: the leading axes are kept
    s3, c3, _ = engine0.scores(d_table.reshape(7, 1, E), y.reshape(7, 1))
    assert tuple(s3.shape) == (2, 7, 1) and same_bits(s3.cpu().numpy().reshape(2, 7), none[0])
    s1, c1, _ = engine0.scores(d_table[2], y[2])                            # and a single row needs none
    assert tuple(s1.shape) == (2,) and same_bits(s1.cpu().numpy(), none[0][:, 2]) and same_bits(c1.cpu().numpy(), none[1][:, 2])


@pytest.mark.parametrize('E', [65, TILE + 1, 2 * TILE + 1])
def test_include_and_member_of_slot(engine0, E):
    rng = np.random.default_rng(900 + E)
    perm = rng.permutation(E).astype(np.int32)                              # slot j holds member perm[j]
    by_member = wc.values('ties', (5, E), rng) + 0.25 * rng.standard_normal((5, E))
    by_slot = np.ascontiguousarray(by_member[:, perm])
    q = rng.integers(0, 1000, E).astype(np.uint64)
    q[int(rng.integers(0, E))] = 1 << 40
    inc = rng.random(E) < 0.8
    inc[int(np.argmax(q))] = False                                          # the mask removes the heaviest member
    y = observations(by_member, rng, with_nan=True)
    mos = dev(engine0, perm)
    got = call(engine0, by_slot, y, weights=q, include=inc, member_of_slot=mos)
    against_mirror(got, by_member, y, q, include=inc, what=('slots', E))
    assert got[2]['T'] == sum(int(v) for v in q[inc]) and got[2]['n_used'] == int(((q > 0) & inc).sum())
    direct = call(engine0, by_member, y, weights=q, include=inc)
    against_mirror(direct, by_member, y, q, include=inc, what=('members', E))
    assert same_bits(direct[1], got[1])                                     # the counts do not see the order of the columns
    nobody = call(engine0, by_slot, y, weights=q, include=np.zeros(E, dtype=bool), member_of_slot=mos)
    assert np.isnan(nobody[0]).all() and (nobody[1] == 0).all() and nobody[2]['T'] == 0 and nobody[2]['n_used'] == 0


def raw_call(eng, E, n_rows, table, weights, y, sums, counts):
    import torch
    L = engine.lib()
    ya = None if y is None else np.ascontiguousarray(y, dtype=np.float64)
    info = abi.ScoreInfo()
    with torch.cuda.device(eng.tdev):
        eng._bind_stream()
        rc = L.simplyp_scores(eng._h, E, n_rows, None if table is None else table.data_ptr(), None, None,
                              None if weights is None else weights.data_ptr(),
                              None if ya is None else ya.ctypes.data_as(C.POINTER(C.c_double)),
                              None if sums is None else sums.data_ptr(), None if counts is None else counts.data_ptr(), C.byref(info))
        torch.cuda.synchronize(eng.tdev)
    return rc, L.simplyp_last_error(eng._h).decode(), info


def test_refusals_write_nothing(engine0):
    import torch
    E, n_rows = 100, 4
    rng = np.random.default_rng(8)
    table = dev(engine0, wc.values('normals', (n_rows, E), rng))
    y = rng.standard_normal(n_rows)
    heavy = wc.weights('ones', E, rng).astype(np.int64)
    heavy[17] = (1 << 40) + 1
    sums = torch.full((2, n_rows), PATTERN, dtype=torch.float64, device=engine0.tdev)
    counts = torch.full((2, n_rows), COUNT_PATTERN, dtype=torch.int64, device=engine0.tdev)
    untouched = lambda: bool((sums == PATTERN).all()) and bool((counts == COUNT_PATTERN).all())
    inf_y = y.copy()
    inf_y[2] = -np.inf
    cases = [(0, n_rows, table, None, y, sums, counts), ((1 << 22) + 1, n_rows, table, None, y, sums, counts),
             (E, -1, table, None, y, sums, counts), (E, n_rows, None, None, y, sums, counts), (E, n_rows, table, None, None, sums, counts),
             (E, n_rows, table, None, inf_y, sums, counts), (E, n_rows, table, dev(engine0, heavy), y, sums, counts)]
    for c in cases:
        rc, msg, _ = raw_call(engine0, *c)
        assert rc == ERR_ARG and msg.startswith('simplyp_scores: '), (rc, msg)
        assert untouched(), msg
    assert raw_call(engine0, E, n_rows, table, None, y, None, counts)[0] == ERR_ARG
    assert raw_call(engine0, E, n_rows, table, None, y, sums, None)[0] == ERR_ARG and untouched()
    assert raw_call(engine0, E, 0, table, None, y, sums, counts)[0] == 0 and untouched()              # n_rows == 0 succeeds
    rc, msg, info = raw_call(engine0, E, n_rows, table, None, np.full(n_rows, np.nan), sums, counts)  # no observation at all
    assert rc == 0 and info.n_rows_scored == 0 and info.n_chunks == 0
    assert bool(torch.isnan(sums).all()) and bool((counts == 0).all())
    rc, msg, info = raw_call(engine0, E, n_rows, table, dev(engine0, np.full(E, 1 << 40, dtype=np.int64)), y, sums, counts)
    assert rc == 0 and info.T == E << 40 and not bool(torch.isnan(sums).any())                         # 2^40 itself is a weight
    with pytest.raises(engine.EngineError, match='exceed 2\\^40'):
        engine0.scores(table, y, weights=heavy)
    with pytest.raises(engine.EngineError, match='infinite'):
        engine0.scores(table, inf_y)
    with pytest.raises(ValueError):
        engine0.scores(table, y[:3])
    with pytest.raises(ValueError):
        engine0.scores(table, y, weights=np.ones(E))                                                  # floats are not weights


# ---- simplyp_predictive_scores on a small run ------------------------------------------------------------------------------
NAME = 'tarland_2004_dynamic'
FLUX4 = ['Qr', 'Msus_kg/day', 'TDP_kg/day', 'PP_kg/day']
SERIES = [abi.TQ_DERIVED + abi.TQ_DERIVED_SERIES.index(s) for s in ('Q_cumecs', 'TDP_mgl')]
SEED = 91
E_RUN = 256
_run = {}


def small_run():
    """The 2004 scenario with 256 members (a_Q, T_g, E_M, fc scaled by seeded factors): the daily table on the device."""
    if not _run:
        met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(NAME)
        base = helpers.marshal_scenario(NAME, E=1)['member_params'][:, 0]
        rng = np.random.default_rng(E_RUN)
        over = {nm: base[marshal.PM_NAMES.index(nm)] * rng.uniform(lo, hi, E_RUN)
                for nm, lo, hi in (('a_Q', 0.6, 1.6), ('T_g', 0.7, 1.4), ('E_M', 0.5, 2.0), ('fc', 0.85, 1.15))}
        res = sp.run_simply_p_ensemble(met, p_struc, p_SU, p_LU, p_SC, p, dyn, overrides=over, outputs=FLUX4, to_host=False)
        rp = np.zeros((len(marshal.PR_NAMES), 1, E_RUN))
        rp[marshal.PR_NAMES.index('A_catch')] = float(p_SC.loc['A_catch', 1])
        _run.update(out=res['data'], mask=marshal.mask_of_columns(res['columns']), kw=dict(f_tdp=float(p['f_TDP']), reach_params=rp))
    return _run


@pytest.mark.parametrize('noisy', [False, True])
@pytest.mark.parametrize('day0', [0, 40])
def test_predictive_scores_equal_series_then_scores(engine0, noisy, day0):
    run = small_run()
    rng = np.random.default_rng(day0 + noisy)
    m = rng.uniform(0.05, 0.4, (2, E_RUN)) if noisy else None
    kw = dict(err_m=m, seed=SEED, day0=day0, **run['kw'])
    series = engine0.predictive_series(run['out'], run['mask'], SERIES, **kw)
    host = series.cpu().numpy()
    assert host.shape == (2, 366, 1, E_RUN)
    # daily discharge observations with a gap, fortnightly chemistry: around the ensemble, some outside it
    obs = np.full((2, 366, 1), np.nan)
    q_days = np.r_[0:200, 230:366]
    obs[0, q_days, 0] = np.median(host[0, q_days, 0], axis=-1) * rng.uniform(0.3, 2.5, len(q_days))
    obs[1, 5::14, 0] = host[1, 5::14, 0, 17]                                # on a member's value
    q = wc.weights('zeros30', E_RUN, rng)
    inc = rng.random(E_RUN) < 0.9
    for weights, include in ((None, None), (q, inc)):
        want_s, want_c, want_i = engine0.scores(series, obs, weights=weights, include=include)
        got_s, got_c, got_i = engine0.predictive_scores(run['out'], run['mask'], SERIES, obs, weights=weights, include=include, **kw)
        assert tuple(got_s.shape) == (2, 2, 366, 1)
        assert same_bits(got_s.cpu().numpy(), want_s.cpu().numpy()) and same_bits(got_c.cpu().numpy(), want_c.cpu().numpy())
        n_obs = int((~np.isnan(obs)).sum())
        assert got_i['n_rows_scored'] == want_i['n_rows_scored'] == n_obs and got_i['T'] == want_i['T']
        assert got_i['bytes_workspace'] == 40 * E_RUN * n_obs and got_i['n_chunks'] == 1
        with chunk_rows(100):                                               # four chunks: the same bits
            part_s, part_c, part_i = engine0.predictive_scores(run['out'], run['mask'], SERIES, obs, weights=weights, include=include, **kw)
        assert same_bits(part_s.cpu().numpy(), got_s.cpu().numpy()) and same_bits(part_c.cpu().numpy(), got_c.cpu().numpy())
        assert part_i['n_chunks'] == -(-n_obs // 100)
    # and the rule itself, on the chemistry days
    days = np.arange(5, 366, 14)
    mirror = score.scores(host[1, days, 0], obs[1, days, 0], q, inc)
    s, c = got_s.cpu().numpy()[:, 1, days, 0], got_c.cpu().numpy()[:, 1, days, 0]
    assert (c[0] == mirror['below'].astype(np.int64)).all() and (c[1] == mirror['at_or_below'].astype(np.int64)).all()
    assert (c[1] > c[0]).all() or not inc[17] or q[17] == 0                 # the observation sits on member 17's value
    for r, ex in enumerate(mirror['exact']):
        for k in range(2):
            assert abs(Fraction(float(s[k, r])) - ex[k]) <= REL * ex[k]


def test_predictive_scores_refusals(engine0):
    run = small_run()
    obs = np.full((2, 366, 1), np.nan)
    obs[0, 3, 0] = 1.0
    with pytest.raises(engine.EngineError, match='simplyp_predictive_scores: '):
        engine0.predictive_scores(run['out'], run['mask'], SERIES, obs, day0=-1, **run['kw'])
    with pytest.raises(engine.EngineError, match='simplyp_predictive_scores: '):
        engine0.predictive_scores(run['out'], run['mask'], [999], obs[:1], **run['kw'])
    bad = obs.copy()
    bad[1, 7, 0] = np.inf
    with pytest.raises(engine.EngineError, match='infinite'):
        engine0.predictive_scores(run['out'], run['mask'], SERIES, bad, **run['kw'])
    with pytest.raises(ValueError):
        engine0.predictive_scores(run['out'], run['mask'], SERIES, obs[:, :10], **run['kw'])
    none = np.full((2, 366, 1), np.nan)                                     # no observation at all succeeds
    s, c, info = engine0.predictive_scores(run['out'], run['mask'], SERIES, none, **run['kw'])
    assert bool(s.isnan().all()) and bool((c == 0).all()) and info['n_rows_scored'] == 0 and info['n_chunks'] == 0
