"""The scoring rules (simplyp_amd/csrc/simplyp_score.h: the two term functions, the reference scoring of a row, the list of scored
rows, the PIT helpers, the scoring entries' argument checks), exercised on the CPU: tests/score_host_main.cpp includes the header,
is built once per session with the host compiler under AddressSanitizer and UBSan, and runs as a child process that reads cases
as text.  The header is compared with simplyp_amd/score.py's statement in Python integers and fractions, and that with the
double sum B is defined by.  No GPU needed.

Tolerances: the counts are integers and compared with ==.  The header's reference sums in long double (64-bit significand):
n <= 200 terms of a few roundings each and one rounding to double stay below 200 * 4 * 2^-64 + 2^-53 = 1.6e-16 relative, inside
the 1e-15 asked of it."""

import os
import re
from fractions import Fraction

import numpy as np
import pytest

from simplyp_amd import abi, engine, score

import host_program
import weighted_cases as wc
from c_header import header_text
from host_program import rejected

SIZES = (1, 2, 7, 64, 200)


@pytest.fixture(scope='session')
def driver():
    return host_program.case_runner(host_program.build('score_host_main.cpp'), timeout=120)


def as_float(bits):
    return float(np.array([int(bits)], dtype=np.uint64).view(np.float64)[0])


def observations(x, rng):
    """The observations a row is scored against: below all, above all, on a (tied) value, +-0.0, between two values, NaN."""
    fin = np.sort(x[np.isfinite(x)])
    if len(fin) == 0:
        fin = np.array([0.0])
    ys = [float(fin[0]) - 1.5, float(fin[-1]) + 2.25, float(fin[int(rng.integers(0, len(fin)))]), 0.0, -0.0, float('nan')]
    if len(fin) > 1:
        k = int(rng.integers(0, len(fin) - 1))
        ys.append(0.5 * (float(fin[k]) + float(fin[k + 1])))
    return ys


def row_case(y, x, q, inc):
    arr = lambda v: 'null' if v is None else '%d %s' % (len(v), ' '.join(str(int(t)) for t in v))
    return 'row %s %d %s %s %s' % (float(y).hex(), len(x), ' '.join(float(v).hex() for v in x), arr(q), arr(inc))


def close(got, want, rel):
    """|got - want| <= rel * want for a float ``got`` and an exact, non-negative Fraction ``want``."""
    return abs(Fraction(got) - want) <= Fraction(rel) * want


def test_rows_equal_the_python_statement(driver):
    rng = np.random.default_rng(31)
    cases = []
    for E in SIZES:
        for vp in wc.VALUE_PATTERNS:
            x = wc.values(vp, (E,), rng)
            if vp != 'ties':
                x[int(rng.integers(0, E))] = 0.0                          # a zero in the row for y = +-0.0
            for wp in wc.WEIGHT_PATTERNS + (None,):
                q = None if wp is None else wc.weights(wp, E, rng)
                inc = None if (E + len(cases)) % 3 else rng.random(E) < 0.7
                for y in observations(x, rng):
                    cases.append((y, x, q, inc))
    got = driver([row_case(*c) for c in cases])
    n_scored = n_nan = 0
    pairwise = {}                                                        # B does not depend on y: once per (row, weights, mask)
    for (y, x, q, inc), (rc, rest) in zip(cases, got):
        a_bits, b_bits, below, at, T = (int(v) for v in rest.split())
        A, B = as_float(a_bits), as_float(b_bits)
        want = score.score_row(x, y, q, inc)
        assert rc == 0 and (below, at, T) == (want['below'], want['at_or_below'], want['T']), (y, x, q, inc)
        assert below <= at <= T
        if want['abs_err'] is None:
            assert np.isnan(A) and np.isnan(B)
            n_nan += 1
            continue
        assert close(A, want['abs_err'], 1e-15) and close(B, want['spread'], 1e-15), (A, B, want)
        key = (id(x), id(q), id(inc))
        if key not in pairwise:
            pairwise[key] = score.pairwise_spread(x, q, inc)
        assert want['spread'] == pairwise[key]                           # the gap form is the double sum, exactly
        assert want['abs_err'] >= want['spread'] >= 0                    # CRPS >= 0
        n_scored += 1
    assert n_scored > 350 and n_nan > 200 and len(cases) > 700, (n_scored, n_nan)


def test_python_scores_table():
    rng = np.random.default_rng(37)
    table = wc.values('normals', (2, 3, 9), rng)
    table[1, 2, 4] = np.nan
    y = rng.standard_normal((2, 3))
    y[0, 1] = np.nan
    q = wc.weights('zeros30', 9, rng)
    s = score.scores(table, y, q)
    assert s['crps'].shape == (2, 3) and s['T'] == sum(int(v) for v in q)
    assert np.isnan(s['crps'][0, 1]) and s['below'][0, 1] == 0 and s['exact'][0, 1] is None
    assert np.isnan(s['abs_err'][1, 2]) == bool(q[4] > 0)                # the NaN member matters iff it takes part
    one = score.score_row(table[1, 0], y[1, 0], q)
    assert s['exact'][1, 0] == (one['abs_err'], one['spread']) and s['crps'][1, 0] == float(one['abs_err'] - one['spread'])
    with pytest.raises(ValueError):
        score.scores(table, np.full((2, 3), np.inf), q)
    with pytest.raises(ValueError):
        score.scores(table, y[0], q)
    with pytest.raises(ValueError):
        score.score_row(table[0, 0], 0.0, np.full(9, (1 << 40) + 1))


def test_properties():
    rng = np.random.default_rng(41)
    for _ in range(20):
        x, y = float(rng.standard_normal()), float(rng.standard_normal())
        s = score.score_row([x], y, [int(rng.integers(1, 1 << 40))])
        assert s['spread'] == 0 and s['abs_err'] == abs(Fraction(x) - Fraction(y))          # E = 1: CRPS = |x - y|
    for E in (2, 7, 64):
        x = wc.values('ties', (E,), rng) + (rng.random(E) < 0.5) * rng.standard_normal(E)
        q = rng.integers(0, 5, E).astype(np.uint64)
        q[0] = 3
        y = float(x[int(rng.integers(0, E))])
        s = score.score_row(x, y, q)
        # all weights times a constant: only the counts change, by that constant
        k = 1 << 20
        t = score.score_row(x, y, q * np.uint64(k))
        assert (t['abs_err'], t['spread']) == (s['abs_err'], s['spread'])
        assert (t['below'], t['at_or_below'], t['T']) == (k * s['below'], k * s['at_or_below'], k * s['T'])
        # a member of weight k is k members of weight 1
        rep = np.repeat(x, q.astype(np.int64))
        u = score.score_row(rep, y)
        assert u == s
        assert s['below'] <= s['at_or_below'] <= s['T']
        # CRPS is the integral of (F - 1{x >= y})^2: piecewise constant between the sorted values and y
        pts = sorted(set(float(v) for v in x[q > 0]) | {y})
        integral = Fraction(0)
        for a, b in zip(pts[:-1], pts[1:]):
            F = Fraction(sum(int(w) for v, w in zip(x, q) if v <= a), s['T'])
            integral += (Fraction(b) - Fraction(a)) * (F - (1 if a >= y else 0)) ** 2
        assert integral == s['abs_err'] - s['spread']


def test_terms_are_the_written_expressions(driver):
    rng = np.random.default_rng(43)
    cases = []
    for _ in range(100):
        T = int(rng.integers(1, 1 << 62))
        Cw = int(rng.integers(0, T + 1))
        q = int(rng.integers(1, min(T, 1 << 40) + 1))
        lo, gap = float(rng.standard_normal()), float(rng.random())
        cases.append((float(rng.standard_normal()), float(rng.standard_normal()), q, lo, lo + gap, Cw, T))
    got = driver(['terms %s %s %d %s %s %d %d' % (x.hex(), y.hex(), q, lo.hex(), hi.hex(), Cw, T) for x, y, q, lo, hi, Cw, T in cases])
    for (x, y, q, lo, hi, Cw, T), (rc, rest) in zip(cases, got):
        a, b = (as_float(v) for v in rest.split())
        assert rc == 0 and a == abs(x - y) * (float(q) / float(T))
        assert b == (hi - lo) * ((float(Cw) / float(T)) * (float(T - Cw) / float(T)))
        assert a >= 0 and b >= 0
        # within 8 roundings of the exact term
        assert close(a, abs(Fraction(x) - Fraction(y)) * Fraction(q, T), 8 * 2.0 ** -53)
        assert close(b, (Fraction(hi) - Fraction(lo)) * Fraction(Cw * (T - Cw), T * T), 8 * 2.0 ** -53)


def test_scored_rows_and_chunks(driver):
    nan = float('nan').hex()
    got = driver(['obs 5 %s 0x1p0 %s -0x1p3 0x0p0' % (nan, nan), 'obs 0', 'obs 2 %s %s' % (nan, nan),
                  'obs 3 0x1p0 inf 0x1p1', 'obs 1 -inf'])
    assert got[0] == (0, '1 3 4') and got[1] == (0, '') and got[2] == (0, '')
    rejected(got[3:])
    budget = 256 << 20
    got = driver(['chunk 10957 3200000 %d null' % budget, 'chunk 10 3200000 %d null' % budget, 'chunk 5 8192 %d 2' % budget,
                  'chunk 5 8192 %d 0' % budget, 'chunk 3 %d %d null' % (budget * 2, budget), 'chunk 0 800 %d null' % budget,
                  'chunk 5 8192 %d 9' % budget, 'chunk 10957 3200000 %d 1000' % budget, 'chunk 10957 3200000 %d 40' % budget])
    assert [int(r) for _, r in got] == [83, 10, 2, 5, 1, 1, 5, 83, 40]        # the environment shortens a chunk, never past the budget


def test_pit(driver):
    rng = np.random.default_rng(47)
    T = (1 << 61) + 12345
    pairs = [(0, 0), (0, T), (T, T), (5, 5), (T // 3, T // 2)] + [tuple(sorted(int(v) for v in rng.integers(0, T + 1, 2))) for _ in range(40)]
    got = driver(['pit %d %d %d' % (l, m, T) for l, m in pairs] + ['pit 0 0 0'])
    want = score.pit([l for l, _ in pairs], [m for _, m in pairs], T)
    for (rc, rest), w in zip(got[:-1], want):
        assert rc == 0 and as_float(rest) == w and 0.0 <= w <= 1.0
    assert np.isnan(as_float(got[-1][1])) and np.isnan(score.pit([3], [4], 0)).all()
    assert list(score.pit([0, 1], [2, 3], 4)) == [0.25, 0.5]
    # the histogram: point masses, 1.0 into the last bin, an interval over several bins
    h = score.pit_histogram([0, 10, 3, 0, 2], [0, 10, 3, 10, 7], 10, 5)
    assert np.allclose(h, np.array([1, 0, 0, 0, 1]) + np.array([0, 1, 0, 0, 0]) + 0.2 + np.array([0, 0.4, 0.4, 0.2, 0]), rtol=0, atol=1e-15)
    assert abs(h.sum() - 5) < 1e-14
    for n_bins, TT in ((10, 1000), (7, T)):
        ps = [(l % (TT + 1), m % (TT + 1)) for l, m in pairs]
        ps = [(min(p), max(p)) for p in ps]
        rc, rest = driver(['hist %d %d %d %s' % (n_bins, TT, len(ps), ' '.join('%d %d' % p for p in ps))])[0]
        hd = np.array([as_float(v) for v in rest.split()])
        hp = score.pit_histogram([l for l, _ in ps], [m for _, m in ps], TT, n_bins)
        assert rc == 0 and np.allclose(hd, hp, rtol=0, atol=1e-12) and abs(hp.sum() - len(ps)) < 1e-12
    seen = np.array([True, False, True, False, True])                   # unscored rows are 0 and 0: masked out, not counted in bin 0
    hm = score.pit_histogram([0, 0, 3, 0, 2], [0, 0, 3, 0, 7], 10, 5, observed=seen)
    assert np.array_equal(hm, score.pit_histogram([0, 3, 2], [0, 3, 7], 10, 5)) and abs(hm.sum() - 3) < 1e-15
    with pytest.raises(ValueError):
        score.pit_histogram([3, 4], [3, 4], 10, 5, observed=[True])
    with pytest.raises(ValueError):
        score.pit_histogram([3], [2], 10, 5)
    with pytest.raises(ValueError):
        score.pit_histogram([3], [4], 10, 0)


def test_argument_checks(driver):
    check = lambda E=10, n_rows=3, table=1, y=1, sums=1, counts=1: 'check %d %d %d %d %d %d' % (E, n_rows, table, y, sums, counts)
    ok = driver([check(), check(E=1, n_rows=0), check(E=1 << 22)])
    assert [rc for rc, _ in ok] == [0] * 3
    rejected(driver([check(E=0), check(E=(1 << 22) + 1), check(n_rows=-1), check(table=0), check(y=0), check(sums=0), check(counts=0)]))


def test_exports_and_tile():
    engine.build()
    L = engine.lib()
    declared = set(re.findall(r'\b(simplyp_[a-z0-9_]*scores)\s*\(', header_text()))
    assert declared == {'simplyp_scores', 'simplyp_predictive_scores'}
    for name in declared:
        assert name in engine.ABI_SYMBOLS and hasattr(L, name), name
    m = re.search(r'constexpr int SCORE_TILE = (\d+);', open(os.path.join(engine.CSRC, 'simplyp_score.h')).read())
    assert int(m.group(1)) == abi.SCORE_TILE


def test_public_refusals_come_before_any_device_call():
    import helpers
    import simplyp_amd as sp
    name = 'tarland_2004_dynamic'
    for kw, msg in ((dict(), 'score needs obs_dict'), (dict(obs_dict={}, reduce='annual'), 'cannot be combined with reduce'),
                    (dict(obs_dict={}, devices=[0]), r'devices=\[...\]'), (dict(obs_dict={}, predictive_seed=1 << 64), 'predictive_seed'),
                    (dict(obs_dict={}, predictive_m={'Qr': 0.1}), 'predictive_m names')):
        met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(name)
        with pytest.raises(ValueError, match=msg):
            sp.run_simply_p_ensemble(met, p_struc, p_SU, p_LU, p_SC, p, dyn, n_members=4, score=True, **kw)
