"""Pareto dominance on the CPU: the plain C++ rules of simplyp_amd/csrc/simplyp_pareto.h (tests/pareto_host_main.cpp includes the
header, is built once per session with the host compiler under AddressSanitizer and UBSan, and runs as a child process that
reads cases as text) against simplyp_amd/pareto.py's statement in NumPy and Python integers, that statement against a case
enumerated by hand, the key map, the header's and the kernels' constants, and the objective resolver.  No GPU needed."""

import os
import re

import numpy as np
import pytest

from simplyp_amd import abi, engine, pareto

import host_program
from c_header import c_values
from host_program import ME, rejected


@pytest.fixture(scope='session')
def driver():
    return host_program.case_runner(host_program.build('pareto_host_main.cpp'), timeout=120)


def hexf(v):
    v = float(v)
    return 'nan' if v != v else float(v).hex()


def ref_case(obj, sense, max_fronts=0, mos=None, inc=None):
    M, E = obj.shape
    opt = lambda a: 'null' if a is None else '%d %s' % (len(a), ' '.join(str(int(v)) for v in a))
    return 'ref %d %d %d %s %s %s %s' % (M, E, max_fronts, ' '.join(str(int(s)) for s in sense),
                                         ' '.join(hexf(v) for v in obj.reshape(-1)), opt(mos), opt(inc))


def parse_ref(rest, E):
    v = [int(x) for x in rest.split()]
    assert len(v) == 5 + 3 * E
    return dict(n_used=v[0], n_fronts=v[1], n_front0=v[2], n_unranked=v[3], pair_tests=v[4],
                dominated_by=np.array(v[5:5 + E]), dominates=np.array(v[5 + E:5 + 2 * E]), rank=np.array(v[5 + 2 * E:]))


def same(got, want):
    for k in ('n_used', 'n_fronts', 'n_front0', 'n_unranked', 'pair_tests'):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ('dominated_by', 'dominates', 'rank'):
        assert np.array_equal(got[k], want[k]), k


def tables(rng):
    """(name, obj [M, E]) of every kind the rule distinguishes."""
    out = []
    for E, M in ((1, 1), (2, 2), (37, 1), (64, 2), (150, 3), (90, 8)):
        out.append(('normals', rng.standard_normal((M, E))))
        out.append(('ties', rng.integers(0, 8, (M, E)).astype(np.float64)))
    dup = rng.standard_normal((3, 20))
    out.append(('duplicates', np.concatenate([dup, dup, dup[:, :7]], axis=1)))
    nanny = rng.integers(0, 4, (3, 80)).astype(np.float64)
    nanny[rng.integers(0, 3, 25), rng.integers(0, 80, 25)] = np.nan
    out.append(('nan', nanny))
    edge = rng.choice([0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, 5e-324, -5e-324], (3, 120))
    out.append(('zeros and infinities', edge))
    out.append(('all nan', np.full((2, 9), np.nan)))
    return out


def test_reference_equals_the_python_statement(driver):
    rng = np.random.default_rng(41)
    cases = []
    for name, obj in tables(rng):
        M, E = obj.shape
        for F in (0, 1, 3):
            sense = rng.choice([1, -1], M)
            inc = None if len(cases) % 3 == 0 else (rng.random(E) < 0.7)
            cases.append((name, obj, sense, F, inc))
    cases.append(('nobody included', rng.standard_normal((2, 12)), [1, 1], 0, np.zeros(12, dtype=bool)))
    got = driver([ref_case(obj, sense, F, inc=inc) for _, obj, sense, F, inc in cases])
    seen_unranked = seen_excluded = 0
    for (name, obj, sense, F, inc), (rc, rest) in zip(cases, got):
        assert rc == 0, (name, rest)
        have = parse_ref(rest, obj.shape[1])
        want = pareto.ranks(obj, sense, include=inc, max_fronts=F, block=32)
        same(have, want)
        seen_unranked += want['n_unranked']
        seen_excluded += int((want['rank'] == pareto.EXCLUDED).sum())
        assert (want['rank'] == pareto.EXCLUDED).sum() == obj.shape[1] - want['n_used']
        if want['n_used'] == 0:
            assert want['n_fronts'] == 0 and (want['dominated_by'] == -1).all() and (want['dominates'] == -1).all()
        if F:
            full = pareto.ranks(obj, sense, include=inc, block=64)
            assert np.array_equal(want['rank'], np.where(full['rank'] >= F, pareto.UNRANKED, full['rank']))
            assert np.array_equal(want['dominated_by'], full['dominated_by']) and np.array_equal(want['dominates'], full['dominates'])
    assert seen_unranked > 100 and seen_excluded > 50


def test_member_of_slot_and_include(driver):
    """Column j holds member mos[j]; include is in member order; the outputs are in member order."""
    rng = np.random.default_rng(43)
    E, M = 70, 3
    obj = rng.integers(0, 6, (M, E)).astype(np.float64)          # member order
    inc = rng.random(E) < 0.6
    mos = rng.permutation(E)
    want = pareto.ranks(obj, [1, -1, 1], include=inc)
    (rc, rest), = driver([ref_case(obj[:, mos], [1, -1, 1], mos=mos, inc=inc)])
    assert rc == 0
    same(parse_ref(rest, E), want)
    # an entry outside [0, E) names nobody: its column takes no part and nothing is written for it
    bad = mos.copy()
    bad[5], bad[9] = -1, E
    inc2 = inc.copy()
    inc2[[mos[5], mos[9]]] = False
    (rc, rest), = driver([ref_case(obj[:, mos], [1, -1, 1], mos=bad, inc=inc)])
    same(parse_ref(rest, E), pareto.ranks(obj, [1, -1, 1], include=inc2))


def test_hand_enumerated_case():
    """Six members, objective 0 maximised and objective 1 minimised; y = (a, -b):
         0: (3, 1)   1: (2, 2)   2: (3, 1) a copy of 0   3: (1, 3)   4: (4, 5)   5: (NaN, 0) takes no part
       0 and 2 are equal and dominate 1 and 3 (3 >= 2, 1 <= 2; 3 >= 1, 1 <= 3); 1 dominates 3; 4 has the best a and the worst b:
       nobody dominates it and it dominates nobody.  Fronts: {0, 2, 4}, {1}, {3}."""
    nan = float('nan')
    obj = np.array([[3.0, 2.0, 3.0, 1.0, 4.0, nan], [1.0, 2.0, 1.0, 3.0, 5.0, 0.0]])
    got = pareto.ranks(obj, [1, -1])
    assert got['dominated_by'].tolist() == [0, 2, 0, 3, 0, -1]
    assert got['dominates'].tolist() == [2, 1, 2, 0, 0, -1]
    assert got['rank'].tolist() == [0, 1, 0, 2, 0, -1]
    assert (got['n_used'], got['n_fronts'], got['n_front0'], got['n_unranked']) == (5, 3, 3, 0)
    assert got['pair_tests'] == 25 + 3 * 2 + 1 * 1
    cut = pareto.ranks(obj, [1, -1], max_fronts=2)
    assert cut['rank'].tolist() == [0, 1, 0, -2, 0, -1] and cut['dominated_by'].tolist() == [0, 2, 0, 3, 0, -1]
    assert (cut['n_fronts'], cut['n_unranked']) == (2, 1)
    masked = pareto.ranks(obj, [1, -1], include=[0, 1, 0, 1, 1, 1])      # without 0 and 2 member 1 is on the front
    assert masked['rank'].tolist() == [-1, 0, -1, 1, 0, -1] and masked['dominates'].tolist() == [-1, 1, -1, 0, 0, -1]
    assert pareto.ranks(-obj, [-1, 1])['rank'].tolist() == got['rank'].tolist()
    for bad in (dict(obj=np.zeros((9, 3)), sense=[1] * 9), dict(obj=np.zeros((2, 3)), sense=[1, 0]), dict(obj=np.zeros((2, 3)), sense=[1]),
                dict(obj=np.zeros((2, 3)), sense=[1, 1], max_fronts=-1), dict(obj=np.zeros((2, 3)), sense=[1, 1], include=[1, 1]),
                dict(obj=np.zeros(3), sense=[1])):
        with pytest.raises(ValueError):
            pareto.ranks(**bad)


def test_key_is_strictly_monotone_and_joins_the_zeros(driver):
    edge = [-np.inf, -1.7976931348623157e308, -1.0, -2.2250738585072014e-308, -5e-324, 0.0, 5e-324, 2.2250738585072014e-308,
            1.0 - 2.0 ** -53, 1.0, 1.0 + 2.0 ** -52, 1.7976931348623157e308, np.inf]
    for sense in (1, -1):
        got = driver(['key %s %d' % (hexf(x), sense) for x in edge] + ['key -0x0p+0 %d' % sense])
        ks = [int(rest) for rc, rest in got]
        assert all(rc == 0 for rc, _ in got)
        assert ks[:-1] == [pareto.key(x, sense) for x in edge]
        assert ks[-1] == ks[edge.index(0.0)] == pareto.key(-0.0, sense) == pareto.key(0.0, sense)
        steps = np.diff(np.array(ks[:-1], dtype=object))
        assert all(s > 0 for s in steps) if sense > 0 else all(s < 0 for s in steps)
        assert [int(k) for k in pareto.keys(np.array([edge]), [sense])[0]] == ks[:-1]
    with pytest.raises(ValueError):
        pareto.key(float('nan'), 1)


def test_argument_checks(driver):
    def check(E=10, M=2, obj=1, F=0, by=1, of=1, rank=1, sense='auto'):
        s = [1, -1, 1, 1, -1, 1, 1, 1][:max(0, min(M, 8))] if sense == 'auto' else sense
        return 'check %d %d %d %d %d %d %d %s' % (E, M, obj, F, by, of, rank,
                                                  'null' if s is None else '%d %s' % (len(s), ' '.join(str(v) for v in s)))
    ok = driver([check(), check(E=1, M=1), check(M=8), check(E=1 << 24), check(by=0, of=0), check(by=0, rank=0), check(F=5),
                 check(of=0, rank=0)])
    assert [rc for rc, _ in ok] == [0] * 8, ok
    bad = driver([check(E=0), check(E=-3), check(E=(1 << 24) + 1), check(M=0), check(M=9), check(M=-1), check(obj=0), check(sense=None),
                  check(sense=[1, 0]), check(sense=[2, 1]), check(M=3, sense=[1, 1, -2]), check(F=-1), check(by=0, of=0, rank=0)])
    rejected(bad)
    # the reference path of the driver goes through the same checks
    (rc, msg), = driver(['ref 1 2 -1 1 0x1p+0 0x1p+1 null null'])
    assert rc == -1 and msg.startswith(ME + ': ') and 'max_fronts' in msg


def test_constants():
    """The header's constants against abi's, and the kernels' constants."""
    got = c_values(['SIMPLYP_PARETO_MAX_OBJ', 'SIMPLYP_PARETO_EXCLUDED', 'SIMPLYP_PARETO_UNRANKED'])
    assert (got['SIMPLYP_PARETO_MAX_OBJ'], got['SIMPLYP_PARETO_EXCLUDED'], got['SIMPLYP_PARETO_UNRANKED']) == (abi.PARETO_MAX_OBJ, abi.PARETO_EXCLUDED, abi.PARETO_UNRANKED)
    # the kernels' constants, as the header of the kernels states them
    with open(os.path.join(engine.CSRC, 'simplyp_pareto.hip.h')) as fh:
        txt = fh.read()
    for name in ('THREADS', 'JTILE', 'JSPLIT'):
        assert int(re.search(r'constexpr int PARETO_%s = (\d+);' % name, txt).group(1)) == getattr(abi, 'PARETO_' + name)
    assert abi.PARETO_JSPLIT % abi.PARETO_JTILE == 0


def test_objective_resolver():
    r = pareto.resolve_objectives([('NSE', 'Q'), ('log NSE', 'Q'), ('r2', 'TDP'), ('nRMSD (%)', 'PP'), ('Bias (%)', 'Q'),
                                   ('spearman', 'SS', 0)], has_spearman=True)
    assert [o['sense'] for o in r] == [1, 1, 1, -1, -1, 1]
    assert [o['absolute'] for o in r] == [False, False, False, False, True, False]
    assert [o['stat_index'] for o in r] == [abi.GOF_STATS.index(s) for s in ('NSE', 'log NSE', 'r2', 'nRMSD (%)', 'Bias (%)')] + [None]
    assert [o['var_index'] for o in r] == [abi.GOF_VARS.index(v) for v in ('Q', 'Q', 'TDP', 'PP', 'Q', 'SS')]
    assert r[4]['label'] == '|Bias (%)|(Q)' and r[0]['label'] == 'NSE(Q)'
    # an explicit sense: the statistic as it is, whatever it is
    r = pareto.resolve_objectives([('N obs', 'Q', 1, 1), ('sum_relsq', 'TP', 0, -1), ('Bias (%)', 'Q', 0, 1)], n_reaches=2)
    assert [(o['sense'], o['absolute'], o['reach']) for o in r] == [(1, False, 1), (-1, False, 0), (1, False, 0)]
    assert r[0]['label'] == 'N obs(Q)[1]'
    for bad in ([('N obs', 'Q')], [('sum_log_sim', 'Q')], [('sum_relsq', 'Q', 0)], [('spearman', 'Q')], [('KGE', 'Q')], [('NSE', 'NO3')],
                [('NSE', 'Q', 1)], [('NSE', 'Q', -1)], [('NSE', 'Q', 0, 0)], [('NSE',)], [], [('NSE', 'Q')] * 9, 5):
        with pytest.raises(ValueError):
            pareto.resolve_objectives(bad)
    assert all(pareto.DEFAULT_SENSE[s] is None for s in ('N obs', 'sum_log_sim', 'sum_relsq'))
    assert set(pareto.DEFAULT_SENSE) == set(abi.GOF_STATS) | {'spearman'}
    # the rows: a host table through torch, the absolute value where asked
    import torch
    rng = np.random.default_rng(3)
    data = torch.from_numpy(rng.standard_normal((8, 6, 2, 5)))
    rho = torch.from_numpy(rng.standard_normal((6, 2, 5)))
    res = pareto.resolve_objectives([('Bias (%)', 'TP', 1), ('spearman', 'Q', 0), ('NSE', 'SS', 1)], n_reaches=2, has_spearman=True)
    rows = pareto.objective_rows(data, rho, res).numpy()
    assert np.array_equal(rows[0], np.abs(data[4, 4, 1].numpy())) and np.array_equal(rows[1], rho[0, 0].numpy())
    assert np.array_equal(rows[2], data[1, 1, 1].numpy())
