"""The host rules the table reductions share (simplyp_amd/csrc/simplyp_table.h: table view, series ids, probabilities and
numpy's 'linear' ranks, period day lists, the prior box), exercised on the CPU: tests/table_host_main.cpp includes the
header, is built once per session with the host compiler under AddressSanitizer and UBSan, and runs as a child process that
reads cases as text.  No GPU needed; the same rules are what the GPU tests of every entry reject bad arguments through."""


import numpy as np
import pytest

from simplyp_amd import abi, marshal

import host_program
from host_program import rejected

COL = {c: i for i, c in enumerate(marshal.OUT_COLUMNS)}
FLUX = ['Qr', 'Msus_kg/day', 'TDP_kg/day', 'PP_kg/day']
LEGAL = (1 << 26) - 1                   # SIMPLYP_MASK_ALL | SIMPLYP_MASK_D_SNOW
DERIVED = [abi.TQ_DERIVED + v for v in range(6)]


@pytest.fixture(scope='session')
def driver():
    return host_program.case_runner(host_program.build('table_host_main.cpp'), timeout=120)


def arr(a):
    return 'null' if a is None else ' '.join([str(len(a))] + [x.hex() if isinstance(x, float) else str(int(x)) for x in a])


def ints(text):
    return [int(x) for x in text.split()]


def lists(text):
    """'n a b c m d e' -> [[a, b, c], [d, e]]"""
    v, out = ints(text), []
    while v:
        out.append(v[1:1 + v[0]])
        v = v[1 + v[0]:]
    return out


def test_linear_ranks_equal_numpy_fp64(driver):
    qs = np.concatenate([[0.0, 1e-300, 0.25, 0.5, 1.0 - 2.0 ** -53, 1.0], np.random.default_rng(11).uniform(0, 1, 50)])
    ns = [1, 2, 3, 64, 65, 10957]
    got = driver(['ranks %s %d' % (float(q).hex(), n) for n in ns for q in qs])
    for i, n in enumerate(ns):
        h = qs * np.float64(n - 1)
        k_lo = np.floor(h).astype(np.int64)
        k_hi = np.minimum(k_lo + 1, n - 1)
        for j in range(len(qs)):
            rc, rest = got[i * len(qs) + j]
            assert rc == 0 and ints(rest) == [k_lo[j], k_hi[j]], (n, qs[j], rest)


def test_probabilities(driver):
    probs = lambda q, K=None, max_K=16: 'probs %d %d %s' % (max_K, len(q) if K is None else K, arr(q))
    rejected(driver([probs([]), probs([0.5] * 17), probs([-1e-9]), probs([1.0 + 1e-9]), probs([0.5, float('nan')]),
                     probs(None, K=1)]))
    assert [rc for rc, _ in driver([probs([0.0]), probs([1.0]), probs([0.0, 1.0, 0.5]), probs([0.5] * 16)])] == [0] * 4


def test_table_view(driver):
    E, S, D = 130, 5, 40
    view = lambda mask=marshal.MASK_REACH5, n=S, reaches=None, legal=LEGAL: 'view %d %d %d %d %d %d %s' % (E, S, D, mask, legal, n, arr(reaches))
    ok = driver([view(), view(n=2, reaches=[4, 0]), view(n=S, reaches=[4, 3, 2, 1, 0]), view(n=99)])
    assert [rc for rc, _ in ok] == [0] * 4
    assert ints(ok[0][1]) == [E, S, D, S, S] + list(range(S))              # out_reaches = NULL: the identity over S
    assert ints(ok[1][1]) == [E, S, D, 2, 2, 4, 0]
    assert ints(ok[2][1]) == [E, S, D, S, S, 4, 3, 2, 1, 0]
    assert ints(ok[3][1]) == [E, S, D, S, S] + list(range(S))              # without a list n_out_reaches is not read
    rejected(driver([view(n=2, reaches=[0, S]), view(n=2, reaches=[-1, 0]), view(n=0, reaches=[0]),
                     view(n=S + 1, reaches=list(range(S)) + [0]), view(mask=marshal.MASK_REACH5 | (1 << 26)), view(mask=0),
                     view(mask=1 << 11, legal=(1 << 11) - 1)]))


def test_flux_slots_are_popcounts(driver):
    no_msus = marshal.mask_of_columns(['Vr', 'Qr', 'TDP_kg/day', 'PP_kg/day'])
    wb_all = (1 << len(abi.WB_COLUMNS)) - 1
    wb_cols = [abi.WB_COLUMNS.index(c) for c in ('Q_cumecs', 'Msus_kg/day', 'TDP_kg/day', 'PP_kg/day')]
    masks = [(marshal.MASK_REACH5, 0), (no_msus, 0), (marshal.MASK_ALL, 0), (wb_all, 1), (wb_all & ~(1 << wb_cols[2]), 1)]
    got = driver(['slots %d %d' % m for m in masks])
    for (mask, wb), (rc, rest) in zip(masks, got):
        cols = wb_cols if wb else [COL[c] for c in FLUX]
        want = [bin(mask & ((1 << c) - 1)).count('1') for c in cols]
        assert rc == 0 and ints(rest) == [int(all((mask >> c) & 1 for c in cols))] + want, (mask, rest)
    assert ints(got[0][1])[0] == 1 and ints(got[1][1])[0] == 0 and ints(got[4][1])[0] == 0


def test_series(driver):
    mask = marshal.MASK_REACH5
    no_msus = marshal.mask_of_columns(['Vr', 'Qr', 'TDP_kg/day', 'PP_kg/day'])

    def series(ids, mask=mask, R=2, f=1, rp=1, n=None, max_series=32):
        return 'series %d %d %d %d %d %d %s' % (max_series, mask, R, f, rp, (0 if ids is None else len(ids)) if n is None else n, arr(ids))
    rejected(driver([series([COL['VsA']]), series([abi.TQ_DERIVED + 6]), series([40]), series([-1]),
                     series([DERIVED[0]], mask=no_msus), series([DERIVED[1]], mask=mask & ~(1 << COL['Qr'])),
                     series([DERIVED[5]], f=0), series([DERIVED[0]], rp=0),
                     series([], n=0), series([COL['Qr']] * 33), series(None, n=1),
                     series([COL['Qr']] * 32, R=2048)]))                    # n_series * R = 65536
    ids = [COL['Vr'], COL['PP_kg/day']] + DERIVED
    got = driver([series(ids), series([COL['Qr']] * 32, R=2047), series([COL['Qr']])] + [series([d]) for d in DERIVED])
    assert [rc for rc, _ in got] == [0] * len(got)
    slot = lambda c: bin(mask & ((1 << COL[c]) - 1)).count('1')
    loads = [1, 2, 2, 2, 3, 2]                                             # Q_cumecs, SS, TDP, PP, TP (three fluxes), SRP
    head, code, raw = ints(got[0][1])[:2], *lists(got[0][1].split(' ', 2)[2])
    assert head == [1, 2 + sum(loads)] and code == [slot('Vr'), slot('PP_kg/day')] + [-1 - v for v in range(6)] and raw == ids
    assert ints(got[1][1])[:2] == [0, 32] and ints(got[2][1]) == [0, 1, 1, slot('Qr'), 1, COL['Qr']]
    for v in range(6):
        assert ints(got[3 + v][1]) == [1, loads[v], 1, -1 - v, 1, DERIVED[v]], v


def test_period_day_lists(driver):
    D = 40
    periods = lambda pod, P, D_=D: 'periods %d %d %s' % (D_, P, arr(None if pod is None else np.asarray(pod, dtype=np.int64)))
    rejected(driver([periods(np.r_[np.ones(20), np.zeros(20)], 2),                                          # decreasing
                     periods(np.r_[np.zeros(10), np.full(5, -1), np.ones(20), np.zeros(5)], 2),             # ... after a gap
                     periods(np.full(D, 2), 2), periods(np.full(D, -2), 2)]))                               # outside [-1, P)
    pod = np.r_[np.full(3, -1), np.zeros(7), np.full(4, -1), np.zeros(2), np.full(10, 2), -1, np.full(13, 3)].astype(np.int64)
    P = 5                                                                   # period 1 is empty, period 4 is past the last named
    got = driver([periods(pod, P), periods(None, 1), periods(None, 1, D_=0), periods(np.full(D, -1), 2)])
    assert [rc for rc, _ in got] == [0] * 4
    days, day_ptr = lists(got[0][1])
    assert days == list(np.flatnonzero(pod >= 0)) and day_ptr == list(np.r_[0, np.cumsum(np.bincount(pod[pod >= 0], minlength=P))])
    assert lists(got[1][1]) == [list(range(D)), [0, D]] and lists(got[2][1]) == [[], [0, 0]] and lists(got[3][1]) == [[], [0, 0, 0]]


def test_prior_box(driver):
    NP_M, NONE, F_TDP = len(marshal.PM_NAMES), abi.MCMC_TARGET_NONE, abi.MCMC_TARGET_F_TDP

    def box(lo, hi, target, mp=1, f=1):
        return 'box %d %d %d %s %s %s' % (len(lo), mp, f, arr([float(x) for x in lo]), arr([float(x) for x in hi]), arr(target))
    rejected(driver([box([0, 1], [1, 1], [0, 1]), box([0, float('nan')], [1, 2], [0, 1]), box([0, 0], [float('nan'), 1], [0, 1]),
                     box([0], [1], [-3]), box([0], [1], [NP_M]), box([0, 0, 0], [1, 1, 1], [2, NONE, 2]),
                     box([0, 0], [1, 1], [F_TDP, F_TDP]), box([0], [1], [3], mp=0), box([0], [1], [F_TDP], f=0)]))
    got = driver([box([0, -5, 2], [1, 5, 2.5], [NONE, 4, NONE]), box([0, 0], [1, 1], [F_TDP, NP_M - 1]),
                  box([0, 0], [1, 1], [NONE, NONE], mp=0, f=0), box([0], [1], [F_TDP], mp=0), box([0], [1], [0], f=0)])
    assert [rc for rc, _ in got] == [0] * 5
    assert all(set(ints(rest)) == {1} for _, rest in got)                   # lo, hi and target arrive in the argument arrays
