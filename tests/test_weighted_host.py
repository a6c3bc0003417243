"""The integer rules of the weighted bands (simplyp_amd/csrc/simplyp_weighted.h: the exact threshold, the reference selection
of a row, the weighted entries' argument checks), exercised on the CPU: tests/weighted_host_main.cpp includes the header, is
built once per session with the host compiler under AddressSanitizer and UBSan, and runs as a child process that reads cases as
text.  The header is compared with simplyp_amd/weighted.py's statement in Python integers, and that with numpy's
``method='inverted_cdf'`` where numpy's floating-point CDF cannot round.  No GPU needed."""

from fractions import Fraction

import numpy as np
import pytest

from simplyp_amd import weighted

import host_program
import weighted_cases as wc
from host_program import rejected


@pytest.fixture(scope='session')
def driver():
    return host_program.case_runner(host_program.build('weighted_host_main.cpp'), timeout=120)


def test_threshold_is_exact(driver):
    Ts = [1, 2, 3, 1 << 40, (1 << 53) + 1, 1 << 62]
    ps = [0.0, 5e-324, 2.0 ** -60, 0.025, 0.5, 1.0 - 2.0 ** -53, 1.0]
    cases = [(p, T) for T in Ts for p in ps]
    # p = c / T for a power-of-two T: the product is an integer and the ceiling must not move it
    for T in (2, 1 << 40, 1 << 62):
        for c in (1, 2, T // 2 - 1 if T > 4 else 1, T // 2, T - 1, T):
            if c < 1 << 53 or c % (T >> 52) == 0:                       # c / T is then a float
                cases.append((c / T, T))
                assert Fraction(c / T) * T == c
    rng = np.random.default_rng(5)
    cases += [(float(p), int(T)) for p, T in zip(rng.uniform(0, 1, 200), rng.integers(1, 1 << 62, 200))]
    got = driver(['thr %s %d' % (float(p).hex(), T) for p, T in cases])
    for (p, T), (rc, rest) in zip(cases, got):
        x = Fraction(p) * T
        want = max(1, -((-x.numerator) // x.denominator))
        assert rc == 0 and int(rest) == want == weighted.threshold(p, T), (p, T, rest, want)
    assert weighted.threshold(0.5, 0) == 1 and driver(['thr %s 0' % 0.5.hex()])[0] == (0, '1')


def row_case(p, x, q, inc=None):
    return 'row %s %d %s %d %s %s' % (float(p).hex(), len(x), ' '.join(float(v).hex() for v in x), len(q), ' '.join(str(int(v)) for v in q),
                                      'null' if inc is None else '%d %s' % (len(inc), ' '.join(str(int(v)) for v in inc)))


def test_row_selection_equals_the_python_statement(driver):
    rng = np.random.default_rng(17)
    cases = []
    for E in (1, 2, 7, 64, 200):
        for vp in wc.VALUE_PATTERNS:
            x = wc.values(vp, (E,), rng)
            for wp in wc.WEIGHT_PATTERNS:
                q = wc.weights(wp, E, rng)
                inc = None if (E + len(cases)) % 3 else rng.random(E) < 0.7
                for p in wc.PROBS + [float(rng.uniform())]:
                    cases.append((p, x, q, inc))
    got = driver([row_case(*c) for c in cases])
    for (p, x, q, inc), (rc, rest) in zip(cases, got):
        bits, T = (int(v) for v in rest.split())
        value = np.array([bits], dtype=np.uint64).view(np.float64)
        want = weighted.quantile_row(x, q, p, include=inc)
        take = (q > 0) if inc is None else (q > 0) & inc
        assert rc == 0 and T == sum(int(v) for v in q[take]), (p, T)
        assert wc.same_bits(value, [want]), (p, x, q, inc, value, want)
        assert wc.same_bits(weighted.quantiles(x[None, :], q, [p], include=inc)[0], [want])
        assert T > 0 or np.isnan(want)                                   # nobody takes part: NaN
        assert np.isnan(want) or want in x[take]                         # otherwise an element of the row


def test_python_statement_equals_numpy_inverted_cdf():
    rng = np.random.default_rng(23)
    n = 0
    for E in (1, 2, 7, 64, 200):
        for vp in ('ties', 'normals'):
            x = wc.values(vp, (3, E), rng)
            q = rng.integers(0, (1 << 20) + 1, E).astype(np.uint64)      # numpy's float sums are exact
            q[rng.random(E) < 0.3] = 0
            if not (q > 0).any():
                q[0] = 5
            take = q > 0
            for r in range(3):
                order = np.argsort(x[r][take], kind='stable')
                C = np.cumsum(q[take][order].astype(np.int64))
                probs = (C - 0.5) / float(C[-1])                           # the mid-points: no rounding can matter
                got = weighted.quantiles(x[r], q, probs)
                want = np.quantile(x[r][take], probs, weights=q[take].astype(np.float64), method='inverted_cdf')
                assert wc.same_bits(got, want), (E, vp, r)
                n += len(probs)
    assert n > 1000


def test_linear_weights():
    w = np.array([3.0, 0.0, 3.0 * 2.0 ** -41, 3.0 * 2.0 ** -40, 1.5, 1.0])
    q = weighted.linear_weights(w)
    assert q.dtype == np.uint64
    assert [int(v) for v in q] == [1 << 40, 0, 0, 1, 1 << 39, (1 << 40) // 3]
    assert int(weighted.linear_weights([7.5])[0]) == 1 << 40
    for bad in ([1.0, -1e-300], [1.0, np.nan], [np.inf, 1.0], [0.0, 0.0], [], [[1.0, 2.0]]):
        with pytest.raises(ValueError):
            weighted.linear_weights(bad)
    with pytest.raises(ValueError):
        weighted.quantile_row([1.0, 2.0], [1, (1 << 40) + 1], 0.5)
    with pytest.raises(ValueError):
        weighted.threshold(1.5, 3)


def test_argument_checks(driver):
    check = lambda E=10, n_rows=3, table=1, weights=1, order=1, K=None, q=(0.5,): 'check %d %d %d %d %d %d %s' % (
        E, n_rows, table, weights, order, (0 if q is None else len(q)) if K is None else K,
        'null' if q is None else '%d %s' % (len(q), ' '.join(float(v).hex() for v in q)))
    ok = driver([check(), check(E=1, n_rows=0), check(E=1 << 22), check(q=[0.0, 1.0] * 8)])
    assert [rc for rc, _ in ok] == [0] * 4
    rejected(driver([check(E=0), check(E=(1 << 22) + 1), check(n_rows=-1), check(table=0), check(weights=0), check(order=0),
                     check(q=None, K=1), check(q=[], K=0), check(q=[0.5] * 17), check(q=[1.5]), check(q=[float('nan')]),
                     check(q=[-1e-9]), 'bad 1']))
    assert driver(['bad 0'])[0][0] == 0
