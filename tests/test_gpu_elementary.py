"""The device's fp64 elementary functions -- sp_expn / sp_exp / sp_exp2, sp_log, sp_rcp, sp_rcp1 of simplyp_kernels.hip.h, the
very inline functions every kernel calls, through simplyp_eval_units -- on chosen arguments against mpmath (40 digits, rounded
once), the error in ulps of the true value.  Every bar is the header's contract or derived in the test; none is fitted to what
the device returned.  The argument lists and the restatement the device is compared with bit for bit are tests/elementary.py,
checked without a GPU by tests/test_elementary_host.py.  Each test prints its worst case: DESIGN.md section "Arithmetic
contracts" records them."""

import numpy as np
import pytest

import elementary as el

pytestmark = pytest.mark.gpu


def test_exp_is_the_restatement_in_every_slot_and_below_one_ulp(engine0):
    x = el.exp_args()
    got = engine0.eval_units('exp', x[:, None])
    assert got.shape == (len(x), 4)
    # alone, slot 1 of two, slots 0 and 6 of seven: the header's claim that a value depends on neither its slot nor its group
    for k in range(1, 4):
        assert np.array_equal(got[:, k], got[:, 0]), k
    # IEEE operations only: any difference from the restatement is a contracted or reordered operation
    want = el.sp_exp(x)
    diff = np.flatnonzero(got[:, 0] != want)
    assert len(diff) == 0, (len(diff), x[diff[:5]].tolist())
    err = el.ulp_error(got[:, 0], el.exp_truth())
    w, at = el.worst(err, x)
    print('sp_exp: worst %.4f ulp at x = %r' % (w, at[0]))
    assert w < 1.0, (w, at)
    assert got[x == 0.0, 0].tolist() == [1.0]


def test_log_stays_below_one_ulp(engine0):
    x = el.log_args()
    got = engine0.eval_units('log', x[:, None])[:, 0]
    err = el.ulp_error(got, el.log_truth())
    w, at = el.worst(err, x)
    print('sp_log: worst %.4f ulp at x = %r; %d of %d differ from the restatement with an IEEE division'
          % (w, at[0], int((got != el.sp_log(x)).sum()), len(x)))
    assert w < 1.0, (w, at)
    assert x[0] == 1.0 and got[0] == 0.0 and not np.signbit(got[0])


def test_reciprocals(engine0):
    """Column 0: the raw hardware seed; 1: one Newton step (sp_rcp1); 2: two (sp_rcp).
    Two steps leave about e0^4 before the last rounding, so sp_rcp is correctly rounded unless the exact reciprocal lies within
    that of a rounding boundary: never on random mantissas, possibly next to 2 (reciprocals just above 1/2, where the spacing of
    the result halves); everywhere it is faithful (< 1 ulp)."""
    rnd, near = el.rcp_args()
    t_rnd, t_near = el.rcp_truth()
    g_rnd, g_near = engine0.eval_units('rcp', rnd[:, None]), engine0.eval_units('rcp', near[:, None])
    e0 = max(float(el.rel_error(g_rnd[:, 0], t_rnd).max()), float(el.rel_error(g_near[:, 0], t_near).max()))
    print('raw seed: worst relative error %.4e' % e0)
    assert e0 <= el.SEED_ERR
    for x, g, t in ((rnd, g_rnd, t_rnd), (near, g_near, t_near)):
        e1 = el.rel_error(g[:, 1], t)
        w1, at1 = el.worst(e1, x)
        print('sp_rcp1: worst relative error %.4e at x = %r (bar %.4e)' % (w1, at1[0], e0 * e0 + 2.0 ** -52))
        assert w1 <= e0 * e0 + 2.0 ** -52
        w2, at2 = el.worst(el.ulp_error(g[:, 2], t), x)
        print('sp_rcp: worst %.4f ulp (0.5 + %.2e) at x = %r' % (w2, w2 - 0.5, at2[0]))
        assert w2 < 1.0, (w2, at2)
    assert np.array_equal(g_rnd[:, 2], t_rnd[0])                                 # correctly rounded on the random set
    miss = np.flatnonzero(g_near[:, 2] != t_near[0])
    m, e = np.frexp(near[miss])
    print('sp_rcp next to 1 and 2: %d of %d not correctly rounded; mantissas as 2 - i 2^-52 with (i, exponent): %r'
          % (len(miss), len(near), [(int(round((2.0 - 2.0 * a) * 2.0 ** 52)), int(b) - 1) for a, b in zip(m, e)]))
    assert (2.0 * m > 1.5).all()                                                 # none next to 1


def test_pow_as_the_right_hand_side_forms_it(engine0):
    """q**b = sp_exp(b sp_log(q)).  The exponential's argument t = b ln q carries sp_log's error (< 1 ulp of ln q: at most
    2^-52 relative) and the product's rounding (2^-53 relative): |dt| <= 1.5 |t| 2^-52, for which the bar grants 3 |t| 2^-52.  An
    absolute error of the argument is a relative error of the result, and sp_exp adds its own ulp (2^-52 relative at most):
    relative error <= (1 + 3 |b ln q|) 2^-52.  Derived, not fitted."""
    a = el.pow_args()
    got = engine0.eval_units('pow', a)[:, 0]
    rel = el.rel_error(got, el.pow_truth())
    bar = (1.0 + 3.0 * np.abs(a[:, 1] * np.log(a[:, 0]))) * 2.0 ** -52
    i = int(np.argmax(rel / bar))
    print('pow: worst %.3f of the bar (relative error %.3e, bar %.3e) at q = %r, b = %r' % (rel[i] / bar[i], rel[i], bar[i], float(a[i, 0]), float(a[i, 1])))
    assert (rel <= bar).all(), (a[i].tolist(), rel[i], bar[i])


def test_unknown_function_is_an_argument_error(engine0):
    import torch
    from simplyp_amd import engine
    L = engine.lib()
    t = torch.ones(4, dtype=torch.float64, device=engine0.tdev)
    for which in (-1, 8):
        assert L.simplyp_eval_units(engine0._h, which, 1, t.data_ptr(), t.data_ptr()) == -1
