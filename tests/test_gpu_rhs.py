"""The device's four statements of the model's right-hand side -- rhs (the literal form), SysAug::f, quad_rhs, SysAugF::f, the very
inline functions the time-stepping kernels call, on a DayConst assembled by the functions run_slot assembles it with
(simplyp_eval_units, which = 6) -- point by point against the plain statement of tests/rhs_model.py (mpmath, 40 digits), on the
rows tests/test_rhs_host.py holds the CPU oracle to: the 96 fixture rows, the knees of the three gates, a dry and a flooding
reach, no forcing and a storm, upstream inputs, the three NC types.

The bound, for every component i:   |got_i - want_i| <= K u M_i + G_i   (rhs_model.py: M_i the sum of the absolute values of the
component's additive terms, Qr**b terms amplified by 1 + |b ln Qr|; G_i what one ulp of 100 in a gate's argument can change).

K = 64, counted, not fitted.  The longest chain is the TDP balance dz[5] of SysAug::f:
    the gate's flow factor  w = fma(Vs, 1/T_s, -fc/T_s)                     3 roundings (1/T_s, -fc/T_s, the fma)
    the cubic               (s s) fma(-2, s, 3), times w                    3   (s itself: G_i)
    Qg                      fma(gate, ug, Qg_min) with ug = fma(Vg, 1/T_g, -Qg_min): 1/T_g, ug, the gate's cubic 3, the fma    6
    the per-day constants   tA = omb wA conc_A (+ tNC): omb, wA 2, two products, the sum; tNC 4; tg 1; tconst 6       ~ 8 on a path
    the balance             three nested FMAs and the subtraction           4
    kap = pbc invKvc, oT    invKvc 3 (Kv, 1/Kv, / cQ with cQ's own 3), kap, oT       ~ 8
which is about 25 on one path through the expression, each at most one ulp (2 u) of a partial result that is no larger than M_i;
with the terms that run in parallel (three sources, each with its constants) 64 u M_i has a factor ~ 2 in hand.  The auxiliary
states are made on the device by sp_log / sp_expn (< 1 ulp each, tests/test_gpu_elementary.py); what the error of exp(b ln Qr)
does to a term is inside M_i.  One caveat of the count, stated so that a miss is read correctly: the fused flow factor w carries a
rounding of fc / T_s, which inside the gate's zone is up to 100 / s times |w| itself, not "a partial result no larger than M_i";
on the rows here that rounding stays below G_i + K u M_i because G_i, the same order (one ulp of 100 in s moves Qs by
6 (1 - s) / (3 - 2 s) 2^-46 of itself), is granted on top.  It is what the fused forms' worst case is made of: a soil box inside its
zone on a day without forcing, where M_i of dVs is |Qs| alone.

Measured worst ratios on an MI355X, in units of u M_i beyond G_i (each test prints them per component):
rhs 2.53 (dTDPr), SysAug::f and quad_rhs 45.88 (dVsA, no forcing, VsA inside the zone; dVg 29.1, dTDPr 11.6, at most 5.1 in
the reach's other components), SysAugF::f 2.55 of its u = 2^-24 (dES)."""

import numpy as np
import pytest

import rhs_model as rm

pytestmark = pytest.mark.gpu

COLS = {'literal': (0, rm.LITERAL), 'aug': (12, rm.AUG_CQ), 'aug_quad_aux': (47, rm.AUG_CQ), 'f32': (62, rm.AUG)}
QUAD0 = 31
QUAD_NAMES = [n for lane in rm.QUAD for n in lane]


@pytest.fixture(scope='module')
def dev(engine0):
    """The device's 77 columns on the fp64 rows and on the rows rounded to fp32: two calls, shared by every test here."""
    return engine0.eval_units('rhs', rm.rows()[0]), engine0.eval_units('rhs', rm.rows_f32()[0])


def _held(got, names, truth, u, labels, what):
    r = truth.ratios(got, names, u)
    w = rm.worst(r, names, labels)
    print('%s: worst %.2f u M beyond the gate allowance, in %s at %s (K = %d)' % ((what,) + w + (rm.K,)))
    for c, k in enumerate(names):
        if k is not None:
            print('    %-8s %.2f' % (k, float(np.nanmax(r[:, c]))))
    assert w[0] <= rm.K, (what,) + w


def test_literal_form(dev):
    _held(dev[0][:, 0:12], rm.LITERAL, rm.truth(), rm.U64, rm.rows()[1], 'rhs')


def test_augmented_form(dev):
    _held(dev[0][:, 12:27], rm.AUG_CQ, rm.truth(), rm.U64, rm.rows()[1], 'SysAug::f')
    # the auxiliary states it was given: exp(-mu Vs) within sp_exp's ulp and the rounding of its argument, mu Vs ~ 4.6
    R = rm.rows()[0]
    for col, slot in ((27, 0), (28, 1)):
        want = np.exp(-R[:, 8 + rm.IX['mu']] * R[:, slot])
        assert np.all(np.abs(dev[0][:, col] - want) <= 16 * rm.U64 * want)


def test_four_lane_form(dev):
    _held(dev[0][:, QUAD0:QUAD0 + 16], QUAD_NAMES, rm.truth(), rm.U64, rm.rows()[1], 'quad_rhs')
    assert np.all(dev[0][:, QUAD0 + 14] == 0.0)                  # the reach lane's empty third slot


def test_fp32_form(dev):
    _held(dev[1][:, 62:77], rm.AUG, rm.truth_f32(), rm.U32, rm.rows_f32()[1], 'SysAugF::f')


def test_four_lane_form_is_the_augmented_form_bit_for_bit(dev):
    """quad_rhs == SysAug::f on the auxiliary states the quad's lanes formed, as uint64 (the sign of zero included); and those
    auxiliary states -- one sp_exp per lane -- are the bits of the one-lane kernels' group of four."""
    out = np.ascontiguousarray(dev[0])
    aug = out[:, 47:62].copy().view(np.uint64)
    quad = out[:, QUAD0:QUAD0 + 16].copy().view(np.uint64)
    for c, k in enumerate(QUAD_NAMES):
        if k is None:
            continue
        bad = np.flatnonzero(quad[:, c] != aug[:, rm.AUG_CQ.index(k)])
        assert len(bad) == 0, (k, len(bad), rm.rows()[1][bad[0]])
    first = out[:, 12:27].copy().view(np.uint64)
    assert np.array_equal(first, aug)


def test_daily_integrands_of_the_literal_and_the_augmented_form_agree(dev):
    """On rows whose Vr lies on its invariant Qr / Vr is the same number either way: the two forms' q[4] differ by no more than
    the bound of the augmented form's integrand (the larger of the two: it carries Qr**b_Q)."""
    R, labels, inv, _ = rm.rows()
    T = rm.truth()
    rows = np.flatnonzero(inv)
    worst = 0.0
    for c, k in enumerate(['Qr', 'oM_i', 'oT_i', 'oP_i']):
        lit, aug = dev[0][rows, 8 + c], dev[0][rows, 23 + c]
        bar = np.array([rm.K * rm.U64 * float(T.M[k][i]) for i in rows])
        with np.errstate(invalid='ignore', divide='ignore'):
            ratio = np.where(bar > 0, np.abs(lit - aug) / np.where(bar > 0, bar, 1.0), np.where(lit == aug, 0.0, np.inf))
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 1.0).all(), (k, labels[rows[int(np.argmax(ratio))]], float(ratio.max()))
    print('q[4], literal against augmented on %d invariant rows: worst %.3f of the bound' % (len(rows), worst))


def test_gates_are_exactly_closed_below_their_zone(dev):
    """No forcing, both soil boxes and the groundwater store below their thresholds: Qs == 0, so dVs == 0, and Qg == Qg_min bit
    for bit, so dVg == -Qg_min -- in every form."""
    R, labels, _, below = rm.rows()
    rows = np.flatnonzero(below)
    assert len(rows) == 12
    qg = R[rows, 8 + rm.IX['Qg_min']]
    for what, (c0, names) in COLS.items():
        out, q = (dev[1], rm.rows_f32()[0][rows, 8 + rm.IX['Qg_min']]) if what == 'f32' else (dev[0], qg)
        assert np.all(out[rows, c0 + names.index('dVsA')] == 0.0), what
        assert np.all(out[rows, c0 + names.index('dVsS')] == 0.0), what
        assert np.array_equal((-out[rows, c0 + names.index('dVg')]).view(np.uint64), q.view(np.uint64)), what
    assert np.all(dev[0][rows, QUAD0] == 0.0) and np.all(dev[0][rows, QUAD0 + 4] == 0.0)
    assert np.array_equal((-dev[0][rows, QUAD0 + 8]).view(np.uint64), qg.view(np.uint64))


def test_non_finite_inputs_give_non_finite_outputs(engine0):
    R = rm.rows()[0]
    a, b = R[0].copy(), R[0].copy()
    a[8 + rm.IX['T_s_A']] = np.nan
    b[0] = np.inf
    out = engine0.eval_units('rhs', np.stack([a, b, R[0]]))
    for row in (0, 1):
        for what, (c0, names) in COLS.items():
            assert not np.isfinite(out[row, c0 + names.index('dVsA')]), (row, what)
        assert not np.isfinite(out[row, QUAD0])
    assert np.isfinite(out[2]).all()                               # and the call went on to the row behind them
