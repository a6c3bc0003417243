"""The five pieces of the step rule that ck_day and ck_day_quad share, on caller-given arguments (simplyp_eval_units, which = 7:
the same inline functions, not copies) against tests/step_model.py.  Whole runs see these only through rhs_evals agreeing with
the oracle to 0.5 % and through quad == one-lane; neither tells a wrong clamp, a wrong exponent of the second pair or a damping
factor off by a tenth from a legitimate accept / reject flip.  Every bar is the reciprocal's or the fp32 log / exp's own."""

import itertools

import numpy as np
import pytest

import elementary as el
import step_model as sm

pytestmark = pytest.mark.gpu

RCP1_BAR = el.SEED_ERR ** 2 + 2.0 ** -52          # sp_rcp1 (tests/test_gpu_elementary.py::test_reciprocals) and the product behind it
C = sm.C


def up(x):
    return float(np.nextafter(x, np.inf))


def down(x):
    return float(np.nextafter(x, -np.inf))


def test_open_step(engine0):
    """Exact where no reciprocal enters; with the second pair, Z_START / rate within sp_rcp1's bar."""
    cases = [(h, T, rate) for T in (0.5, 1.0, 2.0) for rate in (0.1, 400.0)
             for h in (0.0, -1.0, np.nan, 1.5 * T, up(T / C['CTRL_DAY_START']), 5.0 * T, 25.0 * T, 0.01, 0.3 * T, T, 1e-6)]
    got = engine0.eval_units('step', sm.rows_of(sm.OPEN, cases))
    n_rcp = 0
    for (h, T, rate), g in zip(cases, got):
        for col, (kink, stiff, real) in enumerate([(True, False, np.float64), (True, True, np.float64),
                                                   (False, False, np.float64), (False, False, np.float32)]):
            want, rcp = sm.open_step(h, T, rate, kink, stiff, real)
            if rcp:
                n_rcp += 1
                assert abs(g[col] - want) <= RCP1_BAR * want, (h, T, rate, col, g[col], want)
            else:
                assert g[col] == want, (h, T, rate, col, g[col], want)
        assert 0.0 < g[0] <= T and 0.0 < g[1] <= g[0]
    assert n_rcp >= 20                                   # rate 400: the day opens with 0.3 relaxation times


def test_propose(engine0):
    """Bit for bit, with rem exactly 2 h and exactly 1.1 h (as the device forms that product) and one ulp either side."""
    c11 = 1.1
    cases = []
    for h in (0.1, 0.37, 1.0 / 3.0, 1e-3):
        for rem in (2.0 * h, c11 * h, 1.5 * h, 3.0 * h, 0.5 * h, h):
            cases += [(h, down(rem), c11), (h, rem, c11), (h, up(rem), c11)]
    got = engine0.eval_units('step', sm.rows_of(sm.PROPOSE, cases))[:, 4]
    want = np.array([sm.propose(*c) for c in cases])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), [c for c, g, w in zip(cases, got, want) if g != w][:3]
    h, rem = np.array([c[0] for c in cases]), np.array([c[1] for c in cases])
    kept, halved, all_of_it = got == h, got == 0.5 * rem, got == rem            # the carried size | half of what is left | all of it
    assert (kept & ~all_of_it).sum() >= 8 and (halved & ~kept).sum() >= 8 and (all_of_it & ~kept).sum() >= 8


def test_choose_pair(engine0):
    """The flag and the row offset exactly, the shortened step within sp_rcp1's bar; hh x rate one ulp either side of Z_ON (rate 2:
    the product is exact); every combination of the three flags."""
    z = C['STIFF_Z_ON']
    steps = [(0.5 * z, 2.0), (down(0.5 * z), 2.0), (up(0.5 * z), 2.0), (0.5, 100.0), (0.01, 100.0), (0.3, 437.5)]
    cases = [s + f for s in steps for f in itertools.product((0.0, 1.0), repeat=3)]
    got = engine0.eval_units('step', sm.rows_of(sm.CHOOSE, cases))
    seen = set()
    for (hh, rate, kn, last, alive), g in zip(cases, got):
        want, cut, toff, second = sm.choose_pair(hh, rate, bool(kn), bool(last), bool(alive))
        assert (g[6], g[7]) == (float(toff), float(second)), (hh, rate, kn, last, alive)
        if cut:
            assert abs(g[5] - want) <= RCP1_BAR * want, (hh, rate, g[5], want)
        else:
            assert g[5] == hh
        seen.add((cut, second))
    assert seen == {(False, False), (False, True), (True, False)}


def test_damping(engine0):
    """F = clamp(min(lam T / PHI, 1 + lam left), 1, FMAX), lam = min(rate - b_Q dQr / Qr, rate), through the RAW reciprocal:
    |dF| <= SEED_ERR |b_Q dQr / Qr| max(T / PHI, left) + 4 ulp(F)."""
    cases = []
    for T in (0.5, 1.0, 2.0):
        for left in (0.0, 0.25 * T, 0.9 * T):
            for rate in (5.0, 40.0, 100.0, 450.0):
                for qd in (-0.5, 0.0, 0.3, 0.9, 1.5):          # b_Q dQr / Qr as a share of the rate; > 1: the expansive reach
                    Qr = 0.37
                    cases.append((0.5, Qr, qd * rate * Qr / 0.5, rate, T, left))
    got = engine0.eval_units('step', sm.rows_of(sm.DAMP, cases))[:, 8]
    want = np.array([sm.damping(*c) for c in cases])
    a = np.array(cases)
    bar = el.SEED_ERR * np.abs(a[:, 0] * a[:, 2] / a[:, 1]) * np.maximum(a[:, 4] / C['DAMP_PHI'], a[:, 5]) + 4 * np.spacing(want)
    worst = int(np.argmax(np.abs(got - want) / bar))
    print('ck_damping: worst %.3f of the bar at %r' % (abs(got[worst] - want[worst]) / bar[worst], cases[worst]))
    assert (np.abs(got - want) <= bar).all(), (cases[worst], got[worst], want[worst])
    expansive = a[:, 0] * a[:, 2] / a[:, 1] > a[:, 3]
    assert expansive.any() and (got[expansive] == 1.0).all()                     # lam < 0
    assert (got == C['DAMP_FMAX']).any() and (got <= C['DAMP_FMAX']).all() and (got >= 1.0).all()
    assert ((got > 1.0) & (got < C['DAMP_FMAX'])).sum() >= 10
    assert (got[a[:, 5] == 0.0] == 1.0).all()                                    # nothing left of the day: 1 + lam x 0


def test_step_factor(engine0):
    """SAFETY err**exponent in fp32 through v_log_f32 and v_exp_f32, one ulp each, the product t = exponent log2(err) and the
    safety factor: relative error <= (3 + 2 |t|) 2^-23.  The exponent is -1/4 only for <true> with stiff = 1."""
    errs = np.concatenate([10.0 ** np.linspace(-6, 6, 49), [1.0, 0.999, 1.001, 0.9 ** 5, 2.0 ** -20, 1e-30]])
    errs = errs.astype(np.float32).astype(np.float64)
    cases = [(e, s) for e in errs for s in (0.0, 1.0)]
    got = engine0.eval_units('step', sm.rows_of(sm.FACTOR, cases))
    worst = 0.0
    for (e, s), g in zip(cases, got):
        for col, second in ((9, False), (10, bool(s))):
            want, t = sm.step_factor(e, second)
            bar = (3.0 + 2.0 * abs(t)) * 2.0 ** -23 * want
            worst = max(worst, abs(g[col] - want) / bar)
            assert abs(g[col] - want) <= bar, (e, s, col, g[col], want)
    print('ck_step_factor: worst %.3f of the bar' % worst)
    mid = [i for i, (e, s) in enumerate(cases) if s == 1.0 and 0.01 < e < 100.0 and e != 1.0]
    assert all(got[i, 9] != got[i, 10] for i in mid)                             # the two exponents are told apart
    lo, hi = float(np.float32(C['CTRL_FAC_MIN'])), float(np.float32(C['CTRL_FAC_MAX']))
    edge = engine0.eval_units('step', sm.rows_of(sm.FACTOR, [(0.0, 0.0), (0.0, 1.0), (np.inf, 0.0), (np.inf, 1.0), (1e-40, 1.0)]))
    assert edge[:, 9].tolist() == [hi, hi, lo, lo, hi] and edge[:, 10].tolist() == [hi, hi, lo, lo, hi]
