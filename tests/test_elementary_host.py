"""The restatement of the device's fp64 elementary functions (tests/elementary.py) against mpmath, without a GPU: it is the
reference the GPU tests compare the device with bit for bit (exp) and the evidence that the algorithms themselves -- range
reduction, polynomials, reconstruction, Newton steps -- meet the header's contract of < 1 ulp on the argument lists the GPU tests
use.  What only the device can show (the hardware seed, the build's contraction) is left to tests/test_gpu_elementary.py."""

import numpy as np

import elementary as el


def test_vector_fma_is_libm_fma():
    """The restatement's array fma against libm's on operands like the ones it meets: Horner steps, range reductions that
    cancel almost completely, tiny and huge terms, exact cases."""
    rng = np.random.default_rng(5)
    n = 20000
    a = rng.uniform(-2.0, 2.0, n) * 2.0 ** rng.integers(-120, 12, n)
    b = rng.uniform(-2.0, 2.0, n) * 2.0 ** rng.integers(-120, 12, n)
    c = np.concatenate([rng.uniform(-2.0, 2.0, n // 4) * 2.0 ** rng.integers(-120, 12, n // 4),
                        -(a * b)[n // 4:n // 2] * (1.0 + rng.integers(-4, 5, n // 4) * 2.0 ** -52),         # cancellation
                        (a * b)[n // 2:3 * n // 4] * 2.0 ** rng.integers(-60, 60, n // 4).astype(float),   # halfway cases near
                        np.zeros(n // 4)])
    x = el.exp_args()[:4000]
    k = np.rint(x * 1.4426950408889634)
    a, b, c = np.concatenate([a, k]), np.concatenate([b, np.full(len(k), -el.LN2_HI)]), np.concatenate([c, x])
    assert np.array_equal(el.fma(a, b, c), el.libm_fma(a, b, c))


def test_exp_restatement_stays_below_one_ulp():
    x = el.exp_args()
    err = el.ulp_error(el.sp_exp(x), el.exp_truth())
    w, at = el.worst(err, x)
    print('sp_exp restated: worst %.4f ulp at %r' % (w, at))
    assert w < 1.0, (w, at)
    assert el.sp_exp(np.array([0.0]))[0] == 1.0


def test_log_restatement_stays_below_one_ulp():
    x = el.log_args()
    got = el.sp_log(x)
    err = el.ulp_error(got, el.log_truth())
    w, at = el.worst(err, x)
    print('sp_log restated: worst %.4f ulp at %r' % (w, at))
    assert w < 1.0, (w, at)
    assert got[0] == 0.0 and x[0] == 1.0


def test_log_with_a_faithful_reciprocal_stays_below_one_ulp():
    """The device's reciprocal is faithfully, not always correctly, rounded: sp_log with 1/x moved to the neighbour on either
    side (the worst a faithful reciprocal can do) must still meet the bar."""
    x = el.log_args()
    for step in (-np.inf, np.inf):
        err = el.ulp_error(el.sp_log(x, rcp=lambda d: np.nextafter(1.0 / d, step)), el.log_truth())
        w, at = el.worst(err, x)
        print('sp_log restated, reciprocal one ulp towards %s: worst %.4f ulp at %r' % (step, w, at))
        assert w < 1.0, (w, at)


def test_newton_steps_on_a_seed_with_the_hardware_error():
    """Seed = the IEEE reciprocal moved by the recorded hardware error, either sign.  One step: relative error <= e0^2 + 2^-52.
    Two steps: below 1 ulp everywhere (faithful), and correctly rounded on the random arguments."""
    rnd, near = el.rcp_args()
    (t_rnd, t_near) = el.rcp_truth()
    assert np.array_equal(t_rnd[0], 1.0 / rnd) and np.array_equal(t_near[0], 1.0 / near)      # IEEE division is the truth, rounded once
    missed = 0
    for e0 in (el.SEED_ERR, -el.SEED_ERR):
        for x, t, random_set in ((rnd, t_rnd, True), (near, t_near, False)):
            r0 = (1.0 / x) * (1.0 + e0)
            r1 = el.newton(x, r0)
            r2 = el.newton(x, r1)
            assert el.rel_error(r1, t).max() <= e0 * e0 + 2.0 ** -52
            assert el.ulp_error(r2, t).max() < 1.0
            if random_set:
                assert np.array_equal(r2, t[0])
            else:
                missed += int((r2 != t[0]).sum())
    print('two Newton steps next to 1 and 2: %d of %d not correctly rounded' % (missed, 2 * len(near)))
