"""How far two evaluations of the Thornthwaite rule (simplyp_amd/forcing.py thornthwaite_rows) may lie apart: the bound the host
tests (against the reference's golden values) and the GPU tests (device against the NumPy statement) share.  Derived from the
rule, the number format (u = 2^-53) and the stated error of each side's pow; evaluated on the expected side's own monthly
values, never on the values under test.

Two evaluations differ in (1) the monthly means they start from, by at most ``dT`` absolute, and (2) their ``x ** y``, by at most
``e_pow(|y ln x|)`` relative; every other operation is an IEEE operation on both sides, rounded within u.  First order in those:

  term   (T_m / 5)^1.514 moves by 1.514 dT / T_m + e_pow relative (+ 2 u: the division by 5 on either side)
  I      a sum of positive terms moves by no more than its terms do, and either side rounds eleven additions:
         dI = sum term (1.514 dT / T_m + e_pow + 2 u) + 22 u I
  a      da = |a'(I)| dI + 8 u (6.75e-7 I^3 + 7.71e-5 I^2 + 1.792e-2 I + 0.49239): at most four roundings of a partial result no
         larger than that sum on either side (the reference's I ** 3 is one pow where the statement has two products)
  PET_m  = C (10 T_m / I)^a:  rel = a (dT / T_m + dI / I + 4 u) + |ln(10 T_m / I)| da + e_pow(|a ln(10 T_m / I)|) + 10 u
         (the last: five products and quotients around the power on either side)
  V_m    = PET_m / N: + 2 u
  daily  a convex combination of two node values: the larger of their bounds, + 8 u max|V| for the roundings of the difference,
         the quotient, the product and the sum on either side.

First order needs dT << T_m; ``monthly`` asserts that no positive mean lies within 10^6 dT of zero and, when dT > 0, that no
mean at all does (a mean that changes sign between the two sides would be 0 on one of them).  A month with T_m <= 0 is exactly 0
on both sides; a year with I = 0 is NaN on both."""

import numpy as np

U = 2.0 ** -53
DT_SUM = 38.0 * U        # x max|T_air|: a left-to-right sum of <= 31 days, (N - 1) u sum|t| / N <= 30 u max|T|, and its division,
#                          u max|T|, against pandas' pairwise sum and division, <= 7 u max|T|


def e_pow_libm(t):
    """exp(y log x) in libm (log within 1 ulp, the product rounded, exp adding its ulp) against libm's pow (within 1 ulp)."""
    return (2.0 * t + 3.0) * U


def e_pow_device(t):
    """sp_exp(y sp_log(x)) against exp(y log x) in libm: either within (1 + 3 t) 2^-52 of the truth -- the bar
    tests/test_gpu_elementary.py pins for the device's, from sp_log < 1 ulp and sp_exp < 1 ulp; libm's are no worse."""
    return 2.0 * (1.0 + 3.0 * t) * 2.0 ** -52


def monthly(t_m, pet_m, dT, e_pow):
    """The absolute bound [M] of PET_m (mm/month) from the expected side's clamped-or-not monthly means ``t_m`` [M] and its
    ``pet_m`` [M]; also returns the largest |y ln x| met."""
    t_m, pet_m = np.asarray(t_m, dtype=np.float64), np.asarray(pet_m, dtype=np.float64)
    pos = t_m > 0.0
    assert (t_m[pos] > 1e6 * dT).all() and (dT == 0.0 or (np.abs(t_m) > 1e6 * dT).all())
    with np.errstate(all='ignore'):
        safe = np.where(pos, t_m, 1.0)
        t1 = np.abs(1.514 * np.log(safe / 5.0))
        term = np.where(pos, (safe / 5.0) ** 1.514, 0.0)
        I = term.reshape(-1, 12).sum(axis=1)
        dI = (term * (1.514 * dT / safe + e_pow(t1) + 2.0 * U)).reshape(-1, 12).sum(axis=1) + 22.0 * U * I
        poly = 6.75e-07 * I ** 3 + 7.71e-05 * I ** 2 + 1.792e-02 * I + 0.49239
        a = 6.75e-07 * I ** 3 - 7.71e-05 * I ** 2 + 1.792e-02 * I + 0.49239
        da = np.abs(3 * 6.75e-07 * I ** 2 - 2 * 7.71e-05 * I + 1.792e-02) * dI + 8.0 * U * poly
        I, dI, a, da = (np.repeat(v, 12) for v in (I, dI, a, da))
        base = np.where(pos, 10.0 * safe / I, 1.0)
        t2 = np.abs(a * np.log(base))
        rel = a * (dT / safe + dI / I + 4.0 * U) + np.abs(np.log(base)) * da + e_pow(t2) + 10.0 * U
    t_max = float(max(t1[pos].max(initial=0.0), t2[pos].max(initial=0.0)))
    return np.where(pos, rel * np.abs(pet_m), 0.0), t_max


def daily(tol_m, pet_m, plan):
    """The absolute bound [D] of the daily values (mm/day) from the monthly one."""
    N = plan['days'].astype(np.float64)
    v = np.abs(np.asarray(pet_m, dtype=np.float64)) / N
    tol_v = tol_m / N + 2.0 * U * v
    j = plan['node'].astype(np.int64)
    j1 = np.minimum(j + 1, plan['months'] - 1)
    with np.errstate(invalid='ignore'):
        return np.maximum(tol_v[j], tol_v[j1]) + 8.0 * U * np.maximum(v[j], v[j1])
