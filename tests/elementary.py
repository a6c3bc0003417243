"""What the tests of the fp64 elementary functions (simplyp_kernels.hip.h: sp_expn, sp_log, sp_rcp, sp_rcp1) share: the argument
lists, the truth (mpmath at 40 digits, kept as an unevaluated sum of two doubles), the error measure (ulps of the true value), and
a restatement of the functions in IEEE double arithmetic -- numpy for everything that is one rounding, and an fma built from
error-free transformations that is held to libm's.

The restatement of sp_exp is exact: the device function consists of IEEE operations only (multiply, rint, fma, ldexp on a value
that stays normal), so a device result that differs from it in one bit means the build contracted or reordered something.  The
restatement of sp_log puts an IEEE division where the device runs its own reciprocal (hardware seed + two Newton steps)."""

import ctypes
import ctypes.util
import functools

import mpmath
import numpy as np

_libm = ctypes.CDLL(ctypes.util.find_library('m') or 'libm.so.6')
_libm.fma.restype = ctypes.c_double
_libm.fma.argtypes = [ctypes.c_double] * 3

LN2_HI, LN2_LO = 6.93147180369123816490e-01, 1.90821492927058770002e-10      # the header's two-word ln 2
EXP_COEF = [2.08767569878681e-09, 2.505210838544172e-08, 2.755731922398589e-07, 2.7557319223985893e-06, 2.48015873015873e-05,
            1.984126984126984e-04, 1.388888888888889e-03, 8.333333333333333e-03, 4.1666666666666664e-02, 1.6666666666666666e-01,
            0.5, 1.0, 1.0]
LOG_COEF = [1.531383769920937332e-01, 1.818357216161805012e-01, 2.222219843214978396e-01, 2.857142874366239149e-01,
            3.999999999940941908e-01, 6.666666666666735130e-01]
SEED_ERR = 4.6e-8              # relative error of the raw hardware reciprocal as tools/micro/rcp_accuracy.hip records it


def libm_fma(a, b, c):
    """libm's fma, element by element (a microsecond each): the yardstick of `fma` below."""
    return np.array([_libm.fma(x, y, z) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())])


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a                                      # 2^27 + 1 (Veltkamp)
    h = c - (c - a)
    return h, a - h


def fma(a, b, c):
    """round(a b + c) with one rounding, on whole arrays: the exact product as two doubles (Dekker), the exact sum of c and its
    high word (Knuth), the two low words added with rounding to odd, and one last addition (Boldo & Melquiond, "Emulation of a
    FMA and correctly rounded sums", 2008).  No operand here comes near overflow or underflow, where the splitting would fail;
    tests/test_elementary_host.py holds it to libm's fma."""
    a, b, c = (np.asarray(v, dtype=np.float64) for v in np.broadcast_arrays(a, b, c))
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    pe = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    th, tl = _two_sum(c, p)
    v, ve = _two_sum(tl, pe)
    even = (v.view(np.int64) & 1) == 0
    v = np.where((ve != 0.0) & even, np.nextafter(v, np.where(ve > 0.0, np.inf, -np.inf)), v)
    return th + v


def sp_exp(x):
    x = np.asarray(x, dtype=np.float64)
    n = np.rint(x * 1.4426950408889634)
    a = fma(n, -LN2_HI, x)
    a = fma(n, -LN2_LO, a)
    p = np.full_like(x, 1.6059043836821613e-10)
    for c in EXP_COEF:
        p = fma(p, a, c)
    return np.ldexp(p, n.astype(np.int32))


def newton(x, r):
    """One Newton step of the device reciprocals: r + r (1 - x r), two fmas."""
    return fma(fma(-np.asarray(x, dtype=np.float64), r, 1.0), r, r)


def sp_log(x, rcp=lambda d: 1.0 / d):
    x = np.asarray(x, dtype=np.float64)
    m, k = np.frexp(x)                                       # m in [0.5, 1)
    lo = m < 0.70710678118654752440
    m = np.where(lo, m + m, m)
    k = np.where(lo, k - 1, k)
    f = m - 1.0
    s = f * rcp(2.0 + f)
    z = s * s
    R = np.full_like(x, 1.479819860511658591e-01)
    for c in LOG_COEF:
        R = fma(R, z, c)
    R = R * z
    hfsq = 0.5 * f * f
    dk = k.astype(np.float64)
    t = fma(s, hfsq + R, dk * LN2_LO)
    return fma(dk, LN2_HI, f - (hfsq - t))


# ---- truth and the error measure ----

def _truth(fn, args):
    hi, lo = np.empty(len(args)), np.empty(len(args))
    with mpmath.workdps(40):
        for i, a in enumerate(args):
            t = fn(*(mpmath.mpf(float(v)) for v in np.atleast_1d(a)))
            hi[i] = float(t)
            lo[i] = float(t - mpmath.mpf(hi[i]))
    return hi, lo


def ulp_error(got, truth):
    """|got - true| in units in the last place of the TRUE value (2^(e-52) for 2^e <= |true| < 2^(e+1)); where the true value
    is 0, 0 for an exact 0 and inf otherwise."""
    hi, lo = truth
    got = np.asarray(got, dtype=np.float64)
    m, e = np.frexp(np.abs(hi))
    e = e - ((m == 0.5) & (lo * np.sign(hi) < 0.0))          # hi is a power of two and the true value lies just below it
    with np.errstate(invalid='ignore', over='ignore'):
        err = np.abs((got - hi) - lo) / np.ldexp(1.0, e - 53)
    return np.where(hi == 0.0, np.where(got == 0.0, 0.0, np.inf), err)


def rel_error(got, truth):
    hi, lo = truth
    return np.abs((np.asarray(got, dtype=np.float64) - hi) - lo) / np.abs(hi)


def worst(err, args):
    i = int(np.nanargmax(err))
    return float(err[i]), np.atleast_1d(args[i]).tolist()


def _neighbours(centre, n):
    """centre and its n fp64 neighbours on either side (steps in the bit pattern: exact across a power of two)."""
    c = np.atleast_1d(np.asarray(centre, dtype=np.float64))
    bits = c.view(np.int64)[:, None] + np.arange(-n, n + 1, dtype=np.int64)[None, :]
    return bits.view(np.float64).ravel()


# ---- argument lists (deterministic) and their truths, made once per process ----

@functools.lru_cache(maxsize=None)
def exp_args():
    rng = np.random.default_rng(20240)
    ln2 = 0.6931471805599453
    centres = (np.arange(-1000, 1001) + 0.5) * ln2                               # where n = rint(x / ln 2) flips
    x = np.concatenate([[700.0, -700.0, 0.0, 2.0 ** -60, -2.0 ** -60,
                         -700.0],                                                 # what soil_p's fmax(-b, -700) passes for a large b
                        rng.uniform(-700.0, 700.0, 25000), rng.uniform(-8.0, 8.0, 25000), _neighbours(centres, 40)])
    assert np.abs(x).max() <= 700.0
    return x


@functools.lru_cache(maxsize=None)
def log_args():
    rng = np.random.default_rng(20241)
    k = np.arange(1, 53)
    rt = _neighbours(0.70710678118654752440, 2000)
    x = np.concatenate([[1.0, 2.0 ** -53, 1.0 - 2.0 ** -53],
                        10.0 ** rng.uniform(-290.0, 290.0, 30000), rng.uniform(0.5, 2.0, 20000),
                        _neighbours(np.concatenate([1.0 + 2.0 ** -k, 1.0 - 2.0 ** -k]), 25),
                        *[np.ldexp(rt, s) for s in (-1000, -500, 0, 500, 1000)]])
    assert x.min() > 2.0 ** -1022 and np.isfinite(x).all()
    return x


@functools.lru_cache(maxsize=None)
def rcp_args():
    """(random, structured): random mantissas at exponents in +-500; the 2000 mantissas next to 1 and next to 2 at exponents
    -500, 0 and 500."""
    rng = np.random.default_rng(20242)
    rnd = np.ldexp(1.0 + rng.integers(0, 2 ** 52, 50000) * 2.0 ** -52, rng.integers(-500, 501, 50000).astype(np.int32))
    i = np.arange(2000)
    mant = np.concatenate([1.0 + i * 2.0 ** -52, 2.0 - (i + 1) * 2.0 ** -52])
    return rnd, np.concatenate([np.ldexp(mant, s) for s in (-500, 0, 500)])


POW_B = [0.3, 0.5, 1 - 0.5, 1.5, 3.0]


@functools.lru_cache(maxsize=None)
def pow_args():
    rng = np.random.default_rng(20243)
    q = 10.0 ** rng.uniform(-8.0, 4.0, 4000)
    return np.stack([np.tile(q, len(POW_B)), np.repeat(POW_B, len(q))], axis=1)


@functools.lru_cache(maxsize=None)
def exp_truth():
    return _truth(mpmath.exp, exp_args())


@functools.lru_cache(maxsize=None)
def log_truth():
    return _truth(mpmath.log, log_args())


@functools.lru_cache(maxsize=None)
def rcp_truth():
    return tuple(_truth(lambda x: 1 / x, a) for a in rcp_args())


@functools.lru_cache(maxsize=None)
def pow_truth():
    return _truth(lambda q, b: mpmath.power(q, b), pow_args())
