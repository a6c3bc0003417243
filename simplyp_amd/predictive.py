"""NumPy mirror of the device random stream behind the predictive bands (csrc/simplyp_predictive.hip.h).  CPU only.

The reference's overall predictive band (Development/2016/MCMC.ipynb, get_uncertainty_intervals) adds
``norm.rvs(loc=0, scale=m*sim)`` to every member's series before the percentiles are taken.  On the device that draw is
counter-based: a pure function of (seed, member, absolute day, model reach, series id) and of nothing else -- not of the
launch shape, the slot a member sits in, the chunking, the window or the time of day.

* generator: Philox4x32-10 (Salmon et al., SC'11), multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85;
* key = (seed & 0xffffffff, seed >> 32); counter = (member, day0 + d, zero-based model reach, series id as passed to the C ABI);
* outputs x0..x3: h1 = ((x0 << 32) | x1) >> 12, u1 = (h1 + 0.5) 2^-52, h2 / u2 from x2, x3 alike: exact in fp64, u in (0, 1);
* z = sqrt(-2 ln u1) cospi(2 u2): one normal per call, |z| <= 8.58;
* error model: v' = v + (m v) z -- two multiplies and an add, no fma.

The integers match the device bit for bit.  z differs from the device's by the roundings of log, sqrt and cospi only
(tests/test_gpu_predictive.py bounds it by 2^-45).
"""

import numpy as np

PHILOX_M0 = np.uint64(0xD2511F53)
PHILOX_M1 = np.uint64(0xCD9E8D57)
PHILOX_W0 = np.uint32(0x9E3779B9)
PHILOX_W1 = np.uint32(0xBB67AE85)
_LO32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _u32(a):
    """Any integer array-like (Python ints up to 2^32 - 1 included) as uint32."""
    return (np.asarray(a, dtype=np.uint64) & _LO32).astype(np.uint32)


def philox4x32_10(counter, key):
    """Philox4x32 with 10 rounds.  counter: four uint32 arrays (broadcast against each other), key: two.  Returns the four
    uint32 output arrays."""
    c = [np.asarray(x) for x in np.broadcast_arrays(*[_u32(x) for x in counter])]
    k0, k1 = _u32(key[0]), _u32(key[1])
    for r in range(10):
        if r:                                              # the key schedule wraps at 2^32
            k0 = _u32(k0.astype(np.uint64) + np.uint64(PHILOX_W0))
            k1 = _u32(k1.astype(np.uint64) + np.uint64(PHILOX_W1))
        p0 = PHILOX_M0 * c[0].astype(np.uint64)
        p1 = PHILOX_M1 * c[2].astype(np.uint64)
        hi0, lo0 = (p0 >> _S32).astype(np.uint32), (p0 & _LO32).astype(np.uint32)
        hi1, lo1 = (p1 >> _S32).astype(np.uint32), (p1 & _LO32).astype(np.uint32)
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
    return tuple(c)


def _uniform(hi, lo):
    h = ((hi.astype(np.uint64) << _S32) | lo.astype(np.uint64)) >> np.uint64(12)
    return (h.astype(np.float64) + 0.5) * 2.0 ** -52


def _cospi(t):
    """cos(pi t) for t in (0, 2) with the argument reduced exactly (the device's cospi does the same): the reduced
    argument |r| <= 1/4 makes the rounding of pi r harmless."""
    n = np.rint(2.0 * t)                                   # nearest half-integer multiple: t = n / 2 + r
    r = t - 0.5 * n                                        # exact
    q = n.astype(np.int64) & 3
    c, s = np.cos(np.pi * r), np.sin(np.pi * r)
    return np.where(q == 0, c, np.where(q == 1, -s, np.where(q == 2, -c, s)))


def uniforms(seed, member, day, reach, series):
    """The two uniforms (u1, u2) in (0, 1) of a draw."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    x0, x1, x2, x3 = philox4x32_10((member, day, reach, series), (seed & 0xFFFFFFFF, seed >> 32))
    return _uniform(x0, x1), _uniform(x2, x3)


def standard_normal(seed, member, day, reach, series):
    """z of (seed, member id, absolute day index, zero-based model reach, series id); the four index arguments broadcast."""
    u1, u2 = uniforms(seed, member, day, reach, series)
    return np.sqrt(-2.0 * np.log(u1)) * _cospi(2.0 * u2)


def perturb(v, m, z):
    """The error model v + (m v) z in the device's order of operations."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(all='ignore'):
        return v + (np.asarray(m, dtype=np.float64) * v) * np.asarray(z, dtype=np.float64)
