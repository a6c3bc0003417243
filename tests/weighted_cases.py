"""Rows, weights and probabilities the weighted-band tests share (tests/test_weighted_host.py on the CPU,
tests/test_gpu_weighted_quantiles.py on the device), and the bit-for-bit comparison both make."""

import numpy as np

VALUE_PATTERNS = ('ties', 'normals', 'special')
WEIGHT_PATTERNS = ('ones', 'all_max', 'one_heavy', 'zeros30', 'one_survivor', 'all_zero')
PROBS = [0.0, 0.025, 0.5, 0.975, 1.0]


def values(pattern, shape, rng):
    """A table [..., E] of the pattern: heavy ties, distinct normals, or rows with NaN / +-inf / +-0.0 among normals."""
    if pattern == 'ties':
        return rng.integers(0, 8, shape).astype(np.float64)
    x = rng.standard_normal(shape)
    if pattern == 'special':
        pick = rng.integers(0, 12, shape)
        for code, v in enumerate([np.nan, np.inf, -np.inf, 0.0, -0.0]):
            x = np.where(pick == code, v, x)
    return x


def weights(pattern, E, rng):
    """Integer weights [E] (uint64) of the pattern."""
    if pattern == 'ones':
        return np.ones(E, dtype=np.uint64)
    if pattern == 'all_max':
        return np.full(E, 1 << 40, dtype=np.uint64)
    if pattern == 'one_heavy':
        q = np.ones(E, dtype=np.uint64)
        q[int(rng.integers(0, E))] = 1 << 40
        return q
    if pattern == 'zeros30':
        q = rng.integers(1, (1 << 40) + 1, E).astype(np.uint64)
        q[rng.random(E) < 0.3] = 0
        return q
    if pattern == 'one_survivor':
        q = np.zeros(E, dtype=np.uint64)
        q[int(rng.integers(0, E))] = int(rng.integers(1, (1 << 40) + 1))
        return q
    if pattern == 'all_zero':
        return np.zeros(E, dtype=np.uint64)
    raise KeyError(pattern)


def power_of_two_total(E, rng, log2_T=30):
    """Positive weights [E] whose sum is exactly 2^log2_T, so that C_i / T is a float and the boundary probabilities are exact."""
    q = rng.integers(1, 1 << 12, E).astype(np.uint64)
    rest = (1 << log2_T) - int(q.sum())
    assert rest > 0
    q[int(rng.integers(0, E))] += np.uint64(rest)
    assert int(q.sum()) == 1 << log2_T
    return q


def boundary_probs(row, q, n=4, rng=None):
    """Probabilities exactly on a running-sum boundary C_i / T of the sorted row (T a power of two) and one ulp either side."""
    order = np.argsort(row, kind='stable')
    C = np.cumsum(q[order].astype(np.uint64))
    T = int(C[-1])
    assert T & (T - 1) == 0
    at = np.unique(np.linspace(0, len(C) - 1, n).astype(int)) if rng is None else rng.integers(0, len(C), n)
    out = []
    for i in at:
        p = float(int(C[i])) / float(T)                     # exact: T is a power of two and C_i < 2^53
        out += [np.nextafter(p, 0.0), p, min(np.nextafter(p, 2.0), 1.0)]
    return out


def same_bits(a, b):
    """Equal bit for bit, except that -0.0 and +0.0 count as equal."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    both_zero = (a == 0) & (b == 0)
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | both_zero))
