"""What a correct lane-slot order of the members is (order_members of simplyp_amd/csrc/simplyp_order.h, restated as kernels in
simplyp_order.hip.h), the seeded cost tables the rule is tried on, and one checker, ``check_order``, used unchanged for the host
rule (tests/test_order_host.py) and the device's kernels (tests/test_gpu_order_direct.py).

The rule, from a cost table cost[8][E] of uint32:
  total-cost keys  (0xFFFFFFFF - total mod 2^32) << 32 | member, sorted ascending; nb1 = clamp(E / 256, 1, 24) blocks with borders
                   at E b / nb1
  l = log2(cost + 1), standardised per window: z = (l - mean) * inv, inv = 1 / (deviation + 1e-12)
  PC2, PC3         z projected on the eigenvectors of the 2nd and 3rd largest eigenvalue of z's 8 x 8 covariance
  inside block b   nb2 = clamp(E / (256 nb1), 1, 6) sub-blocks by PC2 (ascending iff b is even), inside sub-block c by PC3
                   (ascending iff b nb2 + c is even); the member id decides between equal values

Block membership, the tie rule and the degenerate table are integers and are checked exactly.  Everything else is computed in
fp32 by the rule and is judged stage by stage against fp64, each stage on the values the stage before it REPORTED (the 68
doubles of simplyp_order_members' diag), so that no tolerance has to cover another stage's error."""

import numpy as np

WIN = 8
MIN_BLOCK, MAX_BLOCKS, MAX_SUB = 256, 24, 6
ORD_CHUNK = 8192
ORD_MAX_E = MAX_BLOCKS * ORD_CHUNK
N_COV = WIN * (WIN + 1) // 2
DIAG = 2 * WIN + N_COV + 2 * WIN                  # mean[8], inv[8], cov[36] (i <= j, row by row), v2[8], v3[8]
IU = np.triu_indices(WIN)

# One log cost as the rule forms it in fp32 against fp64: four fp32 ulps of the top binade (l <= 32, an ulp there is 2^-19) for
# log2f, the conversion of the cost, the rounding of the mean to fp32 and the subtraction.
DELTA = 2.0 ** -17
INV_OF_ZERO = 1.0 / 1e-12                         # inv of a window whose deviation is exactly 0

SIZES_PILOT = [1, 2, 63, 64, 255, 256, 257, 511, 512, 1025, 6143, 6144, 8191, 8192, 8193, 12287, 12288, 12289, 16384, 16385,
               36864, 100000, 196607, 196608]
SIZES_OTHER = [257, 8193, 12289, 36864]
TABLES = ['pilot', 'equal', 'constant_window', 'twelve_rows', 'zeros', 'large', 'wrap']
CASES = [('pilot', E) for E in SIZES_PILOT] + [(t, E) for t in TABLES[1:] for E in SIZES_OTHER]


def shape(E):
    """(nb1, nb2): the library's two formulas."""
    nb1 = max(1, min(MAX_BLOCKS, E // MIN_BLOCK))
    return nb1, max(1, min(MAX_SUB, E // (nb1 * MIN_BLOCK)))


def spans(E):
    """[(b, c, lo, hi)]: the positions [lo, hi) of sub-block c of block b."""
    nb1, nb2 = shape(E)
    out = []
    for b in range(nb1):
        lo, hi = E * b // nb1, E * (b + 1) // nb1
        for c in range(nb2):
            out.append((b, c, lo + (hi - lo) * c // nb2, lo + (hi - lo) * (c + 1) // nb2))
    return out


def total_keys(cost):
    """The total-cost keys in member order (uint64): the totals are formed mod 2^32, as both rules form them in uint32."""
    total = cost.astype(np.uint64).sum(axis=0) & np.uint64(0xFFFFFFFF)
    return ((np.uint64(0xFFFFFFFF) - total) << np.uint64(32)) | np.arange(cost.shape[1], dtype=np.uint64)


def blocks_by_total_cost(cost_or_keys, perm):
    """The members of each block of `perm`, sorted, next to the members of the same slice of the sorted keys."""
    E = len(perm)
    keys = cost_or_keys if cost_or_keys.ndim == 1 else np.sort(total_keys(cost_or_keys))
    nb1 = shape(E)[0]
    got = [np.sort(perm[E * b // nb1:E * (b + 1) // nb1]) for b in range(nb1)]
    want = [np.sort((keys[E * b // nb1:E * (b + 1) // nb1] & np.uint64(0xFFFFFFFF)).astype(np.int64)) for b in range(nb1)]
    return got, want


def log_costs(cost):
    return np.log2(cost.astype(np.float64) + 1.0)


# ---- the cost tables ---------------------------------------------------------------------------------------------------------------
# Three latent factors with orthogonal loadings over the eight windows plus noise: per window the variance of l is
# 1.0 + 0.7225 + 0.49 + 0.01, and the covariance of the standardised windows has the eigenvalues (8 * 1.0 + 0.01,
# 8 * 0.7225 + 0.01, 8 * 0.49 + 0.01, 0.01 five times) / 2.2225 = 3.60, 2.61, 1.77, 0.0045: gaps of 1.0, 0.84 and 1.76.  The third
# factor is kept strong on purpose: PC3's spread over a sub-block of 1365 members (E = 196608) is what keeps neighbours further
# apart than their tolerances (with loadings 1.0, 0.6, 0.4 1.5 % of the pairs there were closer: over the cap of the tests).
LOADINGS = np.array([[1.0] * 8, [0.85] * 4 + [-0.85] * 4, [0.7, 0.7, -0.7, -0.7] * 2])
NOISE = 0.1
MIN_GAP = 0.2                                     # between the four largest eigenvalues
MIN_DEVIATION = 0.05                              # of a window's l that is not constant


def _latent(rng, n, centre):
    f = rng.standard_normal((3, n))
    if n >= 63:                                   # the factors' SAMPLE covariance made the identity: the gaps hold at 63 members too
        f -= f.mean(axis=1, keepdims=True)
        f = np.linalg.solve(np.linalg.cholesky(f @ f.T / n), f)
    return centre + LOADINGS.T @ f + NOISE * rng.standard_normal((WIN, n))


def _to_cost(l, top):
    return np.clip(np.rint(np.exp2(l)) - 1.0, 0.0, float(top)).astype(np.uint64).astype(np.uint32)


def table(kind, E, seed=2024):
    """The cost table [8][E] (uint32) of one case.  Asserts what the checker's bounds assume of it: a window's l is constant or
    deviates by at least MIN_DEVIATION, and (from 63 members on) the four largest eigenvalues are MIN_GAP apart."""
    rng = np.random.default_rng([seed, TABLES.index(kind), E])
    gaps = E >= 63
    if kind == 'pilot':                           # lognormal, a few hundred to a few thousand
        cost = _to_cost(_latent(rng, E, 10.5), 2 ** 31)
    elif kind == 'equal':                         # cost + 1 a power of two: l and every sum of it are exact in fp32 and fp64
        cost = np.repeat(np.array([1023, 511, 2047, 1023, 255, 4095, 1023, 511], dtype=np.uint32)[:, None], E, axis=1)
        gaps = False
    elif kind == 'constant_window':
        cost = _to_cost(_latent(rng, E, 10.5), 2 ** 31)
        cost[3] = 1023
    elif kind == 'twelve_rows':                   # the twelve patterns spread along the factors, not drawn: few points, sure gaps
        f = np.array([[-1.5, -1.2, -0.9, -0.6, -0.3, 0.0, 0.3, 0.6, 0.9, 1.2, 1.5, 0.1],
                      [1.0, -1.0, 0.5, -0.5, 1.5, -1.5, -1.0, 1.0, -0.5, 0.5, 0.2, -0.2],
                      [-1.0, -1.0, 1.0, 1.0, 0.0, 0.0, 1.0, -1.0, -1.0, 1.0, 0.0, 0.0]])
        rows = _to_cost(10.5 + LOADINGS.T @ f + NOISE * np.random.default_rng(seed).standard_normal((WIN, 12)), 2 ** 31)
        cost = rows[:, rng.integers(0, 12, E)]
    elif kind == 'zeros':                         # a tenth all zero; a tenth zero in the windows of one of two patterns
        cost = _to_cost(_latent(rng, E, 10.5), 2 ** 31)
        u = rng.random(E)
        cost[:, u < 0.1] = 0
        cost[:4, (u >= 0.1) & (u < 0.17)] = 0
        cost[np.ix_([0, 1, 4, 5], np.flatnonzero((u >= 0.17) & (u < 0.2)))] = 0
    elif kind == 'large':                         # up to 2^29 - 1: totals approach 2^32 and do not pass it
        cost = _to_cost(_latent(rng, E, 25.5), 2 ** 29 - 1)
        assert int(cost.astype(np.uint64).sum(axis=0).max()) < 2 ** 32
    elif kind == 'wrap':                          # totals pass 2^32: the keys are formed mod 2^32
        cost = _to_cost(_latent(rng, E, 29.0), 2 ** 32 - 1)
        assert int(cost.astype(np.uint64).sum(axis=0).max()) >= 2 ** 32
    else:
        raise KeyError(kind)
    l = log_costs(cost)
    const = cost.min(axis=1) == cost.max(axis=1)
    sd = l.std(axis=1)
    assert np.all(const | (sd >= MIN_DEVIATION)), (kind, E, sd)
    if gaps:
        z = (l - l.mean(axis=1, keepdims=True)) / np.where(const, 1.0, sd)[:, None]
        w = np.linalg.eigvalsh(z @ z.T / E)[::-1]
        assert np.all(w[:3] - w[1:4] >= MIN_GAP), (kind, E, w)
    return cost


# ---- the checker --------------------------------------------------------------------------------------------------------------------
def _sorted_within(ref, tol, ascending):
    """(ok, ratio): `ref` counts as sorted ascending when for every j max_{i<j}(ref_i - tol_i) <= ref_j + tol_j (descending: the
    mirror).  ratio: the largest step against the order, over the two tolerances of the members that make it."""
    if len(ref) < 2:
        return True, 0.0
    if not ascending:
        ref = -ref
    low = ref - tol
    at = np.zeros(len(ref), dtype=np.int64)       # the i < j with the largest ref_i - tol_i
    run = np.maximum.accumulate(low)
    first = np.flatnonzero(np.r_[True, low[1:] > run[:-1]])
    at[first] = first
    at = np.maximum.accumulate(at)
    i = at[:-1]
    ok = bool(np.all(low[i] <= ref[1:] + tol[1:]))
    step, room = ref[i] - ref[1:], tol[i] + tol[1:]
    return ok, float(np.max(np.where(room > 0.0, step / np.where(room > 0.0, room, 1.0), np.where(step > 0.0, np.inf, 0.0)), initial=0.0))


def check_order(cost, perm, diag, keys=None):
    """Asserts that `perm` (with the rule's reported intermediate results `diag` [68], and the device's sorted total-cost keys
    where given) is a correct order of the members of `cost` [8][E].  Returns the largest ratio of observed deviation to bound
    of every stage and the share of adjacent pairs that the tolerances leave unconstrained."""
    cost = np.ascontiguousarray(cost, dtype=np.uint32)
    perm = np.asarray(perm).astype(np.int64)
    diag = np.asarray(diag, dtype=np.float64)
    E = cost.shape[1]
    assert cost.shape == (WIN, E) and perm.shape == (E,) and diag.shape == (DIAG,)
    nb1, nb2 = shape(E)
    ratio = {}

    # -- integers: exact
    assert np.array_equal(np.sort(perm), np.arange(E)), 'not a permutation'
    key_sorted = np.sort(total_keys(cost))
    if keys is not None:
        assert np.array_equal(np.asarray(keys, dtype=np.uint64), key_sorted), 'the sorted total-cost keys'
    got, want = blocks_by_total_cost(key_sorted, perm)
    for b in range(nb1):
        assert np.array_equal(got[b], want[b]), 'block %d does not hold its slice of the total-cost order' % b
    _, pattern = np.unique(cost.T, axis=0, return_inverse=True)
    pattern = pattern.reshape(-1)
    for b, c, lo, hi in spans(E):                 # equal costs: bit-identical PC2 and PC3, so the member id decides
        who = perm[lo:hi]
        by = np.lexsort((np.arange(hi - lo), pattern[who]))
        same = pattern[who][by][1:] == pattern[who][by][:-1]
        assert np.all(who[by][1:][same] > who[by][:-1][same]), 'members of equal costs out of member order in sub-block (%d, %d)' % (b, c)

    mean, inv, cov = diag[:WIN], diag[WIN:2 * WIN], diag[2 * WIN:2 * WIN + N_COV]
    v2, v3 = diag[2 * WIN + N_COV:3 * WIN + N_COV], diag[3 * WIN + N_COV:]
    l = log_costs(cost)
    const = cost.min(axis=1) == cost.max(axis=1)
    # a constant window whose sums are exact in both precisions: one member, or cost + 1 a power of two (l a small integer)
    exact = const & ((E == 1) | ((cost[:, 0].astype(np.uint64) + 1) & cost[:, 0].astype(np.uint64) == 0))
    if const.all():                               # zero variance in every window: the index rule decides everything
        assert np.array_equal(perm, np.arange(E)), 'no variance in any window: the identity'
        assert np.array_equal(v2, np.eye(WIN)[1]) and np.array_equal(v3, np.eye(WIN)[2])
        assert np.all(cov == 0.0)
    assert np.all(inv[exact] == INV_OF_ZERO), inv
    power_of_two = (cost[:, 0].astype(np.uint64) + 1) & cost[:, 0].astype(np.uint64) == 0
    assert np.all(mean[const & power_of_two] == l[const & power_of_two, 0]), mean

    # -- moments, against NumPy's on l
    sd = np.where(const, 0.0, l.std(axis=1))
    inv_ref = 1.0 / (sd + 1e-12)
    ratio['mean'] = float(np.max(np.abs(mean - l.mean(axis=1)) / DELTA))
    live = ~const
    ratio['inv'] = float(np.max(np.abs(inv[live] - inv_ref[live]) / inv_ref[live] / (2.0 * DELTA * inv_ref[live] + 1e-9), initial=0.0))
    assert ratio['mean'] <= 1.0 and ratio['inv'] <= 1.0, ratio

    # -- covariance, against the fp64 covariance of z formed from the REPORTED mean and inv.  A constant window's z is exactly 0
    # in the rule (every l equals the mean); elsewhere the rule's fp32 z is off by dz = DELTA inv + 2^-23 |z| (inv's rounding and
    # the product's), a product z_i z_j by |z_i| dz_j + |z_j| dz_i + dz_i dz_j + 2^-24 |z_i z_j| (its own rounding); the fp64 sums
    # add a relative 2^-40 at the very most.
    z = np.where(const[:, None], 0.0, (l - mean[:, None]) * inv[:, None])
    dz = np.where(const[:, None], 0.0, DELTA * inv[:, None] + 2.0 ** -23 * np.abs(z))
    az = np.abs(z)
    cov_ref = (z @ z.T / E)[IU]
    cov_bound = ((az @ dz.T + dz @ az.T + dz @ dz.T + (2.0 ** -24 + 2.0 ** -40) * (az @ az.T)) / E)[IU]
    err = np.abs(cov - cov_ref)
    ratio['cov'] = float(np.max(np.where(err > 0.0, err / np.where(cov_bound > 0.0, cov_bound, 1.0), 0.0)))
    assert np.all(err <= cov_bound), (ratio['cov'], cov, cov_ref)

    # -- eigenvectors, against eigh of the REPORTED covariance: fp32 unit vectors, orthogonal, and ||A v - lambda v|| <=
    # 1e-6 ||A|| with lambda the second and third largest eigenvalue (Jacobi stops at off^2 < 1e-22; the vectors are fp32)
    A = np.zeros((WIN, WIN))
    A[IU] = cov
    A = A + np.triu(A, 1).T
    lam = np.linalg.eigvalsh(A)[::-1]
    norm_A = float(np.max(np.abs(lam)))
    ratio['unit'] = float(max(abs(np.linalg.norm(v2) - 1.0), abs(np.linalg.norm(v3) - 1.0)) / 2.0 ** -22)
    ratio['orthogonal'] = float(abs(v2 @ v3) / 2.0 ** -22)
    res = max(np.linalg.norm(A @ v2 - lam[1] * v2), np.linalg.norm(A @ v3 - lam[2] * v3))
    ratio['eigen'] = float(res / (1e-6 * norm_A)) if norm_A > 0.0 else float(res > 0.0) * 2.0
    assert ratio['unit'] <= 1.0 and ratio['orthogonal'] <= 1.0 and ratio['eigen'] <= 1.0, ratio

    # -- the order, against PC2 and PC3 in fp64 from l and the REPORTED mean, inv, v2, v3
    pc2, pc3 = v2 @ z, v3 @ z
    spread = np.where(const[:, None], 0.0, DELTA * inv[:, None] + 2.0 ** -21 * az)
    tol2, tol3 = np.abs(v2) @ spread, np.abs(v3) @ spread
    ratio['pc2'] = ratio['pc3'] = 0.0
    loose = pairs = 0
    before = None
    for b, c, lo, hi in spans(E):
        who = perm[lo:hi]
        if hi > lo:
            ok, r = _sorted_within(pc3[who], tol3[who], (b * nb2 + c) % 2 == 0)
            ratio['pc3'] = max(ratio['pc3'], r)
            assert ok, 'sub-block (%d, %d) is not sorted by PC3: %.3g of the tolerance' % (b, c, r)
            loose += int(np.sum(np.abs(np.diff(pc3[who])) < tol3[who][1:] + tol3[who][:-1]))
            pairs += hi - lo - 1
        if c > 0 and hi > lo and len(before):     # consecutive sub-blocks of a block are separated in PC2
            up = b % 2 == 0
            first, second = (before, who) if up else (who, before)
            step = np.max(pc2[first] - tol2[first]) - np.min(pc2[second] + tol2[second])
            i, j = first[np.argmax(pc2[first] - tol2[first])], second[np.argmin(pc2[second] + tol2[second])]
            r = max(0.0, float((pc2[i] - pc2[j]) / (tol2[i] + tol2[j]))) if tol2[i] + tol2[j] > 0.0 else float(pc2[i] > pc2[j]) * 2.0
            ratio['pc2'] = max(ratio['pc2'], r)
            assert step <= 0.0, 'sub-blocks (%d, %d) and (%d, %d) overlap in PC2: %.3g of the tolerance' % (b, c - 1, b, c, r)
        before = who
    ratio['unconstrained'] = loose / pairs if pairs else 0.0
    return ratio
