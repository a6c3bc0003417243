"""The second-order ratio predictor of the packed output stream on the host alone (simplyp_pack.h through
simplyp_pack_roundtrip_host_pred).  A column coded against another one is predicted as X[d] * (2 r[d-1] - r[d-2]) with
r[d] = Y[d] / X[d] wherever that makes a span of 64 rows of a block smaller than X[d] * r[d-1] does; the first delta row of a
chunk has no r[d-2] and stays first order.  Whatever the order and whatever the ratio meets, the table comes back bit for bit,
and no table costs more than under the first-order rule alone."""

import numpy as np
import pytest

from oracle import oracle
from simplyp_amd import marshal
from test_gpu_stream_packed import perturbed
from test_pack_rows_host import CHUNK, GROUP, U, f2u, predictor_table, record_overhead, roundtrip

MASK63 = U(0x7FFFFFFFFFFFFFFF)


# ---- tables (shared with tests/test_gpu_stream_order2.py) -----------------------------------------------------------

def smooth_x(rng, rows, E):
    return np.exp(rng.normal(0.0, 0.3, (rows, E)).cumsum(axis=0) * 0.05) * rng.uniform(0.5, 50.0, E)[None, :]


def drifting_table(rows=130, E=200, extrapolates=True):
    """[2, rows, E]: Y = X * k * (1 + 1e-5 * d), a ratio that drifts at a steady rate; `extrapolates` False: the ratio
    alternates between k and k * (1 + 1e-5), which the previous ratio predicts as badly and the extrapolation worse."""
    rng = np.random.default_rng(17)
    x = smooth_x(rng, rows, E)
    d = np.arange(rows)
    k = rng.uniform(0.01, 0.03, E)[None, :]
    y = x * k * (1.0 + 1e-5 * (d if extrapolates else d % 2))[:, None]
    return np.stack([f2u(x), f2u(y)])


def noisy_table(rows=130, E=200):
    """[2, rows, E]: the recipe of predictor_table()'s ordinary members -- the ratio is a constant with 1e-4 of white noise,
    which an extrapolation doubles."""
    rng = np.random.default_rng(5)
    x = smooth_x(rng, rows, E)
    y = x * rng.uniform(0.01, 0.03, E)[None, :] * (1.0 + 1e-4 * rng.normal(size=(rows, E)))
    return np.stack([f2u(x), f2u(y)])


def special_table(rows=130):
    """[2, rows, 200]: a drifting ratio, so that second order is what the spans choose, and in block 0 the special values of
    predictor_table() block 0, a ratio whose doubling overflows and a denormal ratio."""
    u = drifting_table(rows, 200)
    x, y = u[0].view(np.float64).copy(), u[1].view(np.float64).copy()
    d = np.arange(rows)
    x[:, 0] = np.where(d % 5 == 0, np.inf, x[:, 0])
    x[:, 1] = np.where(d % 7 == 3, 0.0, x[:, 1])
    x[:, 2] = np.where(d % 4 == 1, -0.0, x[:, 2])
    x[:, 3] = 4.9e-324 * (1 + d)
    y[:, 3] = 1e-310 * (1 + d)
    x[:, 4] = 1e-300; y[:, 4] = 1e300
    x[:, 5] = 1e300; y[:, 5] = 3e-320
    x[:, 6] = 1e150; y[:, 6] = 1e-165 * (1 + d)
    y[:, 7] = 0.0
    y[:, 8] = np.where(d % 3 == 0, np.inf, y[:, 8])
    x[:, 11] = 1e-300 * (1.0 + 1e-3 * d); y[:, 11] = x[:, 11] * 1e308            # r1 = 1e308: 2 r1 = inf
    x[:, 12] = 1e200 * (1.0 + 1e-3 * d); y[:, 12] = 1e-120 * (1.0 + 2e-3 * d)     # r1 = 1e-320, a denormal; the product is normal
    x[:, 13] = 1e-300; y[:, 13] = np.where(d % 2 == 0, 1.7e308, 1e8)             # 2 r1 - r2 = -inf on odd days
    u = np.stack([f2u(x), f2u(y)])
    u[0, :, 9] = U(0x7FF8000000000000) | (d.astype(np.uint64) * U(0x0000100000000001))
    u[1, :, 10] = U(0xFFF4000000000001) + d.astype(np.uint64)
    return u


# ---- the first-order format restated in numpy -----------------------------------------------------------------------

def bit_length(v):
    w = np.zeros(v.shape, dtype=np.int64)
    for k in range(64):
        w += (v >> U(k)) != 0
    return w


def zigzag(delta):
    return (delta << U(1)) ^ (U(0) - (delta >> U(63)))


def first_order_bytes(u, chunk=CHUNK):
    """Bytes of the records of [X, Y] with Y coded against X[d] * (Y[d-1] / X[d-1]) in every span: per record the overhead and
    8 bytes per bit of row width, a row of a 64-member block being as wide as its widest zigzag difference.  (No block of the
    tables this is used on passes 56 bits, so every record travels packed.)"""
    x, y = u[0].view(np.float64), u[1].view(np.float64)
    rows, E = x.shape
    total = 0
    with np.errstate(all='ignore'):
        for c0 in range(0, rows, chunk):
            nd = min(chunk, rows - c0)
            ux, uy = u[0, c0:c0 + nd], u[1, c0:c0 + nd]
            p = f2u(x[c0 + 1:c0 + nd] * (y[c0:c0 + nd - 1] / x[c0:c0 + nd - 1]))
            mag = p & MASK63
            p = np.where((mag == 0) | ((mag >> U(52)) == U(0x7FF)), uy[:-1], p)
            for z in (zigzag(ux[1:] - ux[:-1]), zigzag(uy[1:] - p)):
                words = 0
                for e0 in range(0, E, GROUP):
                    w = bit_length(np.bitwise_or.reduce(z[:, e0:e0 + GROUP], axis=1))
                    assert w.max(initial=0) <= 56
                    words += int(w.sum())
                total += record_overhead(E, nd) + 8 * words
    return total


# ---- tests ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('chunk', [64, 128])
def test_drifting_ratio(chunk):
    """130 rows: two full chunks and a 2-row one (128-day chunks: two spans, the ratio carried from one into the next)."""
    u, v = drifting_table(), drifting_table(extrapolates=False)
    out, counts, nbytes = roundtrip(u, pred=[-1, 0], chunk=chunk)
    assert np.array_equal(out, u)
    out_v, counts_v, nbytes_v = roundtrip(v, pred=[-1, 0], chunk=chunk)
    assert np.array_equal(out_v, v)
    n_rec = 2 * -(-130 // chunk)
    assert counts == [n_rec, 0, 0] and counts_v == [n_rec, 0, 0]
    print('drifting ratio %d bytes, alternating ratio %d bytes' % (nbytes[0], nbytes_v[0]))
    assert nbytes[0] < nbytes_v[0]                                       # X is the same column in both
    if chunk == 64:
        # the extrapolation misses by rounding alone: well under half of what the first-order rule costs
        fo = first_order_bytes(u)
        x_only = roundtrip(u[:1], chunk=chunk)[2][0]
        assert 2 * (nbytes[0] - x_only) < fo - x_only


def test_noisy_ratio_costs_no_more_than_first_order():
    u = np.ascontiguousarray(predictor_table()[:, :, 64:])               # blocks 1 .. 3
    out, counts, nbytes = roundtrip(u, pred=[-1, 0])
    assert np.array_equal(out, u) and counts == [4, 0, 0]
    fo = first_order_bytes(u)
    print('noisy ratio: %d bytes, first order alone %d' % (nbytes[0], fo))
    assert nbytes[0] <= fo
    v = noisy_table()
    out, counts, nbytes = roundtrip(v, pred=[-1, 0])
    assert np.array_equal(out, v) and counts == [6, 0, 0]
    assert nbytes[0] <= first_order_bytes(v)


_oracle_table = []


def oracle_msus_pp():
    if not _oracle_table:
        E = 192
        m = perturbed('tarland_2004_dynamic', E, out_mask=marshal.MASK_REACH5)
        ref, status, _ = oracle.run(m['forcing'], m['doy'], m['member_params'], m['reach_params'], m['up_ptr'], m['up_idx'], m['opts'])
        assert int(status.max()) == 0
        cols = marshal.REACH5_COLUMNS
        pick = [cols.index('Msus_kg/day'), cols.index('PP_kg/day')]
        _oracle_table.append(np.ascontiguousarray(ref[pick, :, 0, :]).view(np.uint64))
    return _oracle_table[0]


def test_size_of_pp_on_the_oracle_table():
    """tarland_2004_dynamic, 192 perturbed members, Msus and PP: the PP column costs at most 4.80 bytes per coded value.  (The
    CPU model of the format gives 4.59 with the second-order rule and 5.09 with the first-order rule alone.)"""
    u = oracle_msus_pp()
    rows, E = 366, 192
    assert u.shape == (2, rows, E)
    out, counts, both = roundtrip(u, pred=[-1, 0])
    n_chunks = -(-rows // CHUNK)
    assert np.array_equal(out, u) and counts[0] == 2 * n_chunks and counts[2] == 0
    _, _, msus = roundtrip(u[:1])
    overhead = sum(record_overhead(E, min(CHUNK, rows - c0)) for c0 in range(0, rows, CHUNK))
    per_value = (both[0] - msus[0] - overhead) / float((rows - n_chunks) * E)
    print('PP: %.3f bytes per coded value' % per_value)
    assert per_value <= 4.80


@pytest.mark.parametrize('chunk', [64, 128])
def test_special_values_round_trip(chunk):
    for u in (predictor_table(), special_table()):
        out, _, _ = roundtrip(u, pred=[-1, 0], chunk=chunk)
        assert np.array_equal(out, u)


def test_special_values_when_every_row_is_a_first_delta_row():
    """Chunks of 2 rows (a table of 2 rows is one such chunk): each day coded from the day before with no r[d-2]."""
    for u in (predictor_table(), special_table(70)):
        for d in range(u.shape[1] - 1):
            v = np.ascontiguousarray(u[:, d:d + 2, :])
            out, _, _ = roundtrip(v, pred=[-1, 0], chunk=2)
            assert np.array_equal(out, v)


def test_first_delta_row_is_first_order():
    """On 2-row tables of ordinary members the bytes are the first-order rule's exactly."""
    u = np.ascontiguousarray(drifting_table()[:, :, 64:])
    for d in (0, 1, 63, 64, 128):
        v = np.ascontiguousarray(u[:, d:d + 2, :])
        out, counts, nbytes = roundtrip(v, pred=[-1, 0], chunk=2)
        assert np.array_equal(out, v) and counts == [2, 0, 0]
        assert nbytes[0] == first_order_bytes(v)
