"""The row-adaptive records of the packed output stream on the host alone (simplyp_pack.h through
simplyp_pack_roundtrip_host_pred): the plain C++ encoder, then the decoder the stream's pool uses.  Every row of a 64-member block
is stored at the bit width of its widest coded difference; a column may be coded against X[d] * (Y[d-1] / X[d-1]) of another one.
Whatever the widths and whatever the predictor meets, the decoded table is the input bit for bit."""

import ctypes as C

import numpy as np
import pytest

from oracle import oracle
from simplyp_amd import engine, marshal
from test_gpu_stream_packed import made_up_table, perturbed

GROUP, CHUNK = 64, 64
U = np.uint64
SIGN = U(1) << U(63)


def roundtrip(u, pred=None, chunk=CHUNK):
    """u: [n_cols, rows, E] uint64 patterns.  Returns (decoded, counts, bytes)."""
    u = np.ascontiguousarray(u, dtype=np.uint64)
    n_cols, rows, E = u.shape
    out = np.full_like(u, 7)
    counts = (C.c_int32 * 3)()
    nbytes = (C.c_int64 * 2)()
    pc = None if pred is None else (C.c_int32 * n_cols)(*pred)
    rc = engine.lib().simplyp_pack_roundtrip_host_pred(C.c_void_p(u.ctypes.data), n_cols, rows, E, chunk, pc, C.c_void_p(out.ctypes.data),
                                                       counts, nbytes)
    assert rc == 0
    return out, list(counts), list(nbytes)


def smooth(rng, n_cols, rows, E, bits=50):
    base = U(0x3FF0000000000000) + (np.arange(E, dtype=np.uint64) * U(12345))[None, :]
    steps = rng.integers(-(1 << bits), 1 << bits, size=(n_cols, rows, E), dtype=np.int64)
    steps[:, 0, :] = 0
    return (base[None, :, :] + np.cumsum(steps, axis=1).astype(np.uint64)).astype(np.uint64)


def record_overhead(E, nd):
    """Bytes of a record whose rows all have width 0: first row and directory, each padded to 256, and 8 bytes of padding."""
    G, rows = -(-E // GROUP), nd - 1
    n_spans = -(-rows // 64)
    entry = -(-(4 * n_spans + rows) // 4) * 4
    off_dir = -(-E * 8 // 256) * 256
    return -(-(off_dir + G * entry) // 256) * 256 + 8


def test_made_up_table_and_its_counters():
    u = made_up_table()
    out, counts, nbytes = roundtrip(u)
    assert np.array_equal(out, u)
    assert counts == [3, 4, 3]
    assert nbytes[1] == 3 * 200 * 8


def test_constant_column_has_width_zero():
    u = np.full((1, 130, 200), 0x400921FB54442D18, dtype=np.uint64)
    u[0, :, 7] = 0x7FF8000000000123           # a NaN that stays is constant too
    out, counts, nbytes = roundtrip(u)
    assert np.array_equal(out, u) and counts == [3, 0, 0]
    assert nbytes[0] == 2 * record_overhead(200, 64) + record_overhead(200, 2)
    assert nbytes[1] == 3 * 200 * 8


@pytest.mark.parametrize('bits', [1, 55, 56, 57, 63, 64])
def test_rows_of_an_exact_width(bits):
    """Block 1 of 3: on odd days one member's coded difference needs exactly `bits` bits, on even days the row is as narrow as
    the rest.  The body grows by 8 * bits bytes for each such row and by nothing else."""
    rng = np.random.default_rng(bits)
    E, rows = 150, 64
    u = smooth(rng, 1, rows, E, bits=20)
    quiet, _, quiet_bytes = roundtrip(u)
    assert np.array_equal(quiet, u)
    # zigzag(delta) has `bits` bits with the top one set: delta = +2^(bits-2) ... for even z, or its negative twin for odd z
    z = (U(1) << U(bits - 1)) | U(rng.integers(0, 1 << 20) if bits > 21 else 0)
    v = u.copy()
    member = 64 + 17
    with np.errstate(over='ignore'):                             # modulo 2^64
        delta = (z >> U(1)) ^ (U(0) - (z & U(1)))
        for d in range(1, rows, 2):
            v[0, d, member] = v[0, d - 1, member] + delta
            if d + 1 < rows:
                v[0, d + 1, member] = v[0, d, member]
    out, counts, nbytes = roundtrip(v)
    assert np.array_equal(out, v)
    assert counts == [1, 1 if bits > 56 else 0, 0]
    if bits >= 22:
        # 32 odd days, on which block 1's row goes from <= 22 bits to `bits`; the 31 even days after them, on which the member's
        # difference is now 0, can only lose width, 22 bits at the most
        assert nbytes[0] >= quiet_bytes[0] + 32 * 8 * (bits - 22) - 31 * 8 * 22
        assert nbytes[0] <= quiet_bytes[0] + 32 * 8 * bits


@pytest.mark.parametrize('E', [1, 63, 64, 65, 200])
@pytest.mark.parametrize('rows,chunk', [(2, 2), (64, 64), (65, 64), (130, 64), (130, 128)])
def test_member_and_day_counts(E, rows, chunk):
    rng = np.random.default_rng(E * 1000 + rows)
    u = smooth(rng, 2, rows, E)
    u[1, :, 0] ^= (np.arange(rows, dtype=np.uint64) % U(2)) * SIGN       # 64-bit rows in block 0 of column 1
    out, counts, _ = roundtrip(u, chunk=chunk)
    assert np.array_equal(out, u)
    assert counts[0] == 2 * -(-rows // (-(-chunk // 64) * 64)) and counts[2] == 0


def f2u(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def predictor_table():
    """[2, 70, 200]: column 1 is coded against column 0.  Members of block 0 carry what the ratio can meet."""
    rng = np.random.default_rng(5)
    rows, E = 70, 200
    x = np.exp(rng.normal(0.0, 0.3, (rows, E)).cumsum(axis=0) * 0.05) * rng.uniform(0.5, 50.0, E)[None, :]
    y = x * rng.uniform(0.01, 0.03, E)[None, :] * (1.0 + 1e-4 * rng.normal(size=(rows, E)))
    d = np.arange(rows)
    x[:, 0] = np.where(d % 5 == 0, np.inf, x[:, 0])                      # inf in X
    x[:, 1] = np.where(d % 7 == 3, 0.0, x[:, 1])                         # X[d-1] = 0: the ratio is inf or NaN
    x[:, 2] = np.where(d % 4 == 1, -0.0, x[:, 2])
    x[:, 3] = 4.9e-324 * (1 + d)                                         # denormal X
    y[:, 3] = 1e-310 * (1 + d)                                           # and Y: the ratio is large, the product denormal
    x[:, 4] = 1e-300; y[:, 4] = 1e300                                    # a ratio that overflows
    x[:, 5] = 1e300; y[:, 5] = 3e-320                                    # a ratio that underflows to 0 / a denormal
    x[:, 6] = 1e150; y[:, 6] = 1e-165 * (1 + d)                          # ratio 1e-315: a denormal ratio, a normal product
    y[:, 7] = 0.0                                                        # Y = 0: the prediction is 0, the previous day is used
    y[:, 8] = np.where(d % 3 == 0, np.inf, y[:, 8])
    u = np.stack([f2u(x), f2u(y)])
    u[0, :, 9] = U(0x7FF8000000000000) | (d.astype(np.uint64) * U(0x0000100000000001))          # NaN payloads in X
    u[1, :, 10] = U(0xFFF4000000000001) + d.astype(np.uint64)                                    # and in Y
    return u


def test_ratio_predictor_round_trip():
    u = predictor_table()
    out, counts, nbytes = roundtrip(u, pred=[-1, 0])
    assert np.array_equal(out, u)
    assert counts[0] + counts[2] == 4
    # where nothing special happens the ratio predicts far better than the previous day: blocks 1 .. 3 alone
    v = np.ascontiguousarray(u[:, :64, 64:])
    _, c_prev, b_prev = roundtrip(v, pred=[-1, -1])
    out, c_ratio, b_ratio = roundtrip(v, pred=[-1, 0])
    assert np.array_equal(out, v) and c_prev == [2, 0, 0] and c_ratio == [2, 0, 0]
    assert b_ratio[0] < b_prev[0]


def test_exact_multiple_has_width_zero():
    """Y = k * X with k a power of two: Y[d-1] / X[d-1] = k and X[d] * k = Y[d] exactly, so every coded difference of Y is 0."""
    rng = np.random.default_rng(9)
    rows, E = 64, 130
    x = rng.uniform(0.5, 50.0, (rows, E))
    x[:, 3] *= -1.0
    x[:, 4] = 3.0 * 2.0 ** -1000                                         # (0.25 * X stays normal)
    u = np.stack([f2u(x), f2u(0.25 * x)])
    out, counts, nbytes = roundtrip(u, pred=[-1, 0])
    assert np.array_equal(out, u) and counts == [2, 0, 0]
    const = u.copy()
    const[1] = const[1, 0]
    _, _, nbytes_const = roundtrip(const, pred=[-1, -1])
    assert nbytes[0] == nbytes_const[0]                                  # column 1 costs what a constant column costs
    _, _, only_x = roundtrip(u[:1])
    assert nbytes[0] == only_x[0] + record_overhead(E, rows)


def dependency_table(overflowing=True):
    """[3, 130, 200], 64-day chunks: 4 blocks, so a record may hold 4 / 8 + 3 = 3 overflow blocks.  Column 0: member 64 * g of
    every block alternates daily between 1.5 and 1.5 * 2**200 -- every block overflows in every chunk, 4 > 3 (`overflowing`
    False: those members stay at 1.5).  Column 1 = 0.25 * column 0 exactly: coded against column 0 its differences are all zero,
    so its own counters are clean.  Column 2 is smooth."""
    rng = np.random.default_rng(31)
    rows, E = 130, 200
    x = rng.uniform(0.5, 50.0, (rows, E))
    for g in range(4):
        x[:, 64 * g] = np.where(np.arange(rows) % 2 == 1, 1.5 * 2.0 ** 200, 1.5) if overflowing else 1.5
    return np.stack([f2u(x), f2u(0.25 * x), smooth(rng, 1, rows, E)[0]])


def test_column_predicted_from_a_raw_column_travels_raw():
    """Column 1 can only be raw by the dependency rule: a decoder that read column 0's rows from the host table while a raw
    copy of them is still on its way would read half-written rows."""
    u = dependency_table()
    out, counts, nbytes = roundtrip(u, pred=[-1, 0, -1])
    assert np.array_equal(out, u)
    assert counts == [3, 0, 6]                                           # column 2's three records; columns 0 and 1 raw
    assert nbytes[1] == 3 * 200 * 8
    quiet = dependency_table(overflowing=False)
    out, counts, _ = roundtrip(quiet, pred=[-1, 0, -1])
    assert np.array_equal(out, quiet) and counts == [9, 0, 0]


def test_round_trip_with_ftz_daz_in_the_caller():
    """The codec resets MXCSR for itself: a caller that flushes denormals gets the same records and the same table."""
    import platform
    if platform.machine() not in ('x86_64', 'AMD64'):
        pytest.skip('MXCSR is an x86 register')
    import mmap
    # stmxcsr / ldmxcsr [rdi]; ret
    code = {'get': b'\x0f\xae\x1f\xc3', 'set': b'\x0f\xae\x17\xc3'}
    buf = mmap.mmap(-1, 4096, prot=mmap.PROT_READ | mmap.PROT_WRITE | mmap.PROT_EXEC)
    buf.write(code['get'].ljust(16, b'\xcc') + code['set'])
    base = C.addressof(C.c_char.from_buffer(buf))
    get = C.CFUNCTYPE(None, C.POINTER(C.c_uint32))(base)
    put = C.CFUNCTYPE(None, C.POINTER(C.c_uint32))(base + 16)
    u = predictor_table()
    want_out, want_counts, want_bytes = roundtrip(u, pred=[-1, 0])
    old = C.c_uint32()
    get(C.byref(old))
    try:
        put(C.byref(C.c_uint32(old.value | 0x8040)))                     # FTZ | DAZ
        out, counts, nbytes = roundtrip(u, pred=[-1, 0])
        now = C.c_uint32()
        get(C.byref(now))
    finally:
        put(C.byref(old))
    assert now.value & 0x8040 == 0x8040                                  # and the caller's setting is handed back
    assert np.array_equal(out, u) and counts == want_counts and nbytes == want_bytes
    del get, put


def test_bad_predictor_columns_are_refused():
    u = smooth(np.random.default_rng(1), 2, 10, 10)
    out = np.zeros_like(u)
    for pred in ([0, -1], [-1, 1], [-2, -1], [-1, 2]):
        pc = (C.c_int32 * 2)(*pred)
        assert engine.lib().simplyp_pack_roundtrip_host_pred(C.c_void_p(u.ctypes.data), 2, 10, 10, CHUNK, pc, C.c_void_p(out.ctypes.data),
                                                             None, None) != 0


def test_size_on_the_oracle_table():
    """tarland_2004_dynamic, 192 perturbed members (three full blocks), the five reach columns with PP coded against Msus:
    the packed rows cost at most 0.90 x 7 bytes per coded value (the oracle gives 0.870 here).  A silent fall-back to wide rows or
    raw records does not pass."""
    E = 192
    m = perturbed('tarland_2004_dynamic', E, out_mask=marshal.MASK_REACH5)
    ref, status, _ = oracle.run(m['forcing'], m['doy'], m['member_params'], m['reach_params'], m['up_ptr'], m['up_idx'], m['opts'])
    assert int(status.max()) == 0
    u = np.ascontiguousarray(ref[:, :, 0, :]).view(np.uint64)
    assert u.shape == (5, 366, E)
    cols = marshal.REACH5_COLUMNS
    pred = [-1] * 5
    pred[cols.index('PP_kg/day')] = cols.index('Msus_kg/day')
    out, counts, nbytes = roundtrip(u, pred=pred)
    n_chunks = -(-366 // CHUNK)
    assert np.array_equal(out, u)
    assert counts[0] == n_chunks * 5 and counts[2] == 0
    n_delta = 5 * (366 - n_chunks) * E
    ratio = (nbytes[0] - nbytes[1]) / (7.0 * n_delta)
    print('packed bytes %d, first rows %d, %d coded values: %.3f of 7 bytes per value' % (nbytes[0], nbytes[1], n_delta, ratio))
    assert nbytes[1] == n_chunks * 5 * E * 8
    assert ratio <= 0.90
