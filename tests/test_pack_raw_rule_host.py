"""Which records of the packed output stream travel raw, on the host alone (simplyp_pack::route_of through
simplyp_pack_roundtrip_host_pred).  A record goes raw when its body passed its capacity, or when it has more overflow blocks
(blocks with a coded difference of 2^56 or more) than the capacity allows for AND its packed copy would not be smaller than its
rows.  Many overflow blocks alone send nothing raw: a block with one wide row is still small.  The raw path itself is pinned by
column 1 of made_up_table and by dependency_table (tests/test_pack_rows_host.py), where every row of every block is wide."""

import numpy as np

from oracle import oracle
from simplyp_amd import marshal, synthetic
from test_pack_rows_host import CHUNK, U, roundtrip, smooth

JUMP_MEMBERS = (0, 64, 128, 192)         # the first member of each of the 4 blocks
JUMP_DAYS = (10, 80)                     # one in chunk 0, one in chunk 1, none in chunk 2 (days 128, 129)


def jump_table():
    """[2, 130, 200]: 3 chunks of 64, 64 and 2 days, 4 blocks, so the capacity allows for 4 / 8 + 3 = 3 overflow blocks.  Both
    columns are smooth (rows of at most 42 bits: a record's 256 coded lanes stay well below 200 raw doubles).  In column 0 the
    first member of every block takes a lasting jump of 2^57 on day 10 and another on day 80: 4 overflow blocks, one more than
    the capacity allows for, in chunks 0 and 1, each with a single wide row."""
    u = smooth(np.random.default_rng(23), 2, 130, 200, bits=40)
    for e in JUMP_MEMBERS:
        for d in JUMP_DAYS:
            u[0, d:, e] += U(1) << U(57)
    return u


def ratio_table():
    """jump_table() with column 1 = 0.25 x column 0 exactly, to be coded against column 0."""
    u = jump_table()
    x = u[0].view(np.float64)
    assert np.isfinite(x).all() and (np.abs(x) > 1e-300).all()
    u[1] = np.ascontiguousarray(0.25 * x).view(np.uint64)
    return u


def test_many_overflow_blocks_in_a_small_record_travel_packed():
    u = jump_table()
    out, counts, nbytes = roundtrip(u)
    assert np.array_equal(out, u)
    assert counts == [6, 8, 0]                                           # (the count alone made it [4, 0, 2])
    assert nbytes[1] == 6 * 200 * 8                                      # every record's first row travels


def test_column_predicted_from_such_a_column_travels_packed():
    u = ratio_table()
    out, counts, _ = roundtrip(u, pred=[-1, 0])
    assert np.array_equal(out, u)
    assert counts[2] == 0


MODEL_E, MODEL_DAYS, MODEL_END = 256, 1408, '1984-11-08'                  # 22 chunks
MODEL_SEED = synthetic.C3_SEED + 7
# what travelled under the count rule: 108 packed records of 10 777 592 bytes together and two raw ones of 64 x 256 x 8 each
MODEL_BYTES_BEFORE = 10777592 + 2 * 131072


def model_pred():
    pred = [-1] * 5
    pred[marshal.REACH5_COLUMNS.index('PP_kg/day')] = marshal.REACH5_COLUMNS.index('Msus_kg/day')
    return pred


def test_model_table_has_no_raw_record_and_fewer_bytes():
    """The CPU oracle's table of 256 members of the C3 draw, 1408 days, member order, PP coded against Msus.  On a few days
    Msus starts from nothing in every member at once: every block of such a chunk is an overflow block, with a few wide rows."""
    pr = synthetic.c3_problem(MODEL_E, end_dt=MODEL_END, seed=MODEL_SEED)
    ref, status, _ = oracle.run(pr['forcing'], pr['doy'], pr['member_params'], pr['reach_params'], pr['up_ptr'], pr['up_idx'], pr['opts'])
    assert int(status.max()) == 0
    u = np.ascontiguousarray(ref[:, :, 0, :]).view(np.uint64)
    assert u.shape == (5, MODEL_DAYS, MODEL_E) and model_pred() == [-1, -1, -1, -1, 2]
    out, counts, nbytes = roundtrip(u, pred=model_pred())
    print('counts %s, packed bytes %d (before: %d with the raw records)' % (counts, nbytes[0], MODEL_BYTES_BEFORE))
    assert np.array_equal(out, u)
    assert counts == [110, 9, 0]
    assert nbytes[0] < MODEL_BYTES_BEFORE
    assert CHUNK * 22 == MODEL_DAYS
