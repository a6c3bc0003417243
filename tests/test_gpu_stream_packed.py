"""The packed output stream (SIMPLYP_STREAM_PACK, simplyp_pack.h): the daily table crosses the link as records of row-adaptive
day-to-day deltas and is decoded on the host.  Whatever path a (time chunk, column) record takes -- packed, packed with overflow
blocks (rows wider than 56 bits), or raw because it holds too many of them -- the host table is the device table bit for bit,
and the counters say which path it was.  Runs the pack epilogue does not handle ignore the switch."""

import ctypes as C

import numpy as np
import pytest

import helpers
from simplyp_amd import engine, marshal

GROUP, CHUNK = 64, 64


def run(eng, m, **kw):
    return eng.run(m['forcing'], m['doy'], m['member_params'], m['reach_params'], m['up_ptr'], m['up_idx'], m['opts'], **kw)


def perturbed(name, E, seed=3, **kw):
    m = helpers.marshal_scenario(name, E=E, **kw)
    rng = np.random.default_rng(seed)
    m['member_params'][marshal.PM_NAMES.index('fc')] *= rng.uniform(0.85, 1.15, E)
    m['member_params'][marshal.PM_NAMES.index('T_g')] *= rng.uniform(0.6, 1.5, E)
    m['member_params'][marshal.PM_NAMES.index('a_Q')] *= rng.uniform(0.6, 1.6, E)
    return m


# ---- made-up tables -------------------------------------------------------------------------------------------------

def made_up_table():
    """[2, 130, 200] as uint64 patterns: 3 chunks (64, 64 and 2 days) of 4 member groups (the last one ragged, 8 members); a
    record holds 4 / 8 + 3 = 3 overflow blocks.
    Column 0: a smooth base whose deltas need <= 52 bits.  Group 0 carries what a delta cannot hold in 56 bits -- sign flips
    every day, +0 / -0 alternating, +inf / -inf, NaNs with changing payloads, a denormal against a normal -- so its block
    overflows in every chunk.  Group 1 has a single jump of 2^57 (member 70, day 80): one more overflow block, in chunk 1 only.
    Group 2 has specials that stay put or move slowly and must come through the packed rows: NaNs with payloads, infinities, zeros,
    growing denormals.  Expected: 3 records packed, 1 + 2 + 1 = 4 overflow blocks.
    Column 1: the first member of every group flips its sign every day, so every block of every chunk overflows: 4 > 3, all three
    records come back raw."""
    rng = np.random.default_rng(11)
    C_, D, E = 2, 130, 200
    base = np.uint64(0x3FF0000000000000) + (np.arange(E, dtype=np.uint64) * np.uint64(12345))[None, :]
    steps = rng.integers(-(1 << 50), 1 << 50, size=(C_, D, E), dtype=np.int64)
    steps[:, 0, :] = 0
    u = (base[None, :, :] + np.cumsum(steps, axis=1).astype(np.uint64)).astype(np.uint64)          # modulo 2^64
    d = np.arange(D, dtype=np.uint64)
    sign = np.uint64(1) << np.uint64(63)
    # column 0, group 0
    u[0, :, 0] ^= (d % np.uint64(2)) * sign                                          # sign flips every day
    u[0, :, 1] = (d % np.uint64(2)) * sign                                           # +0, -0, +0, ...
    u[0, :, 2] = np.uint64(0x7FF0000000000000) | ((d % np.uint64(2)) * sign)         # +inf, -inf, ...
    u[0, :, 3] = np.uint64(0x7FF8000000000000) | (d * np.uint64(0x0000100000000001)) | ((d % np.uint64(3) == 0) * sign)   # NaN payloads
    u[0, :, 4] = np.where(d % np.uint64(2) == 0, np.uint64(5), np.uint64(0x3FF0000000000005))      # a denormal against a normal
    # column 0, group 1: one jump of 2^57 in the pattern, kept from there on
    u[0, 80:, 70] += np.uint64(1) << np.uint64(57)
    # column 0, group 2: specials whose deltas fit 56 bits
    u[0, :, 130] = np.uint64(0x7FF8000000ABCDEF)                                     # a NaN payload that stays
    u[0, :, 131] = np.uint64(0xFFF0000000000000)                                     # -inf
    u[0, :, 132] = sign                                                              # -0
    u[0, :, 133] = np.uint64(1) + d * np.uint64(977)                                 # growing denormals
    u[0, :, 134] = np.uint64(0xFFF4000000000001) + d                                 # signalling-NaN payloads, counting up
    # column 1: every block jumps, every day
    for g in range(4):
        u[1, :, g * GROUP] ^= (d % np.uint64(2)) * sign
    return u


EXPECT_COUNTS = [3, 4, 3]          # records packed, overflow blocks, records raw


def test_host_codec_round_trip_is_exact():
    """The host half of the codec without a GPU: the plain C++ encoder, then the decoder the stream uses."""
    u = made_up_table()
    out = np.zeros_like(u)
    counts = (C.c_int32 * 3)()
    rc = engine.lib().simplyp_pack_roundtrip_host(C.c_void_p(u.ctypes.data), 2, 130, 200, CHUNK, C.c_void_p(out.ctypes.data), counts)
    assert rc == 0
    assert np.array_equal(out, u)
    assert list(counts) == EXPECT_COUNTS
    # one column, one chunk, fewer members than a group; a smooth table has no overflow at all
    v = np.ascontiguousarray(u[0:1, :64, 128:170])
    out = np.zeros_like(v)
    assert engine.lib().simplyp_pack_roundtrip_host(C.c_void_p(v.ctypes.data), 1, 64, 42, CHUNK, C.c_void_p(out.ctypes.data), counts) == 0
    assert np.array_equal(out, v) and list(counts) == [1, 0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize('pinned', [True, False])
def test_made_up_table_through_the_device_packer(engine0, pinned):
    import torch
    u = made_up_table()
    dev = torch.from_numpy(u.view(np.int64)).to(engine0.tdev)
    host = engine.pinned_empty(u.shape) if pinned else np.empty(u.shape)
    host.view(np.uint64)[...] = 7
    counts = (C.c_int32 * 3)()
    with torch.cuda.device(engine0.tdev):
        rc = engine.lib().simplyp_fetch_packed(engine0._h, dev.data_ptr(), 2, 130, 200, CHUNK, C.c_void_p(host.ctypes.data),
                                               C.c_int64(host.nbytes), counts)
    assert rc == 0, engine.lib().simplyp_last_error(engine0._h)
    assert np.array_equal(host.view(np.uint64), u)
    assert list(counts) == EXPECT_COUNTS


# ---- model data ---------------------------------------------------------------------------------------------------

FULL_WAVES = dict(out_slot_order=1, lanes_per_wave=64, lanes_per_member=1)       # what a large ensemble gets by itself

_reference = {}


def model_case(engine0, name, E):
    """The scenario and its unstreamed run (computed once, never modified)."""
    if (name, E) not in _reference:
        m = perturbed(name, E, out_mask=marshal.MASK_REACH5, solver=FULL_WAVES)
        ref, ref_status, _ = run(engine0, m)
        _reference[(name, E)] = (m, ref.cpu().numpy(), ref_status.cpu().numpy())
    return _reference[(name, E)]


@pytest.mark.gpu
@pytest.mark.parametrize('name,E,how', [
    ('tarland_1981_2010_dynamic', 700, 'pinned'),        # 172 chunks, 11 member groups with the last one ragged
    ('tarland_1981_2010_dynamic', 700, 'pageable'),
    ('tarland_1981_2010_dynamic', 700, 'defer_sync'),
    ('tarland_2004_dynamic', 700, 'pinned'),             # 366 days: the last chunk has 46
])
def test_packed_stream_delivers_the_device_table(engine0, monkeypatch, name, E, how):
    import torch
    monkeypatch.setenv('SIMPLYP_STREAM_PACK', '1')
    m, ref, ref_status = model_case(engine0, name, E)
    D = m['forcing'].shape[2]
    shape = (5, D, 1, E)
    host = np.empty(shape) if how == 'pageable' else engine.pinned_empty(shape)
    host[...] = -7.0
    if how == 'defer_sync':
        with torch.cuda.stream(torch.cuda.Stream(engine0.tdev)):
            out, status, st = run(engine0, m, host_out=host, defer_sync=True)
            st.update(st.pop('finish')())
    else:
        out, status, st = run(engine0, m, host_out=host)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    n_chunks = -(-D // CHUNK)
    n_groups = -(-E // GROUP)
    print('packed_records %d (raw %d), overflow blocks %d of %d' % (st['packed_records'] & 0xFFFF, st['packed_records'] >> 16,
                                                                    st['pack_overflow_blocks'], n_chunks * 5 * n_groups))
    assert st['queued'] == 1 and st['lanes_per_wave'] == 64
    assert np.array_equal(host.view(np.uint64), got.view(np.uint64))              # host table = device table
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))              # = the unstreamed run
    assert np.array_equal(status.cpu().numpy(), ref_status)
    assert st['packed_records'] == n_chunks * 5                                  # every record packed, none sent raw
    assert st['pack_overflow_blocks'] < 0.10 * n_chunks * 5 * n_groups           # (2.3 % of two columns' blocks on the CPU sample)


@pytest.mark.gpu
@pytest.mark.parametrize('name,E,solver,annual', [
    ('tarland_2004_dynamic', 200, dict(FULL_WAVES, integrator='cashkarp_aug', lanes_per_wave=0, lanes_per_member=4), False),
    ('tarland_2004_dynamic', 200, dict(FULL_WAVES, lanes_per_wave=8), False),
    ('tarland_1981_2010_dynamic', 130, FULL_WAVES, True),                                   # annual sums
    ('tarland_2004_dynamic', 200, dict(FULL_WAVES, out_slot_order=0, balance=1), False),    # cost-ordered slots, member-order table
    ('tarland_2004_dynamic', 200, dict(FULL_WAVES, time_chunk_days=-1), False),             # the chain kernel
    ('tarland_2004_dynamic', 70, dict(FULL_WAVES, integrator='rk4', substeps=16), False),   # RK4
    ('chain4_val_2004', 150, FULL_WAVES, False),                                            # a 4-reach network
])
def test_ineligible_runs_ignore_the_switch(engine0, monkeypatch, name, E, solver, annual):
    monkeypatch.setenv('SIMPLYP_STREAM_PACK', '1')
    m = perturbed(name, E, out_mask=marshal.MASK_REACH5, solver=solver)
    kw = {}
    rows = m['forcing'].shape[2]
    if annual:
        periods, pod = np.unique(m['met'].index.year.values, return_inverse=True)
        m['opts'].n_periods = rows = len(periods)
        kw['period_of_day'] = np.ascontiguousarray(pod, dtype=np.int32)
    host = engine.pinned_empty((5, rows, m['reach_params'].shape[1], E))
    host[...] = -7.0
    out, status, st = run(engine0, m, host_out=host, **kw)
    assert st['packed_records'] == 0 and st['pack_overflow_blocks'] == 0
    assert np.array_equal(host, out.cpu().numpy(), equal_nan=True)
