"""The second-order ratio predictor of the packed output stream with the device as encoder: the pack device function chooses
each span's order and writes the records, the host pool decodes them.  The host table must be the input bit for bit, and records
and counters must be the ones the host's own encoder makes -- a difference between the two sides in the carried ratio, in the
choice of a span's order or in a fall-back shows in one of the two."""

import ctypes as C

import numpy as np
import pytest

from simplyp_amd import engine, marshal
from test_gpu_stream_packed import FULL_WAVES, perturbed, run
from test_pack_order2_host import drifting_table, noisy_table, special_table
from test_pack_rows_host import roundtrip

TABLES = {
    'drifting': drifting_table,                      # [2, 130, 200]: two full chunks and a 2-row one, a ragged last block
    'alternating': lambda: drifting_table(extrapolates=False),
    'noisy': noisy_table,
    'special': special_table,
}


@pytest.mark.gpu
@pytest.mark.parametrize('chunk', [64, 128])         # 128: two spans in a chunk, the ratio carried from one into the next
@pytest.mark.parametrize('members', ['all', 'one'])
@pytest.mark.parametrize('name', sorted(TABLES))
def test_device_encoder_against_host_decoder(engine0, name, members, chunk):
    import torch
    u = TABLES[name]()
    if members == 'one':
        u = np.ascontiguousarray(u[:, :, 100:101])
    n_cols, rows, E = u.shape
    want_out, want_counts, want_bytes = roundtrip(u, pred=[-1, 0], chunk=chunk)
    assert np.array_equal(want_out, u)
    dev = torch.from_numpy(u.view(np.int64)).to(engine0.tdev)
    host = engine.pinned_empty(u.shape)
    host.view(np.uint64)[...] = 7
    counts = (C.c_int32 * 3)()
    nbytes = (C.c_int64 * 2)()
    pc = (C.c_int32 * n_cols)(-1, 0)
    with torch.cuda.device(engine0.tdev):
        rc = engine.lib().simplyp_fetch_packed_pred(engine0._h, dev.data_ptr(), n_cols, rows, E, chunk, pc, C.c_void_p(host.ctypes.data),
                                                    C.c_int64(host.nbytes), counts, nbytes)
    assert rc == 0, engine.lib().simplyp_last_error(engine0._h)
    assert np.array_equal(host.view(np.uint64), u)
    assert list(counts) == want_counts
    assert list(nbytes) == want_bytes


@pytest.mark.gpu
def test_packed_run_delivers_the_device_table(engine0, monkeypatch):
    name, E = 'tarland_2004_dynamic', 192
    m = perturbed(name, E, out_mask=marshal.MASK_REACH5, solver=FULL_WAVES)
    monkeypatch.delenv('SIMPLYP_STREAM_PACK', raising=False)
    ref, ref_status, _ = run(engine0, m)
    ref, ref_status = ref.cpu().numpy(), ref_status.cpu().numpy()
    monkeypatch.setenv('SIMPLYP_STREAM_PACK', '1')
    D = m['forcing'].shape[2]
    host = engine.pinned_empty((5, D, 1, E))
    host[...] = -7.0
    out, status, st = run(engine0, m, host_out=host)
    import torch
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert st['queued'] == 1 and st['lanes_per_wave'] == 64
    assert np.array_equal(host.view(np.uint64), got.view(np.uint64))              # host table = device table
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))              # = the unstreamed run
    assert np.array_equal(status.cpu().numpy(), ref_status)
    assert st['packed_records'] == -(-D // 64) * 5                               # every record packed, none sent raw
    # the records are the host encoder's: the same bytes for the table the device made
    u = np.ascontiguousarray(got[:, :, 0, :]).view(np.uint64)
    pred = [-1] * 5
    pred[marshal.REACH5_COLUMNS.index('PP_kg/day')] = marshal.REACH5_COLUMNS.index('Msus_kg/day')
    out_h, counts_h, _ = roundtrip(u, pred=pred)
    assert np.array_equal(out_h, u) and counts_h[0] == st['packed_records'] and counts_h[1] == st['pack_overflow_blocks']
