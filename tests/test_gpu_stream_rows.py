"""The row-adaptive records of the packed output stream with the device as encoder: the pack device function writes the records,
the host pool decodes them.  The host table must be the input bit for bit and the records must have the size the host's own
encoder gives them -- any difference between the two sides in the widths or in the fp64 ratio predictor shows in one of the two."""

import ctypes as C

import numpy as np
import pytest

from simplyp_amd import engine, marshal
from test_gpu_stream_packed import FULL_WAVES, made_up_table, perturbed, run
from test_pack_rows_host import U, dependency_table, f2u, predictor_table, roundtrip, smooth

CHUNK = 64


def width_table():
    """[1, 130, 200]: block 1 is constant but for one member a day, whose step makes the row exactly 1, 55, 56, 57, 63 or 64
    bits wide (a day in seven stays at width 0); block 2 is constant throughout."""
    rng = np.random.default_rng(21)
    u = smooth(rng, 1, 130, 200, bits=20)
    u[0, :, 64:192] = U(0x400921FB54442D18)
    with np.errstate(over='ignore'):
        for i, bits in enumerate([1, 55, 56, 57, 63, 64]):
            z = (U(1) << U(bits - 1)) | U(bits > 1)
            delta = (z >> U(1)) ^ (U(0) - (z & U(1)))
            for d in range(1 + i, 130, 7):
                u[0, d:, 64 + i] += delta
    return u


def exact_multiple_table():
    rng = np.random.default_rng(9)
    x = rng.uniform(0.5, 50.0, (70, 130))
    return np.stack([f2u(x), f2u(0.25 * x)])


TABLES = {
    'made_up': (made_up_table, None),
    'widths': (width_table, None),
    'predictor': (predictor_table, [-1, 0]),
    'exact_multiple': (exact_multiple_table, [-1, 0]),
    'dependency': (dependency_table, [-1, 0, -1]),                   # column 0 raw by its counters, column 1 raw because of it
    'one_member': (lambda: np.ascontiguousarray(predictor_table()[:, :, 100:101]), [-1, 0]),
    'two_spans': (lambda: smooth(np.random.default_rng(2), 2, 130, 65), [-1, 0]),      # 128-day chunks: two spans of rows
}


@pytest.mark.gpu
@pytest.mark.parametrize('pinned', [True, False])
@pytest.mark.parametrize('name', sorted(TABLES))
def test_device_encoder_against_host_decoder(engine0, name, pinned):
    import torch
    make, pred = TABLES[name]
    u = make()
    chunk = 128 if name == 'two_spans' else CHUNK
    n_cols, rows, E = u.shape
    want_out, want_counts, want_bytes = roundtrip(u, pred=pred, chunk=chunk)
    assert np.array_equal(want_out, u)
    dev = torch.from_numpy(u.view(np.int64)).to(engine0.tdev)
    host = engine.pinned_empty(u.shape) if pinned else np.empty(u.shape)
    host.view(np.uint64)[...] = 7
    counts = (C.c_int32 * 3)()
    nbytes = (C.c_int64 * 2)()
    pc = None if pred is None else (C.c_int32 * n_cols)(*pred)
    with torch.cuda.device(engine0.tdev):
        rc = engine.lib().simplyp_fetch_packed_pred(engine0._h, dev.data_ptr(), n_cols, rows, E, chunk, pc, C.c_void_p(host.ctypes.data),
                                                    C.c_int64(host.nbytes), counts, nbytes)
    assert rc == 0, engine.lib().simplyp_last_error(engine0._h)
    assert np.array_equal(host.view(np.uint64), u)
    assert list(counts) == want_counts
    assert list(nbytes) == want_bytes


# ---- model runs -----------------------------------------------------------------------------------------------------

def mask_of(columns):
    return sum(1 << marshal.OUT_COLUMNS.index(c) for c in columns)


MASKS = {
    'reach5': marshal.MASK_REACH5,                                                                # PP coded against Msus
    'pp_without_msus': mask_of(['Vr', 'Qr', 'TDP_kg/day', 'PP_kg/day']),                          # predictor off
    # Msus and PP with other columns before and between them: they are columns 4 and 7 of 8, paired by what they are
    'spread': marshal.MASK_REACH5 | mask_of(['VsA', 'Qr_EndOfDay', 'PPr_EndOfDay']),
}


@pytest.mark.gpu
@pytest.mark.parametrize('mask', sorted(MASKS))
def test_packed_run_delivers_the_device_table(engine0, monkeypatch, mask):
    name, E = 'tarland_2004_dynamic', 200                # ragged last block; 366 days: the last chunk has 46
    m = perturbed(name, E, out_mask=MASKS[mask], solver=FULL_WAVES)
    ncols = bin(MASKS[mask]).count('1')
    monkeypatch.delenv('SIMPLYP_STREAM_PACK', raising=False)
    ref, ref_status, _ = run(engine0, m)
    ref, ref_status = ref.cpu().numpy(), ref_status.cpu().numpy()
    monkeypatch.setenv('SIMPLYP_STREAM_PACK', '1')
    D = m['forcing'].shape[2]
    host = engine.pinned_empty((ncols, D, 1, E))
    host[...] = -7.0
    out, status, st = run(engine0, m, host_out=host)
    import torch
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    n_chunks = -(-D // CHUNK)
    assert st['queued'] == 1 and st['lanes_per_wave'] == 64
    assert np.array_equal(host.view(np.uint64), got.view(np.uint64))              # host table = device table
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))              # = the unstreamed run
    assert np.array_equal(status.cpu().numpy(), ref_status)
    assert st['packed_records'] == n_chunks * ncols                              # every record packed, none sent raw
