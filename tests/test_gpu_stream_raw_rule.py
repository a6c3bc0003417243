"""Which records of the packed output stream travel raw, with the device as encoder (tests/test_pack_raw_rule_host.py has
the rule and the tables).  The device's counters feed the same router: a small record with more overflow blocks than the
capacity allows for travels packed, through simplyp_fetch_packed and in a streamed model run alike."""

import ctypes as C

import numpy as np
import pytest

from simplyp_amd import engine, synthetic
from test_gpu_stream_packed import CHUNK, FULL_WAVES, run
from test_pack_raw_rule_host import MODEL_DAYS, MODEL_E, MODEL_END, MODEL_SEED, jump_table


@pytest.mark.gpu
def test_jump_table_through_the_device_packer(engine0):
    import torch
    u = jump_table()
    dev = torch.from_numpy(u.view(np.int64)).to(engine0.tdev)
    host = engine.pinned_empty(u.shape)
    host.view(np.uint64)[...] = 7
    counts = (C.c_int32 * 3)()
    with torch.cuda.device(engine0.tdev):
        rc = engine.lib().simplyp_fetch_packed(engine0._h, dev.data_ptr(), 2, 130, 200, CHUNK, C.c_void_p(host.ctypes.data),
                                               C.c_int64(host.nbytes), counts)
    assert rc == 0, engine.lib().simplyp_last_error(engine0._h)
    assert np.array_equal(host.view(np.uint64), u)
    assert list(counts) == [6, 8, 0]


@pytest.mark.gpu
def test_streamed_model_run_has_no_raw_record(engine0, monkeypatch):
    """256 members of the C3 draw, 1408 days = 22 chunks: under the count rule two Msus records and their PP records went raw.
    The members are in slot order here, so the overflow-block count is the run's own; it is printed, not pinned."""
    import torch
    monkeypatch.setenv('SIMPLYP_STREAM_PACK', '1')
    pr = synthetic.c3_problem(MODEL_E, end_dt=MODEL_END, seed=MODEL_SEED, solver=FULL_WAVES)
    assert pr['forcing'].shape[2] == MODEL_DAYS
    host = engine.pinned_empty((5, MODEL_DAYS, 1, MODEL_E))
    host[...] = -7.0
    out, status, st = run(engine0, pr, host_out=host)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    print('packed_records %d (raw %d), overflow blocks %d' % (st['packed_records'] & 0xFFFF, st['packed_records'] >> 16,
                                                             st['pack_overflow_blocks']))
    assert int(status.cpu().numpy().max()) == 0
    assert st['queued'] == 1 and st['lanes_per_wave'] == 64
    assert np.array_equal(host.view(np.uint64), got.view(np.uint64))              # host table = device table
    assert st['packed_records'] == 110                                           # 22 chunks x 5 columns packed, none raw
