"""The refusal census: what every analysis entry of the C ABI answers to a scalar argument it rejects -- return code, error text
and the info struct it was handed -- equals, byte for byte, what the library answered before the entries were moved onto one
entry frame (tests/golden/refusals.json, written by tests/golden/make_refusals.py at that commit).  Every case is refused on the
host: nothing is launched, the test takes milliseconds."""

import ctypes as C
import importlib.util
import json
import os

import pytest

from simplyp_amd import abi, engine

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _census():
    spec = importlib.util.spec_from_file_location('make_refusals', os.path.join(GOLDEN, 'make_refusals.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope='module')
def replayed(engine0):
    import torch
    scratch = torch.zeros(4096, dtype=torch.float64, device=engine0.tdev)
    torch.cuda.synchronize()
    got = _census().replay(engine.lib(), engine0._h, scratch.data_ptr())
    torch.cuda.synchronize()
    assert not bool(scratch.any()), "a refused call wrote to the device"
    return got


@pytest.fixture(scope='module')
def recorded():
    with open(os.path.join(GOLDEN, 'refusals.json')) as fh:
        return json.load(fh)


def test_every_refusal_keeps_its_code_and_text(replayed, recorded):
    assert [(g['entry'], g['case']) for g in replayed] == [(w['entry'], w['case']) for w in recorded]
    for got, want in zip(replayed, recorded):
        print(got['entry'], got['case'], got['rc'], got['error'])
        assert want['rc'] != 0
        assert (got['rc'], got['error']) == (want['rc'], want['error']), (got['entry'], got['case'])


def test_every_analysis_entry_is_in_the_census(recorded):
    skip = {'simplyp_abi_version', 'simplyp_device_count', 'simplyp_ctx_create', 'simplyp_ctx_destroy', 'simplyp_last_error',
            'simplyp_ctx_set_stream', 'simplyp_out_bytes', 'simplyp_run', 'simplyp_run_async', 'simplyp_sync', 'simplyp_plan',
            'simplyp_host_alloc', 'simplyp_host_free', 'simplyp_device_alloc', 'simplyp_device_free', 'simplyp_memcpy_h2d',
            'simplyp_memcpy_d2h', 'simplyp_stream_out', 'simplyp_state_bytes', 'simplyp_set_state', 'simplyp_fetch_packed',
            'simplyp_pack_roundtrip_host', 'simplyp_fetch_packed_pred', 'simplyp_pack_roundtrip_host_pred'}
    assert {w['entry'] for w in recorded} == set(engine.ABI_SYMBOLS) - skip


def test_a_refused_call_leaves_its_info_as_it_was_before(replayed, recorded):
    """... except simplyp_sobol_indices' check of n_rows (1 + n_boot), which comes after the entry has cleared its info and set
    n_resamples: that order is part of the census too."""
    late = ('simplyp_sobol_indices', 'n_rows (1 + n_boot) = 2^32 - 2')
    for got, want in zip(replayed, recorded):
        assert got['info'] == want['info'], (got['entry'], got['case'])
        if got['info'] is not None and (got['entry'], got['case']) != late:
            assert set(bytes.fromhex(got['info'])) == {0xA5}, (got['entry'], got['case'])
    info = abi.SobolInfo.from_buffer_copy(bytes.fromhex(next(g['info'] for g in replayed if (g['entry'], g['case']) == late)))
    assert info.as_dict() == dict(kernel_ms=0.0, counts_ms=0.0, contract_ms=0.0, flops=0, bytes_workspace=0, n_valid=0, n_resamples=2)
    assert C.sizeof(info) == 48
