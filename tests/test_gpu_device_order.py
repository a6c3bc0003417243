"""The members' lane-slot order computed on the device (simplyp_order.hip.h) against the host's order_members
(SIMPLYP_ORDER_HOST=1): the same blocks by total cost, a permutation that is the same on every run, the same results in member
order bit for bit, and lanes of a wavefront as alike as the host's order makes them."""

import numpy as np
import pytest

import order_model
from simplyp_amd import marshal, synthetic
from test_gpu_stream_packed import perturbed, run

pytestmark = pytest.mark.gpu

BALANCED = dict(balance=1, balance_pilot_days=40, out_slot_order=1)


def ordered_run(engine0, monkeypatch, m, host):
    if host:
        monkeypatch.setenv('SIMPLYP_ORDER_HOST', '1')
    else:
        monkeypatch.delenv('SIMPLYP_ORDER_HOST', raising=False)
    out, status, st = run(engine0, m)
    assert st['balanced'] == 1
    mos = st['member_of_slot'].cpu().numpy()
    got = out.cpu().numpy()
    table = np.empty_like(got)
    table[..., mos] = got                                                # member order
    return mos, table, status.cpu().numpy(), st


def blocks_by_total_cost(mos):
    """order_members' blocks: nb1 = clamp(E / 256, 1, 24), borders at E b / nb1; the members of each as a sorted list."""
    E = len(mos)
    nb1 = max(1, min(24, E // 256))
    return [sorted(mos[E * b // nb1:E * (b + 1) // nb1].tolist()) for b in range(nb1)]


def compare_orders(engine0, monkeypatch, m, E):
    mos, table, status, st = ordered_run(engine0, monkeypatch, m, host=False)
    assert sorted(mos.tolist()) == list(range(E))
    mos2, table2, _, _ = ordered_run(engine0, monkeypatch, m, host=False)
    assert np.array_equal(mos2, mos)
    mos_h, table_h, status_h, st_h = ordered_run(engine0, monkeypatch, m, host=True)
    assert sorted(mos_h.tolist()) == list(range(E))
    assert blocks_by_total_cost(mos) == blocks_by_total_cost(mos_h)
    # order_model's exact block test, the host's order standing for the sorted keys (their low halves are the members): what
    # the sub-blocks (E >= 12288) are cut from.  Inside a block the two may differ where fp32 PC2 values all but tie.
    got, want = order_model.blocks_by_total_cost(mos_h.astype(np.uint64), mos)
    assert len(got) == order_model.shape(E)[0] and all(np.array_equal(a, b) for a, b in zip(got, want))
    assert np.array_equal(table.view(np.uint64), table_h.view(np.uint64)) and np.array_equal(table2.view(np.uint64), table_h.view(np.uint64))
    assert np.array_equal(status, status_h)
    return st, st_h


@pytest.mark.parametrize('E', [1, 63, 300, 6145, 8193, 12288])
def test_device_order_against_host_order(engine0, monkeypatch, E):
    """6145 members: 24 blocks of 256 by total cost, one sub-block each; 300: one block; 63 and 1: less than a wavefront.
    8193: the sort's first stride in global memory; 12288: two sub-blocks per block (one output column: three tables stay small)."""
    m = perturbed('tarland_2004_dynamic', E, out_mask=marshal.MASK_REACH5 if E <= 6145 else 1 << marshal.OUT_COLUMNS.index('Qr'),
                  solver=BALANCED)
    compare_orders(engine0, monkeypatch, m, E)


def test_device_order_on_a_reach_network(engine0, monkeypatch):
    """Three reaches: the pilot is several launches that feed one cost table."""
    m = perturbed('confluence3_nc_2004', 90, out_mask=marshal.MASK_REACH5, solver=BALANCED)
    compare_orders(engine0, monkeypatch, m, 90)


def test_device_order_keeps_the_lanes_alike(engine0, monkeypatch):
    """The bench's Monte-Carlo distribution, 8192 members over two years: SIMT efficiency under the device's order is at most
    0.01 below the host's -- a quarter of what ordering by cost patterns gains over ordering by total cost alone (0.78 -> 0.82,
    order_members' comment).  Measured at this size, where a member is spread over several lanes: 0.4359 under both."""
    pr = synthetic.c3_problem(8192, end_dt='1982-12-31', solver=dict(balance=1, out_slot_order=1))
    st, st_h = compare_orders(engine0, monkeypatch, pr, 8192)
    print('simt_efficiency: device order %.4f, host order %.4f' % (st['simt_efficiency'], st_h['simt_efficiency']))
    assert st['simt_efficiency'] >= st_h['simt_efficiency'] - 0.01
