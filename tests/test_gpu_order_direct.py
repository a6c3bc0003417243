"""The device's ordering kernels (simplyp_order.hip.h) through their own door, simplyp_order_members, on the cost tables and sizes
of tests/order_model.py: every case through ``check_order`` -- the checker tests/test_order_host.py has put the host rule through
on the CPU --, twice with equal results, and with the host rule's blocks by total cost.  The sizes reach what a model run of
the suite never has: the bitonic sort's strides in global memory (E > 8192; stages with k < P from E = 16385), sub-blocks
(E >= 12288), blocks that fill the LDS sort (E = 196608), the refusal one member above, and a workspace reused after a larger
ensemble."""

import numpy as np
import pytest

import order_model as om
from simplyp_amd import engine

pytestmark = pytest.mark.gpu
MAX_UNCONSTRAINED = 0.01                # as in test_order_host.py: a condition on the pilot-like inputs


def same_bits(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(a, b))


@pytest.mark.parametrize('kind,E', om.CASES, ids=['%s-%d' % c for c in om.CASES])
def test_device_order_is_a_correct_order(engine0, kind, E):
    cost = om.table(kind, E)
    perm, diag, keys = engine0.order_members(cost, diag=True, keys=True)
    ratio = om.check_order(cost, perm, diag, keys)
    print('%s E=%d %s' % (kind, E, ' '.join('%s=%.3g' % kv for kv in sorted(ratio.items()))))
    if kind == 'pilot' and E > 2:
        assert ratio['unconstrained'] <= MAX_UNCONSTRAINED, ratio
    assert same_bits(engine0.order_members(cost, diag=True, keys=True), (perm, diag, keys)), 'a second run differs'
    perm_h, diag_h = engine0.order_members(cost, where='host', diag=True)
    om.check_order(cost, perm_h, diag_h)
    got, want = om.blocks_by_total_cost(cost, perm)
    got_h, _ = om.blocks_by_total_cost(cost, perm_h)
    assert all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(got, got_h, want))


def test_workspace_reused_after_a_larger_ensemble():
    """The entry's workspace only grows: after E = 100000 (P = 131072 keys, 98 workgroups of partial sums) a call at E = 300
    lays its arrays out in the head of the same allocation and must not read what the larger call left behind."""
    big, small = om.table('pilot', 100000), om.table('pilot', 300)
    used, fresh = engine.Engine(0), engine.Engine(0)
    try:
        used.order_members(big)
        got = used.order_members(small, diag=True, keys=True)
        want = fresh.order_members(small, diag=True, keys=True)
    finally:
        used.close()
        fresh.close()
    assert same_bits(got, want)
    om.check_order(small, *got)


def test_one_member_above_the_device_limit(engine0):
    cost = om.table('pilot', om.ORD_MAX_E + 1)
    with pytest.raises(engine.EngineError, match=r'simplyp_order_members: the device orders at most 196608 members \(got 196609\)'):
        engine0.order_members(cost)
    perm, diag = engine0.order_members(cost, where='host', diag=True)
    om.check_order(cost, perm, diag)


def test_arguments_the_entry_refuses(engine0):
    cost = om.table('pilot', 64)
    with pytest.raises(engine.EngineError, match='keys are the device'):
        engine0.order_members(cost, where='host', keys=True)
    with pytest.raises(engine.EngineError, match=r'E must be >= 1 \(got 0\)'):
        engine0.order_members(np.zeros((8, 0), dtype=np.uint32))
