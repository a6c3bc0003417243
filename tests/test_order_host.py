"""The host rule of the members' lane-slot order (order_members, simplyp_amd/csrc/simplyp_order.h) against the statement of a
correct order in tests/order_model.py, on the CPU: tests/order_host_main.cpp includes the header, is built once per session with
the host compiler under AddressSanitizer and UBSan, and runs as a child process per cost table.  Every table and size that
tests/test_gpu_order_direct.py puts to the device's kernels goes through the same ``check_order`` here first, which also shows
that the checker's derived bounds hold for a rule that is known to be right -- and, with three wrong orders made from a right one,
that it does not pass by looseness."""

import subprocess

import numpy as np
import pytest

import host_program
import order_model as om

MAX_UNCONSTRAINED = 0.01                # of the adjacent pairs of a pilot-like table: a condition on the INPUTS (change them, not this)
_done = {}


@pytest.fixture(scope='session')
def host_order(tmp_path_factory):
    """run(cost) -> (perm, diag) of the stand-alone host program; the sanitizers abort the child on any finding."""
    work = tmp_path_factory.mktemp('order_host')
    exe = host_program.build('order_host_main.cpp', '-pthread')

    def run(cost):
        E = cost.shape[1]
        src, dst = str(work / 'cost.bin'), str(work / 'out.bin')
        np.ascontiguousarray(cost, dtype=np.uint32).tofile(src)
        p = subprocess.run([exe, str(E), src, dst], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and p.stderr == '', p.stderr
        raw = open(dst, 'rb').read()
        assert len(raw) == 4 * E + 8 * om.DIAG
        return np.frombuffer(raw, dtype=np.int32, count=E).copy(), np.frombuffer(raw, dtype=np.float64, offset=4 * E).copy()
    return run


def host_case(host_order, kind, E):
    """(cost, perm, diag) of one case, computed once per session."""
    if (kind, E) not in _done:
        cost = om.table(kind, E)
        _done[(kind, E)] = (cost,) + host_order(cost)
    return _done[(kind, E)]


@pytest.mark.parametrize('kind,E', om.CASES, ids=['%s-%d' % c for c in om.CASES])
def test_host_rule_gives_a_correct_order(host_order, kind, E):
    cost, perm, diag = host_case(host_order, kind, E)
    ratio = om.check_order(cost, perm, diag)
    print('%s E=%d %s' % (kind, E, ' '.join('%s=%.3g' % kv for kv in sorted(ratio.items()))))
    if kind == 'pilot' and E > 2:
        assert ratio['unconstrained'] <= MAX_UNCONSTRAINED, ratio


def test_shapes_the_sizes_are_chosen_for():
    assert om.shape(12287) == (24, 1) and om.shape(12288) == (24, 2) and om.shape(36864) == (24, 6) and om.shape(196608) == (24, 6)
    assert om.shape(6143) == (23, 1) and om.shape(6144) == (24, 1) and om.shape(255) == (1, 1) and om.shape(511) == (1, 1)
    assert om.ORD_MAX_E == 196608 and {hi - lo for b, c, lo, hi in om.spans(196608)} == {8192 // 6, 8192 // 6 + 1}
    assert max(E for _, E in om.CASES) == om.ORD_MAX_E


def _refused(cost, perm, diag):
    with pytest.raises(AssertionError):
        om.check_order(cost, perm, diag)


def test_checker_refuses_wrong_orders(host_order):
    """A right order made wrong in the ways a kernel could get it wrong, each still a valid permutation."""
    cost, perm, diag = host_case(host_order, 'pilot', 12288)
    spans = om.spans(12288)
    b, c, lo, hi = spans[3]                                     # block 1, sub-block 1: direction (1 * 2 + 1) % 2, not 1 % 2
    assert (b, c) == (1, 1)
    wrong = perm.copy()
    wrong[lo:hi] = perm[lo:hi][::-1]                            # the sub-block's direction taken from b alone
    _refused(cost, wrong, diag)
    wrong = perm.copy()
    wrong[[0, 12287]] = perm[[12287, 0]]                        # a member of the cheapest block in the dearest
    _refused(cost, wrong, diag)
    wrong = perm.copy()
    b, c, lo, hi = spans[0]
    b2, c2, lo2, hi2 = spans[1]
    wrong[lo:hi2] = np.r_[perm[lo2:hi2], perm[lo:hi]]           # the sub-blocks of block 0 in PC2's other direction
    _refused(cost, wrong, diag)
    wrong = perm.copy()
    wrong[lo:hi] = np.roll(perm[lo:hi], 1)                      # one member out of place in PC3
    _refused(cost, wrong, diag)
    bad = diag.copy()
    bad[2 * om.WIN + om.N_COV:3 * om.WIN + om.N_COV] = diag[3 * om.WIN + om.N_COV:]      # v2 and v3 exchanged
    bad[3 * om.WIN + om.N_COV:] = diag[2 * om.WIN + om.N_COV:3 * om.WIN + om.N_COV]
    _refused(cost, perm, bad)
    bad = diag.copy()
    bad[0] += 4 * om.DELTA                                      # a mean that is off by more than fp32 allows
    _refused(cost, perm, bad)
    cost, perm, diag = host_case(host_order, 'twelve_rows', 257)
    same = np.flatnonzero(np.all(cost[:, perm[1:]] == cost[:, perm[:-1]], axis=0))
    assert len(same) > 100                                      # heavy ties: most neighbours share all eight costs
    wrong = perm.copy()
    wrong[[same[0], same[0] + 1]] = perm[[same[0] + 1, same[0]]]
    _refused(cost, wrong, diag)                                 # the member id did not decide
    keys = np.sort(om.total_keys(cost))
    om.check_order(cost, perm, diag, keys)
    keys[[5, 6]] = keys[[6, 5]]
    with pytest.raises(AssertionError):
        om.check_order(cost, perm, diag, keys)


@pytest.mark.gpu
@pytest.mark.parametrize('kind,E', [('pilot', 300), ('twelve_rows', 12289), ('wrap', 36864), ('pilot', om.ORD_MAX_E + 1)])
def test_library_host_rule_equals_the_standalone_program(engine0, host_order, kind, E):
    """simplyp_order_members with where = 1 runs the header's rule on a copy of the costs: the same permutation and the same 68
    doubles as the stand-alone program, bit for bit."""
    cost = om.table(kind, E)
    perm, diag = host_order(cost)
    got_perm, got_diag = engine0.order_members(cost, where='host', diag=True)
    assert np.array_equal(got_perm, perm)
    assert np.array_equal(got_diag.view(np.uint64), diag.view(np.uint64))
