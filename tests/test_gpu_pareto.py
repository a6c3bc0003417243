"""Pareto counts and ranks on the device (simplyp_pareto through Engine.pareto) against the NumPy statement of the rule
(simplyp_amd/pareto.py).  Every comparison is equality of integers: the rule is comparisons and counts, there is no tolerance.

Sizes are where the kernels can go wrong: E around the wavefront (63, 64, 65) and the workgroup (255, 256, 257), one below, at
and one above the j tile the all-pairs kernel stages in LDS and the j stretch one workgroup takes (abi.PARETO_JTILE,
abi.PARETO_JSPLIT), with M = 1, 2, 3 and 8 (the compiled widths 1, 2, 3, 8; M = 5 and 7 run the padded widths 6 and 8 below)."""

import ctypes as C

import numpy as np
import pytest

from simplyp_amd import abi, engine, pareto

pytestmark = pytest.mark.gpu

ERR_ARG = -1
PATTERN = -77
SIZES = sorted({1, 2, 63, 64, 65, 255, 256, 257, abi.PARETO_JTILE - 1, abi.PARETO_JTILE, abi.PARETO_JTILE + 1,
                abi.PARETO_JSPLIT - 1, abi.PARETO_JSPLIT, abi.PARETO_JSPLIT + 1})
INTS = ('n_used', 'n_fronts', 'n_front0', 'n_unranked', 'pair_tests')
OUTS = ('dominated_by', 'dominates', 'rank')


def dev(eng, a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(eng.tdev)


def check(eng, obj, sense, include=None, max_fronts=0, want=None, what=None, **kw):
    """One call against the statement: the three outputs and the info's integers.  Returns (got, want)."""
    got = eng.pareto(dev(eng, obj), sense, include=include, max_fronts=max_fronts, **kw)
    if want is None:
        want = pareto.ranks(obj, sense, include=include, max_fronts=max_fronts)
    for k in OUTS:
        g = got[k].cpu().numpy()
        assert g.dtype == np.int32 and g.shape == (obj.shape[1],)
        assert np.array_equal(g, want[k]), (what, k, np.flatnonzero(g != want[k])[:8], g[g != want[k]][:8], want[k][g != want[k]][:8])
    for k in INTS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    return got, want


@pytest.mark.parametrize('M', [1, 2, 3, 8])
def test_sizes_around_every_boundary(engine0, M):
    rng = np.random.default_rng(500 + M)
    for k, E in enumerate(SIZES):
        # M = 8 of normals makes nearly everybody non-dominated; two values per objective and a wider set of integers give depth
        obj = rng.standard_normal((M, E)) if k % 2 == 0 else rng.integers(0, 2 if M == 8 else 8, (M, E)).astype(np.float64)
        sense = rng.choice([1, -1], M)
        got, want = check(engine0, obj, sense, what=(M, E))
        assert want['n_used'] == E and want['pair_tests'] >= E * E


@pytest.mark.parametrize('M', [2, 3, 4])
def test_normals_4099(engine0, M):
    obj = np.random.default_rng(1).standard_normal((M, 4099))
    got, want = check(engine0, obj, [1] * M, what=M)
    assert want['n_fronts'] == {2: 121, 3: 33, 4: 16}[M]          # (this seed, counted on the CPU)


def test_padded_widths(engine0):
    rng = np.random.default_rng(57)
    for M in (5, 6, 7):
        check(engine0, rng.integers(0, 3, (M, 1500)).astype(np.float64), rng.choice([1, -1], M), what=M)


def test_heavy_ties_mixed_senses(engine0):
    obj = np.random.default_rng(2).integers(0, 8, (3, 4099)).astype(np.float64)
    got, want = check(engine0, obj, [1, -1, 1])
    assert want['n_fronts'] > 10 and want['n_front0'] > 1


def test_one_front_and_a_chain(engine0):
    # an anti-correlated pair: better in one is worse in the other, so nobody dominates anybody
    x = np.random.default_rng(3).permutation(3000).astype(np.float64)
    got, want = check(engine0, np.stack([x, -x]), [1, 1])
    assert want['n_fronts'] == 1 and want['n_front0'] == 3000 and (want['rank'] == 0).all() and (want['dominates'] == 0).all()
    # a total order: E fronts of one member, the peel loop's stop condition runs E times
    y = np.random.default_rng(4).permutation(600).astype(np.float64)
    got, want = check(engine0, np.stack([y, 2.0 * y]), [-1, -1])
    assert want['n_fronts'] == 600 and want['n_front0'] == 1
    assert np.array_equal(want['rank'], y.astype(np.int32)) and np.array_equal(want['dominates'], 599 - y.astype(np.int32))
    got, want = check(engine0, y[None, :], [1])                        # M = 1
    assert want['n_fronts'] == 600 and np.array_equal(want['dominated_by'], 599 - y.astype(np.int32))


def test_nan_masks_and_member_of_slot(engine0):
    rng = np.random.default_rng(5)
    E = 2500
    obj = rng.integers(0, 6, (3, E)).astype(np.float64)
    obj[rng.integers(0, 3, 300), rng.integers(0, E, 300)] = np.nan      # NaN in one objective of some members
    got, want = check(engine0, obj, [1, 1, -1])
    assert 0 < want['n_used'] < E and (want['rank'] == abi.PARETO_EXCLUDED).sum() == E - want['n_used']
    inc = rng.random(E) < 0.5
    check(engine0, obj, [1, 1, -1], include=inc)
    # nobody takes part: by the mask, and by NaN
    for o, i in ((obj, np.zeros(E, dtype=bool)), (np.full((2, 70), np.nan), None)):
        got, want = check(engine0, o, [1] * o.shape[0] if o.shape[0] == 2 else [1, 1, -1], include=i)
        assert want['n_used'] == 0 and got['n_fronts'] == 0 and bool((got['rank'] == -1).all()) and bool((got['dominates'] == -1).all())
    # the table in a shuffled column order: include and the outputs stay in member order
    mos = rng.permutation(E).astype(np.int32)
    want = pareto.ranks(obj, [1, 1, -1], include=inc)
    got = engine0.pareto(dev(engine0, obj[:, mos]), [1, 1, -1], include=inc, member_of_slot=dev(engine0, mos))
    for k in OUTS:
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    assert all(got[k] == want[k] for k in INTS)


def test_zeros_and_infinities(engine0):
    rng = np.random.default_rng(6)
    obj = rng.choice([0.0, -0.0, 1.0, -1.0], (2, 700))
    got, want = check(engine0, obj, [1, -1])
    same = pareto.ranks(np.where(obj == 0.0, 0.0, obj), [1, -1])         # the two zeros are one value
    assert all(np.array_equal(want[k], same[k]) for k in OUTS)
    obj = rng.choice([np.inf, -np.inf, 0.0, 3.0], (3, 900))             # +inf ties: equal, nobody beats them there
    got, want = check(engine0, obj, [1, 1, -1])
    top = np.flatnonzero((obj[0] == np.inf) & (obj[1] == np.inf) & (obj[2] == -np.inf))
    assert top.size > 1 and (want['rank'][top] == 0).all() and len(set(want['dominates'][top])) == 1


def test_max_fronts_and_no_rank(engine0):
    obj = np.random.default_rng(7).standard_normal((2, 1800))
    full = pareto.ranks(obj, [1, 1])
    assert full['n_fronts'] > 6
    for F in (1, 3):
        got, want = check(engine0, obj, [1, 1], max_fronts=F)
        assert got['n_fronts'] == F and want['n_unranked'] == int((full['rank'] >= F).sum()) > 0
        assert np.array_equal(want['rank'], np.where(full['rank'] >= F, abi.PARETO_UNRANKED, full['rank']))
        assert np.array_equal(got['dominated_by'].cpu().numpy(), full['dominated_by'])
        assert np.array_equal(got['dominates'].cpu().numpy(), full['dominates'])
    # without ranks no front is peeled
    got = engine0.pareto(dev(engine0, obj), [1, 1], rank=False)
    assert 'rank' not in got and got['n_fronts'] == 0 and got['pair_tests'] == 1800 * 1800 and got['n_used'] == 1800
    assert np.array_equal(got['dominated_by'].cpu().numpy(), full['dominated_by'])
    assert np.array_equal(got['dominates'].cpu().numpy(), full['dominates'])
    # ranks alone
    got = engine0.pareto(dev(engine0, obj), [1, 1], counts=False)
    assert 'dominates' not in got and np.array_equal(got['rank'].cpu().numpy(), full['rank']) and got['n_fronts'] == full['n_fronts']


def test_same_call_twice_gives_equal_bits(engine0):
    obj = dev(engine0, np.random.default_rng(8).integers(0, 9, (4, 5000)).astype(np.float64))
    a = engine0.pareto(obj, [1, -1, 1, -1])
    b = engine0.pareto(obj, [1, -1, 1, -1])
    for k in OUTS:
        assert bool((a[k] == b[k]).all()), k
    assert all(a[k] == b[k] for k in INTS)


def test_every_grid_split(engine0):
    """E = 20 011: ten j stretches and 79 workgroups of members in the all-pairs launch, fronts of every size in the peeling."""
    obj = np.random.default_rng(1).standard_normal((3, 20011))
    got, want = check(engine0, obj, [1, -1, 1])
    assert want['n_fronts'] > 30 and want['pair_tests'] > 20011 * 20011


def raw_call(eng, E, M, obj, sense, F, by, of, rank):
    import torch
    L = engine.lib()
    sa = None if sense is None else np.ascontiguousarray(sense, dtype=np.int32)
    info = abi.ParetoInfo()
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(eng.tdev):
        eng._bind_stream()
        rc = L.simplyp_pareto(eng._h, E, M, ptr(obj), None if sa is None else sa.ctypes.data_as(C.POINTER(C.c_int32)), None, None, F,
                              ptr(by), ptr(of), ptr(rank), C.byref(info))
        torch.cuda.synchronize(eng.tdev)
    return rc, L.simplyp_last_error(eng._h).decode()


def test_refusals_write_nothing(engine0):
    import torch
    E, M = 300, 3
    obj = dev(engine0, np.random.default_rng(9).standard_normal((M, E)))
    outs = [torch.full((E,), PATTERN, dtype=torch.int32, device=engine0.tdev) for _ in range(3)]
    ok = [1, -1, 1]
    cases = [(0, M, obj, ok, 0), (-5, M, obj, ok, 0), ((1 << 24) + 1, M, obj, ok, 0), (E, 0, obj, ok, 0), (E, 9, obj, [1] * 9, 0),
             (E, M, None, ok, 0), (E, M, obj, None, 0), (E, M, obj, [1, 0, 1], 0), (E, M, obj, [1, 1, 2], 0), (E, M, obj, ok, -1)]
    for E_, M_, o_, s_, F in cases:
        rc, msg = raw_call(engine0, E_, M_, o_, s_, F, *outs)
        assert rc == ERR_ARG and msg.startswith('simplyp_pareto: '), (rc, msg, E_, M_, F)
        assert all(bool((t == PATTERN).all()) for t in outs), msg
    rc, msg = raw_call(engine0, E, M, obj, ok, 0, None, None, None)
    assert rc == ERR_ARG and msg.startswith('simplyp_pareto: ')
    # one output alone is a call; the others stay as they were
    rc, msg = raw_call(engine0, E, M, obj, ok, 0, None, outs[1], None)
    assert rc == 0 and bool((outs[1] != PATTERN).all()) and bool((outs[0] == PATTERN).all()) and bool((outs[2] == PATTERN).all())
    with pytest.raises(engine.EngineError, match='sense'):
        engine0.pareto(obj, [1, 1, 3])
    for bad in (dict(obj=obj.to(torch.float32), sense=ok), dict(obj=obj[0], sense=[1]), dict(obj=obj, sense=[1, 1]),
                dict(obj=obj, sense=ok, counts=False, rank=False), dict(obj=obj, sense=ok, include=np.ones(E + 1)),
                dict(obj=obj.cpu(), sense=ok)):
        with pytest.raises(ValueError):
            engine0.pareto(**bad)
