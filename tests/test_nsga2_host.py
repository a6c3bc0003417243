"""NSGA-II on the CPU: simplyp_amd/nsga2.py's statement of crowding and selection against an independent one written here with
np.lexsort (tests/nsga2_cases.py), the variation of simplyp_amd/csrc/simplyp_nsga2.h in host C++ (tests/nsga2_host_main.cpp, built
with -ffp-contract=off under AddressSanitizer and UBSan, a child process that reads cases as text) against NumPy as hex floats,
the whole loop on ZDT1, the extension header, and what find_pareto refuses on the host.  No GPU needed."""

import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import simplyp_amd as sp
from simplyp_amd import abi, calibrate, engine, nsga2

import host_program
import nsga2_cases as nc
from host_program import rejected

NAN = float('nan')


@pytest.fixture(scope='session')
def driver():
    return host_program.case_runner(host_program.build('nsga2_host_main.cpp', '-ffp-contract=off'), timeout=120)


# ---- crowding and positions ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('M', [1, 2, 3, 8])
def test_crowding_and_positions_equal_an_independent_sort(M):
    rng = np.random.default_rng(700 + M)
    seen_inf = seen_interior = seen_zero_span = False
    for n in (4, 2, 38, 130):
        for name, obj, sense, rank in nc.planted(rng, n, M):
            got = nsga2.crowding(obj, sense, rank)
            nc.same_bits(got, nc.crowding_by_sorting(obj, sense, rank), (name, n, M))
            assert (got[rank < 0] == 0.0).all() and not np.signbit(got).any() and not np.isnan(got).any()
            seen_inf |= bool(np.isinf(got).any())
            seen_interior |= bool((np.isfinite(got) & (got > 0)).any())
            seen_zero_span |= bool(((got == 0.0) & (rank >= 0)).any())
            N = n // 2 if n >= 8 else n
            pos, survivor = nsga2.select(N, rank, got)
            assert np.array_equal(pos, nc.positions_by_sorting(rank, got)), (name, n, M)
            assert sorted(pos) == list(range(n)) and survivor.shape == (N,) and np.array_equal(pos[survivor], np.arange(N))
            n_valid = int((rank >= 0).sum())
            assert int((rank[survivor] < 0).sum()) == max(0, N - n_valid), name       # the invalid survive only to fill up
            r = np.where(rank[survivor] < 0, 1 << 40, rank[survivor].astype(np.int64))
            assert (np.diff(r) >= 0).all() and all(got[survivor][i] >= got[survivor][i + 1] for i in range(N - 1) if r[i] == r[i + 1])
    assert seen_inf and seen_interior and seen_zero_span


def test_crowding_by_hand():
    # one front, M = 2: members sorted by the first objective are 2, 0, 3, 1; by the second (maximised through sense -1) 1, 3, 0, 2
    obj = np.array([[1.0, 4.0, 0.0, 2.0], [3.0, 0.0, 5.0, 1.0]])
    got = nsga2.crowding(obj, [1, -1], np.zeros(4, dtype=np.int32))
    assert got[2] == np.inf and got[1] == np.inf
    assert got[0] == (2.0 - 0.0) / 4.0 + ((-1.0) - (-5.0)) / 5.0 and got[3] == (4.0 - 1.0) / 4.0 + ((-0.0) - (-3.0)) / 5.0
    # -0.0 and +0.0 tie and the index decides; a duplicated member's neighbour is its twin
    obj = np.array([[0.0, -0.0, -0.0, 0.0, 1.0, -1.0]])
    got = nsga2.crowding(obj, [1], np.zeros(6, dtype=np.int32))
    assert np.array_equal(got, [0.5, 0.0, 0.0, 0.5, np.inf, np.inf]) and not np.signbit(got).any()      # order 5 | 0 1 2 3 | 4
    # fronts of one and two members, an invalid member
    got = nsga2.crowding(np.array([[1.0, 2.0, 3.0, NAN]]), [1], np.array([0, 1, 1, -1], dtype=np.int32))
    assert np.array_equal(got, [np.inf, np.inf, np.inf, 0.0])


# ---- the variation: host C++ against NumPy ------------------------------------------------------------------------------------

def h(v):
    return float(v).hex()


def vary_case(a):
    return 'vary %s %s %s %s %d %d %s %d %s' % (h(a[0]), h(a[1]), h(a[2]), h(a[3]), a[4], a[5], h(a[6]), int(a[7]),
                                                  ' '.join(h(u) for u in a[8:]))


def vary_grid():
    tiny, half, one_minus = 2.0 ** -53, 0.5, 1.0 - 2.0 ** -53
    just_above_half = 0.5 + 2.0 ** -53
    boxes = [(0.0, 1.0), (-3.5, 12.25), (200.0, 380.0), (1e-9, 1.7e-9), (1e6, 1e6 * (1 + 2.0 ** -50)), (-1.0, np.nextafter(-1.0, 0.0) + 2e-16)]
    rng = np.random.default_rng(5)
    rows = []
    for lo, hi in boxes:
        mid, q = lo + 0.5 * (hi - lo), lo + 0.25 * (hi - lo)
        pairs = [(lo, hi), (hi, lo), (lo, lo), (hi, hi), (mid, mid), (q, mid), (mid, q), (lo, np.nextafter(lo, hi)), (np.nextafter(hi, lo), hi)]
        pairs += [tuple(lo + (hi - lo) * rng.uniform(size=2)) for _ in range(3)]
        pairs = [(min(max(a, lo), hi), min(max(b, lo), hi)) for a, b in pairs]
        for k in range(1, 6):
            for x1, x2 in pairs:
                for u in (tiny, half, just_above_half, one_minus, float(rng.uniform())):
                    for p_mut, cross in ((1.0, 1), (0.0, 1), (1.0, 0), (0.0, 0), (0.5, 1)):
                        u_take, u_swap = (0.25, 0.75) if rng.uniform() < 0.7 else (float(rng.uniform()), float(rng.uniform()))
                        rows.append((x1, x2, lo, hi, k, 6 - k if k < 5 else 5, p_mut, cross, u, u_take, u_swap,
                                     float(rng.uniform()), u, float(rng.uniform()), 1.0 - u))
    return rows


def test_variation_in_host_cpp_equals_numpy_bit_for_bit(driver):
    rows = vary_grid()
    got = driver([vary_case(r) for r in rows])
    cols = list(zip(*rows))
    arr = lambda i: np.array(cols[i], dtype=np.float64)
    k_c, k_m = np.array(cols[4]), np.array(cols[5])
    want_a, want_b = np.empty(len(rows)), np.empty(len(rows))
    for kc in range(1, 6):
        for km in range(1, 6):
            s = (k_c == kc) & (k_m == km)
            if s.any():
                a, b = nsga2.vary(arr(0)[s], arr(1)[s], arr(2)[s], arr(3)[s], kc, km, arr(6)[s], np.array(cols[7])[s] != 0, arr(8)[s], arr(9)[s],
                                  arr(10)[s], arr(11)[s], arr(12)[s], arr(13)[s], arr(14)[s])
                want_a[s], want_b[s] = a, b
    moved = 0
    for r, (rc, rest), wa, wb in zip(rows, got, want_a, want_b):
        assert rc == 0, rest
        a, b = rest.split()
        assert (float.fromhex(a).hex(), float.fromhex(b).hex()) == (float(wa).hex(), float(wb).hex()), r
        assert r[2] <= wa <= r[3] and r[2] <= wb <= r[3], r                      # inside the closed box, always
        if r[6] == 0.0 and not r[7]:
            assert (wa, wb) == (r[0], r[1]), r                                   # nothing drawn: the parents
        if r[0] == r[1] and r[6] == 0.0:
            assert (wa, wb) == (r[0], r[1]), r                                   # equal parents do not cross
        moved += (wa, wb) != (r[0], r[1])
    assert moved > len(rows) // 3


def test_whole_pairs_without_draws_return_the_parents():
    rng = np.random.default_rng(2)
    lo, hi = np.array([0.0, -2.0, 5.0]), np.array([1.0, 2.0, 9.0])
    theta = lo[:, None] + (hi - lo)[:, None] * rng.uniform(size=(3, 10))
    rank, crowd = np.zeros(10, dtype=np.int32), rng.uniform(size=10)
    off = nsga2.offspring(theta, rank, crowd, 3, lo, hi, p_cross=0.0, p_mut=0.0, seed=9)
    assert np.array_equal(off['child'][:, :5], theta[:, off['parents'][0, :5]])
    assert np.array_equal(off['child'][:, 5:], theta[:, off['parents'][1, 5:]])
    assert np.array_equal(off['parents'][:, :5], off['parents'][:, 5:])
    # a draw depends on (seed, t, pair, dimension) alone: the first pairs of a larger population with the same parents' data
    again = nsga2.offspring(theta, rank, crowd, 3, lo, hi, seed=9)
    assert not np.array_equal(again['child'], off['child']) and np.array_equal(again['child'], nsga2.offspring(theta, rank, crowd, 3, lo, hi, seed=9)['child'])
    assert not np.array_equal(again['child'], nsga2.offspring(theta, rank, crowd, 4, lo, hi, seed=9)['child'])
    assert ((again['child'] >= lo[:, None]) & (again['child'] <= hi[:, None])).all()


def test_tournaments_prefer_rank_then_crowding_then_index():
    N = 64
    rng = np.random.default_rng(3)
    rank = rng.integers(-1, 3, N).astype(np.int32)
    crowd = np.where(rank < 0, 0.0, rng.choice([0.0, 0.5, 0.5, 2.0, np.inf], N))
    par = nsga2.mating(N, 7, rank, crowd, seed=1)
    x = nsga2._draw(1, np.arange(N // 2), 7, nsga2.TOURNAMENT)
    cand = [((w.astype(np.uint64) * np.uint64(N)) >> np.uint64(32)).astype(int) for w in x]
    key = lambda i: (rank[i] if rank[i] >= 0 else 99, -crowd[i], i)
    for p in range(N // 2):
        assert par[0, p] == min(cand[0][p], cand[1][p], key=key) and par[1, p] == min(cand[2][p], cand[3][p], key=key)
    valid_met_invalid = [(a, b) for a, b in zip(cand[0], cand[1]) if (rank[a] < 0) != (rank[b] < 0)]
    assert valid_met_invalid and all(rank[w] >= 0 for w, (a, b) in zip(par[0], zip(cand[0], cand[1])) if (rank[a] < 0) != (rank[b] < 0))


def test_nested_roots_are_the_roots(driver):
    rng = np.random.default_rng(4)
    x = np.concatenate([rng.uniform(0.0, 2.0, 200), 10.0 ** rng.uniform(-300, 300, 200), [1.0, 0.0, 5e-324, 1.7976931348623157e308]])
    for k in range(1, 6):
        got = nsga2.rootk(x, k)
        want = x ** (1.0 / 2 ** k)
        assert (np.abs(got - want) <= 2 * np.spacing(want)).all(), k
        back = nsga2.powk(got, k)
        assert np.allclose(back[x > 1e-300], x[x > 1e-300], rtol=2.0 ** (k - 50), atol=0.0)
    res = driver(['rootk %s %d' % (h(v), k) for v in x[:50] for k in (1, 5)] + ['powk %s %d' % (h(v), k) for v in x[:50] for k in (1, 5)])
    want = [nsga2.rootk(v, k) for v in x[:50] for k in (1, 5)] + [nsga2.powk(v, k) for v in x[:50] for k in (1, 5)]
    with np.errstate(over='ignore'):
        assert [float.fromhex(r[1].strip()).hex() for r in res] == [float(w).hex() for w in want]


# ---- the whole loop -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('seed', range(5))
def test_the_loop_converges_on_zdt1(seed):
    lo, hi = np.zeros(8), np.ones(8)
    first = np.median(nc.zdt1(nsga2.initial_population(64, lo, hi, seed))[1])
    state, records = nsga2.run(lambda x: nc.zdt1(x)[0], 64, 60, [-1, -1], lo, hi, eta_c=15, eta_m=15, seed=seed)
    last = np.median(nc.zdt1(state['theta'])[1])
    print('seed %d: median g %.4f -> %.4f' % (seed, first, last))
    assert first >= 4.0 and last <= 1.05, (seed, first, last)
    assert len(records) == 61 and state['t'] == 60 and ((state['theta'] >= 0.0) & (state['theta'] <= 1.0)).all()
    if seed == 0:                                        # stopped and continued: the same bits
        a, _ = nsga2.run(lambda x: nc.zdt1(x)[0], 64, 25, [-1, -1], lo, hi, seed=seed)
        b, _ = nsga2.run(lambda x: nc.zdt1(x)[0], 64, 35, [-1, -1], lo, hi, seed=seed, state=a)
        for k in ('theta', 'obj', 'crowd'):
            nc.same_bits(b[k], state[k], k)
        assert np.array_equal(b['rank'], state['rank']) and b['t'] == 60


def test_invalid_members_leave_with_the_first_selection():
    lo, hi = np.zeros(4), np.ones(4)

    def f(x):
        obj = nc.zdt1(x)[0]
        obj[1, x[1] > 0.8] = np.nan                      # a corner where the "model" fails
        return obj

    theta0 = nsga2.initial_population(32, lo, hi, 6)
    state, rec = nsga2.new_state(theta0, f(theta0), [-1, -1])
    n_bad = int((theta0[1] > 0.8).sum())
    assert 0 < n_bad < 16 and rec['n_invalid'] == n_bad and (state['rank'][-n_bad:] == -1).all() and (state['rank'][:-n_bad] >= 0).all()
    assert (state['crowd'][-n_bad:] == 0.0).all()
    state, rec = nsga2.step(state, f, [-1, -1], lo, hi, seed=6)
    assert (state['rank'] >= 0).all() and np.isfinite(state['obj']).all()
    assert (np.asarray(rec['all_rank'])[rec['parents'].reshape(-1)] >= 0).sum() >= rec['parents'].size - 4


# ---- the argument checks of the four entries ----------------------------------------------------------------------------------

def test_the_entries_argument_checks(driver):
    good = ['init 4 1 1', 'init 65536 16 1', 'offspring 64 3 1 5 0x0p+0 0x1p+0 1 1 1 1', 'offspring 4 16 4 4 0x1.ccccccccccccdp-1 0x1p-4 1 1 1 1',
            'crowding 1 1 1 1 1 1 1', 'crowding 131072 8 1 1 1 8 1 -1 1 -1 1 -1 1 -1', 'select 8 4 1 1 1 1 0 0 0', 'select 4 4 1 1 1 1 64 1 1',
            'select 131072 65536 1 1 1 1 24 1 1']
    assert [rc for rc, _ in driver(good)] == [0] * len(good)
    bad = ['init 5 1 1', 'init 2 1 1', 'init 0 1 1', 'init 65538 1 1', 'init 64 0 1', 'init 64 17 1', 'init 64 3 0',
           'offspring 63 3 4 4 0x1p-1 0x1p-1 1 1 1 1', 'offspring 64 17 4 4 0x1p-1 0x1p-1 1 1 1 1',
           'offspring 64 3 0 4 0x1p-1 0x1p-1 1 1 1 1', 'offspring 64 3 6 4 0x1p-1 0x1p-1 1 1 1 1', 'offspring 64 3 4 0 0x1p-1 0x1p-1 1 1 1 1',
           'offspring 64 3 4 6 0x1p-1 0x1p-1 1 1 1 1', 'offspring 64 3 4 4 -0x1p-10 0x1p-1 1 1 1 1', 'offspring 64 3 4 4 0x1.0000000000001p+0 0x1p-1 1 1 1 1',
           'offspring 64 3 4 4 nan 0x1p-1 1 1 1 1', 'offspring 64 3 4 4 0x1p-1 nan 1 1 1 1', 'offspring 64 3 4 4 0x1p-1 0x1p+1 1 1 1 1',
           'offspring 64 3 4 4 0x1p-1 -0x1p-1 1 1 1 1', 'offspring 64 3 4 4 0x1p-1 0x1p-1 0 1 1 1', 'offspring 64 3 4 4 0x1p-1 0x1p-1 1 0 1 1',
           'offspring 64 3 4 4 0x1p-1 0x1p-1 1 1 0 1', 'offspring 64 3 4 4 0x1p-1 0x1p-1 1 1 1 0',
           'crowding 0 1 1 1 1 1 1', 'crowding 131073 1 1 1 1 1 1', 'crowding 8 0 1 1 1 1 1', 'crowding 8 9 1 1 1 9 1 1 1 1 1 1 1 1 1',
           'crowding 8 2 0 1 1 2 1 1', 'crowding 8 2 1 0 1 2 1 1', 'crowding 8 2 1 1 0 2 1 1', 'crowding 8 2 1 1 1 null', 'crowding 8 2 1 1 1 2 1 0',
           'crowding 8 2 1 1 1 2 2 1',
           'select 8 5 1 1 1 1 0 0 0', 'select 8 2 1 1 1 1 0 0 0', 'select 3 4 1 1 1 1 0 0 0', 'select 9 4 1 1 1 1 0 0 0', 'select 8 65538 1 1 1 1 0 0 0',
           'select 8 4 0 1 1 1 0 0 0', 'select 8 4 1 0 1 1 0 0 0', 'select 8 4 1 1 0 1 0 0 0', 'select 8 4 1 1 1 0 0 0 0', 'select 8 4 1 1 1 1 -1 0 0',
           'select 8 4 1 1 1 1 65 1 1', 'select 8 4 1 1 1 1 2 0 1', 'select 8 4 1 1 1 1 2 1 0']
    rejected(driver(bad))


def test_eta_is_two_to_the_k_minus_one():
    assert [nsga2.k_of_eta(e) for e in (1, 3, 7, 15, 31)] == [1, 2, 3, 4, 5] and nsga2.k_of_eta(15.0) == 4
    for e in (0, 2, 20, 63, 15.5, NAN, None, 'x'):
        with pytest.raises(ValueError, match=r'must be one of \[1, 3, 7, 15, 31\]'):
            nsga2.k_of_eta(e)


# ---- the extension header and its binding -------------------------------------------------------------------------------------

ENTRIES = ['simplyp_nsga2_init', 'simplyp_nsga2_crowding', 'simplyp_nsga2_select', 'simplyp_nsga2_offspring']


def test_the_extension_header_declares_the_four_entries_and_the_library_exports_them():
    path = os.path.join(engine.INCLUDE, 'simplyp_nsga2.h')
    with open(path) as fh:
        text = fh.read()
    assert set(re.findall(r'\b(simplyp_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', ' ', text, flags=re.S))) == set(ENTRIES)
    assert engine.NSGA2_SYMBOLS == ENTRIES
    assert not set(engine.NSGA2_SYMBOLS) & set(engine.ABI_SYMBOLS) and not set(engine.NSGA2_SYMBOLS) & set(engine.RESIDUALS_SYMBOLS)
    assert len(engine.ABI_SYMBOLS) == 51 and abi.ABI_VERSION == 18
    vp, i32, u32, u64, dbl = C.c_void_p, C.c_int32, C.c_uint32, C.c_uint64, C.c_double
    proto = {name: (restype, argtypes) for name, restype, argtypes in engine.NSGA2_PROTOTYPES}
    assert proto['simplyp_nsga2_init'] == (C.c_int, [vp, i32, i32, u64] + [vp] * 6 + [C.POINTER(abi.McmcInfo)])
    assert proto['simplyp_nsga2_crowding'] == (C.c_int, [vp, i32, i32] + [vp] * 4 + [C.POINTER(abi.ParetoInfo)])
    assert proto['simplyp_nsga2_select'] == (C.c_int, [vp, i32, i32] + [vp] * 4 + [i32] + [vp] * 4 + [C.POINTER(abi.ParetoInfo)])
    assert proto['simplyp_nsga2_offspring'] == (C.c_int, [vp, i32, i32, u64, u32, i32, i32, dbl, dbl] + [vp] * 10 + [C.POINTER(abi.McmcInfo)])
    engine.build()
    L = engine.lib()
    for name, (restype, argtypes) in proto.items():
        assert getattr(L, name).restype is restype and list(getattr(L, name).argtypes) == argtypes, name
    with tempfile.TemporaryDirectory() as tmp:                   # the header stands on its own in C
        src, obj = os.path.join(tmp, 'alone.c'), os.path.join(tmp, 'alone.o')
        with open(src, 'w') as fh:
            fh.write('#include "%s"\nint (*entry_of_the_header)(simplyp_ctx*, int32_t, int32_t, const double*, const int32_t*, const int32_t*, '
                     'double*, simplyp_pareto_info*) = simplyp_nsga2_crowding;\n' % path)
        subprocess.check_call(['gcc', '-Wall', '-Werror', '-c', '-o', obj, src])
    # the mirror's constants are the kernels'
    with open(os.path.join(engine.CSRC, 'simplyp_nsga2.hip.h')) as fh:
        kernels = fh.read()
    assert 'NSGA2_STREAM = 0x%08Xu' % nsga2.STREAM in kernels
    assert 'enum { NSGA2_TOURNAMENT = 0, NSGA2_CROSS, NSGA2_SBX, NSGA2_MUTATE_A, NSGA2_MUTATE_B, NSGA2_INIT };' in kernels
    assert (nsga2.TOURNAMENT, nsga2.CROSS, nsga2.SBX, nsga2.MUTATE_A, nsga2.MUTATE_B, nsga2.INIT) == (0, 1, 2, 3, 4, 5)


# ---- what the public call refuses on the host ---------------------------------------------------------------------------------

OBJ = [('NSE', 'Q'), ('NSE', 'TP'), ('Bias (%)', 'Q')]
BOX = {'fc': (200.0, 380.0), 'T_g': (45.0, 85.0)}


@pytest.mark.parametrize('kw, text', [
    (dict(priors={}), 'priors must be a dict'),
    (dict(priors={'fc': (200.0, 380.0), 'm_Q': (0.01, 1.0)}), "takes no error-model parameter \\('m_Q'\\)"),
    (dict(priors={'fc': (200.0, 380.0), 'phi_Q': (0.0, 0.5)}), "takes no error-model parameter \\('phi_Q'\\)"),
    (dict(priors={'nonsense': (0.0, 1.0)}), "unknown parameter 'nonsense'"),
    (dict(priors={'fc': (380.0, 200.0)}), 'needs lo < hi'),
    (dict(priors={'fc': (NAN, 200.0)}), 'needs lo < hi'),
    (dict(n_pop=None), 'n_pop must be given'),
    (dict(n_pop=63), 'population must be even'),
    (dict(n_pop=2), 'population must be even and in'),
    (dict(n_pop=65538), 'population must be even and in'),
    (dict(objectives=[]), 'between 1 and 8 objectives'),
    (dict(objectives=[('NSE', 'Q')] * 9), 'between 1 and 8 objectives'),
    (dict(objectives=[('spearman', 'Q')]), "takes no 'spearman' objective"),
    (dict(objectives=[('NSE', 'Q'), ('N obs', 'Q')]), 'has no direction of its own'),
    (dict(objectives=[('NSE', 'discharge')]), 'the variable must be one of'),
    (dict(objectives=[('NSE', 'Q', 0, 2)]), 'the sense must be'),
    (dict(objectives=5), 'objectives must be a list'),
    (dict(eta_c=10), r'eta_c must be one of \[1, 3, 7, 15, 31\]'),
    (dict(eta_m=0), r'eta_m must be one of \[1, 3, 7, 15, 31\]'),
    (dict(p_cross=1.5), r'p_cross must be in \[0, 1\]'),
    (dict(p_cross=NAN), r'p_cross must be in \[0, 1\]'),
    (dict(p_mut=-0.1), r'p_mut must be in \[0, 1\]'),
    (dict(seed=-1), 'seed must be in'),
    (dict(n_gen=-1), 'n_gen >= 0'),
])
def test_find_pareto_refuses_before_any_input_is_looked_at(kw, text):
    """The plan comes before the inputs are even looked at: placeholders do for them."""
    args = dict(priors=BOX, objectives=OBJ, n_pop=64, n_gen=2)
    args.update(kw)
    with pytest.raises(ValueError, match=text):
        sp.find_pareto(None, None, None, None, None, None, None, {1: 'observations'}, **args)


def test_find_pareto_needs_observations_and_is_exported():
    assert 'find_pareto' in sp.__all__ and sp.find_pareto is calibrate.find_pareto and sp.nsga2 is nsga2
    with pytest.raises(ValueError, match='find_pareto needs obs_dict'):
        sp.find_pareto(None, None, None, None, None, None, None, None, BOX, OBJ, n_pop=64)


def test_find_pareto_refusals_that_need_the_inputs(monkeypatch):
    """What depends on the data -- the start, a state, the observations behind an objective, a reach index -- is refused on the
    host too: the device ensemble is never built."""
    import helpers

    def no_device(*a, **k):
        raise AssertionError("a device call")
    monkeypatch.setattr(calibrate, '_Evaluator', no_device)
    obs_dict = None

    def call(**kw):
        nonlocal obs_dict
        met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs('tarland_2004_dynamic')
        obs_dict = helpers.observations(p_SU['st_dt'], p_SU['end_dt'])
        args = dict(priors=BOX, objectives=OBJ, n_pop=4, n_gen=1)
        args.update(kw)
        return sp.find_pareto(met, p_struc, p_SU, p_LU, p_SC, p, dyn, obs_dict, **args)

    inside = np.array([[250.0, 300.0, 200.0, 380.0], [45.0, 85.0, 60.0, 70.0]])            # the box is closed: its faces are inside
    with pytest.raises(AssertionError, match='a device call'):
        call(start=inside)
    with pytest.raises(ValueError, match=r'start must have shape \[n_dim, n_pop\]'):
        call(start=inside[:, :3])
    for bad in ((0, 2, 380.5), (1, 0, 44.0), (1, 1, NAN)):
        start = inside.copy()
        start[bad[0], bad[1]] = bad[2]
        with pytest.raises(ValueError, match='the start lies outside the box in %r' % list(BOX)[bad[0]]):
            call(start=start)
    with pytest.raises(ValueError, match='reach_index must be in'):
        call(objectives=[('NSE', 'Q', 3)])
    state = dict(theta=inside, objectives=np.zeros((3, 4)), rank=np.zeros(4, dtype=np.int32), crowd=np.zeros(4), t=2)
    with pytest.raises(AssertionError, match='a device call'):
        call(state=state)
    with pytest.raises(ValueError, match='state does not match this call'):
        call(state=dict(state, objectives=np.zeros((2, 4))))
    with pytest.raises(ValueError, match='state does not match this call'):
        call(state=dict(state, t=-1))
    with pytest.raises(ValueError, match='the state lies outside the box'):
        call(state=dict(state, theta=inside + 200.0))
    with pytest.raises(ValueError, match='generation count must stay below'):
        call(state=dict(state, t=(1 << 32) - 1))
    with pytest.raises(ValueError, match='prior box holds points the model rejects'):
        call(priors={'d_maxE_spr': (20.0, 100.0)})
    # an objective whose variable has too few observations at its reach
    few = {k: v.copy() for k, v in obs_dict.items()}
    few[1].loc[few[1].index[10:], 'SRP'] = np.nan
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs('tarland_2004_dynamic')
    with pytest.raises(ValueError, match='10 or fewer observations'):
        sp.find_pareto(met, p_struc, p_SU, p_LU, p_SC, p, dyn, few, BOX, [('NSE', 'Q'), ('NSE', 'SRP')], n_pop=4)
