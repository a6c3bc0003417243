"""The budgets of tests/budgets.py on the kernel's own tables: water, sediment, PP and TDP of every (day, reach, member) in the closable
configuration (alpha = 0, k_M = 1, ten other parameters perturbed per member) over a covering set of kernel paths, the PP : sediment
ratio identity and the evapotranspiration bracket at the scenarios' own parameters under the default solver, a run resumed from a
saved state, and config C4's chain 256 reaches deep.  No second integration is involved: a budget needs the table and the parameters.

E = 70: one full wave of 64 lanes and a ragged one; 18 quads of four lanes per member.  Bounds: budgets.bounds -- ten times the CPU
oracle's measured rounding-level residual for the linear budgets, 10 x rtol where Vr comes from its invariant (tests/budgets.py).
Every test prints the worst residual per budget, and asserts how many reaches it checked."""

import numpy as np
import pytest

import budgets
import helpers
from simplyp_amd import marshal, synthetic

pytestmark = pytest.mark.gpu

E = 70
SOLVERS = {'rk4': dict(integrator='rk4', substeps=384, project_vr=0), 'cashkarp': dict(integrator='cashkarp', project_vr=0),
           'cashkarp_projected': dict(integrator='cashkarp', project_vr=1), 'aug': dict(integrator='cashkarp_aug'),
           'f32': dict(integrator='cashkarp_aug_f32', rtol=1e-5, atol=1e-7)}
SINGLE = ('tarland_2004_dynamic', 'tarland_2004_dynamic+snow')
# scenario, integrator, lanes per member, time_chunk_days (-1: chain kernel, 64: task queue), stiff_pair, balance = out_slot_order,
# step_len, extra ('' | 'fom': two forcing sets with a per-member index | 'subset': out_reaches leaves reaches out)
COVER = [
    ('tarland_2004_dynamic', 'rk4', 1, -1, -1, 0, 1.0, ''),
    ('tarland_2004_dynamic', 'cashkarp', 1, 64, -1, 1, 2.0, ''),
    ('tarland_2004_dynamic+snow', 'aug', 4, 64, 1, 0, 0.5, ''),
    ('tarland_2004_dynamic', 'aug', 1, -1, -1, 1, 1.0, 'fom'),
    ('tarland_2004_dynamic', 'f32', 1, 64, -1, 0, 1.0, 'subset'),
    ('tarland_2004_dynamic+snow', 'cashkarp_projected', 1, -1, -1, 0, 1.0, ''),
    ('chain4_val_2004', 'rk4', 1, -1, -1, 0, 1.0, ''),
    ('confluence3_nc_2004', 'cashkarp', 1, 64, -1, 1, 2.0, ''),
    ('stiff_chain12_2004+snow', 'aug', 4, 64, 1, 0, 1.0, ''),
    ('branch', 'aug', 1, -1, -1, 0, 0.5, 'fom'),
    ('random1', 'f32', 1, 64, -1, 1, 1.0, ''),
    ('random2', 'aug', 4, -1, 1, 0, 2.0, 'subset'),
    ('random3', 'cashkarp_projected', 1, -1, -1, 0, 1.0, ''),
    ('chain4_val_2004', 'aug', 1, 64, -1, 1, 1.0, 'subset'),
    ('stiff_chain12_2004', 'cashkarp', 1, -1, -1, 0, 1.0, ''),
    # five reaches, new land of both kinds: static EPC0 (constant EPC0 and soil-water concentrations, new land included), dynamic EPC0 with
    # S-type new land while the last sub-catchment is 'A' / has none
    ('net5_static_2004', 'f32', 1, 64, -1, 0, 1.0, ''),
    ('net5_static_erod_val_2004', 'aug', 4, -1, 1, 1, 1.0, ''),
    ('net5_dynamic_leakA_2004', 'aug', 1, 64, -1, 0, 1.0, ''),
    ('net5_dynamic_leaknone_2004', 'aug', 4, 64, 1, 0, 2.0, 'subset'),
]


def test_the_covering_set_covers():
    """Every value of every axis at least once on a network and once on the single reach; every scenario of helpers.BUDGET_SCENARIOS."""
    for where in (True, False):
        cases = [c for c in COVER if (c[0] in SINGLE) == where]
        for axis, values in ((1, ('rk4', 'cashkarp', 'aug', 'f32')), (2, (1, 4)), (3, (-1, 64)), (4, (-1, 1)), (5, (0, 1)), (6, (0.5, 1.0, 2.0)),
                             (7, ('', 'fom', 'subset'))):
            for v in values:
                assert any(c[axis] == v for c in cases), (where, axis, v)
        assert any(c[0].endswith('+snow') for c in cases), where
    assert {c[0].split('+')[0] for c in COVER} == {n.split('+')[0] for n in helpers.BUDGET_SCENARIOS}


def problem(scenario, integ, lanes, chunk, stiff_pair, balance, step_len, extra, closable=True):
    """(problem dict, keywords of the run that the budgets need too)"""
    solver = dict(SOLVERS[integ], lanes_per_member=lanes if integ == 'aug' else 0, time_chunk_days=chunk, stiff_pair=stiff_pair,
                  balance=balance, balance_pilot_days=40 if balance else 0, out_slot_order=balance,
                  max_steps=100000 if step_len > 1 else 4000)           # two-day rows take more attempts than the default cap at a stiff outlet
    if integ == 'rk4':
        solver['substeps'] = int(SOLVERS['rk4']['substeps'] * (4 if scenario == 'branch' else 1) * step_len)
    m = helpers.budget_problem(scenario, E, solver=solver, step_len=step_len, closable=closable)
    kw = {}
    if extra == 'fom':          # a second forcing set: 1.25 x the precipitation, 0.9 x PET; odd members read it
        f2 = m['forcing'].copy()
        f2[:, 0] *= 1.25
        f2[:, 1] *= 0.9
        m['forcing'] = np.ascontiguousarray(np.concatenate([m['forcing'], f2], axis=0))
        kw['forcing_of_member'] = (np.arange(E) % 2).astype(np.int32)
    if extra == 'subset':       # all but the first headwater, downstream first: the reaches it feeds lose their upstream columns
        S = m['reach_params'].shape[1]
        kw['out_reaches'] = list(range(S - 1, 0, -1)) if S > 1 else [0]
    return m, kw


def engine_table(eng, m, kw, **more):
    """(table [n_cols, D, n_out, E] as the run left it, status, stats, budget keywords incl. member_of_slot under out_slot_order)"""
    out, status, stats = eng.run(m['forcing'], m['doy'], m['member_params'], m['reach_params'], m['up_ptr'], m['up_idx'], m['opts'], **kw, **more)
    bkw = dict(kw)
    if m['opts'].out_slot_order:
        bkw['member_of_slot'] = stats['member_of_slot'].cpu().numpy()
    return out.cpu().numpy(), status.cpu().numpy(), stats, bkw


def expected_counts(m, kw):
    """(checked, skipped) from the graph alone: a kept reach is checked when every reach directly upstream of it is kept."""
    S = m['reach_params'].shape[1]
    kept = list(range(S)) if kw.get('out_reaches') is None else list(kw['out_reaches'])
    ok = [all(int(u) in kept for u in m['up_idx'][m['up_ptr'][s]:m['up_ptr'][s + 1]]) for s in kept]
    return sum(ok), len(ok) - sum(ok)


def budget_args(out, m):
    return (out, m['columns'], m['forcing'], m['member_params'], m['reach_params'], m['up_ptr'], m['up_idx'], m['opts'])


def assert_budgets(res, bound, what):
    worst = budgets.worst(res)
    print('budgets %s: %s' % (what, {k: '%.2e' % v for k, v in worst.items()}))
    for k, v in worst.items():
        assert v < bound[k], (what, k, v, bound[k])


@pytest.mark.parametrize('scenario,integ,lanes,chunk,stiff_pair,balance,step_len,extra', COVER)
def test_budgets_close_on_every_kernel_path(engine0, scenario, integ, lanes, chunk, stiff_pair, balance, step_len, extra):
    m, kw = problem(scenario, integ, lanes, chunk, stiff_pair, balance, step_len, extra)
    out, status, stats, bkw = engine_table(engine0, m, kw)
    assert status.max() == 0 and np.isfinite(out).all()
    assert stats['queued'] == (chunk > 0) and stats['balanced'] == balance
    if integ == 'aug':
        assert stats['lanes_per_member'] == lanes and stats['stiff_pair'] == (stiff_pair > 0)
    res, checked, skipped = budgets.residuals(*budget_args(out, m), **bkw)
    res['ratio'] = budgets.ratio_identity(*budget_args(out, m), **bkw)[0]
    assert (checked, skipped) == expected_counts(m, kw) and checked >= 1
    if extra == 'subset' and m['reach_params'].shape[1] > 1:
        assert skipped >= 1
    assert_budgets(res, budgets.bounds(m['opts'], budgets.literal_vr(m['opts'])), (scenario, integ, lanes, chunk, stiff_pair, balance, step_len, extra))


@pytest.mark.parametrize('scenario', helpers.BUDGET_SCENARIOS)
def test_ratio_identity_and_et_bracket_under_the_default_solver(engine0, scenario):
    """The scenario's own members (alpha = 1; k_M = 2, 1.7 on the 4-reach chain), the default solver: the PP : sediment input ratio at
    rounding level, and what left as evapotranspiration inside [0, T x alpha x PET], with 10 x rtol of the term sum as slack."""
    m = helpers.budget_problem(scenario, E, closable=False)
    assert not budgets.closable(m['member_params'])
    out, status, stats, bkw = engine_table(engine0, m, {})
    assert status.max() == 0 and np.isfinite(out).all()
    S = m['reach_params'].shape[1]
    ratio, checked, skipped = budgets.ratio_identity(*budget_args(out, m))
    assert (checked, skipped) == (S, 0)
    lower, upper, checked, skipped = budgets.et_bracket(*budget_args(out, m))
    assert (checked, skipped) == (S, 0)
    print('budgets %s, default solver: ratio %.2e, ET bracket margins %.2e / %.2e' % (scenario, np.nanmax(ratio), lower.min(), upper.min()))
    assert np.nanmax(ratio) < budgets.BOUND_FP64['ratio']
    slack = 10 * m['opts'].rtol
    assert lower.min() > -slack and upper.min() > -slack, (lower.min(), upper.min())


@pytest.mark.parametrize('scenario,chunk', [('tarland_2004_dynamic+snow', -1), ('confluence3_nc_2004', 64)])
def test_budgets_of_a_resumed_run_start_from_the_state(engine0, scenario, chunk):
    """Days [0, 200) with the state saved, then [200, 366) started from it: the first resumed day's budgets close from the state's rows
    (and every later day's from the table), and the state's Vg row is the last day's Qg x T_g, the value the next day starts from."""
    m, kw = problem(scenario, 'cashkarp', 1, chunk, -1, 0, 1.0, '')
    cut = 200
    first = dict(m, forcing=np.ascontiguousarray(m['forcing'][:, :, :cut]), doy=np.ascontiguousarray(m['doy'][:cut]))
    rest = dict(m, forcing=np.ascontiguousarray(m['forcing'][:, :, cut:]), doy=np.ascontiguousarray(m['doy'][cut:]))
    out1, status1, stats1, _ = engine_table(engine0, first, kw, state_out=True)
    state = stats1['state']
    out2, status2, _, _ = engine_table(engine0, rest, kw, state_in=state)
    assert status1.max() == 0 and status2.max() == 0
    st = state.cpu().numpy()
    S = m['reach_params'].shape[1]
    col = m['columns'].index
    T_g = m['member_params'][marshal.PM_NAMES.index('T_g')]
    np.testing.assert_allclose(st[:, budgets.ROW['Vg']], out1[col('Qg'), -1] * T_g[None, :], rtol=4e-16, atol=0)
    for row, c in (('VsA', 'VsA'), ('Vr', 'Vr'), ('Msus', 'Msus_EndOfDay'), ('TDPr', 'TDPr_EndOfDay'), ('PPr', 'PPr_EndOfDay'),
                   ('Plab_A', 'P_labile_A_kg'), ('conc_TDPs_NC', 'conc_TDPs_NC_kgmm')):
        assert np.array_equal(st[:, budgets.ROW[row]], out1[col(c), -1]), row
    res, checked, skipped = budgets.residuals(*budget_args(out2, rest), start=st)
    assert (checked, skipped) == (S, 0)
    bound = budgets.bounds(m['opts'], True)
    assert_budgets({k: v[:1] for k, v in res.items()}, bound, (scenario, 'first resumed day'))
    assert_budgets(res, bound, (scenario, 'resumed'))
    # the same table held against the initial conditions instead of the state does not close on its first day: the check reads the state
    wrong, _, _ = budgets.residuals(*budget_args(out2, rest))
    assert all(np.nanmax(wrong[k][0]) > 1e3 * bound[k] for k in ('water', 'sediment'))


@pytest.mark.parametrize('integ', ['aug', 'cashkarp'])
def test_budgets_close_far_down_the_chain(engine0, integ):
    """Config C4's chain, 256 reaches x 16 members of its own distribution x 64 days, closable: the default solver (the second pair on,
    as on every network) and Cash-Karp alone with Vr integrated literally -- every reach's budgets, the 255 with an upstream reach among
    them, at the same bounds as a single reach."""
    pr = synthetic.c4_problem(16, n_reaches=256, n_days=64, solver=SOLVERS[integ], out_mask=marshal.MASK_ALL, out_reaches=None)
    pr['member_params'] = budgets.make_closable(pr['member_params'])
    pr['columns'] = list(marshal.OUT_COLUMNS)
    out, status, stats, _ = engine_table(engine0, pr, {})
    assert status.max() == 0 and out.shape == (25, 64, 256, 16)
    if integ == 'aug':
        assert stats['stiff_pair'] == 1
    res, checked, skipped = budgets.residuals(*budget_args(out, pr))
    res['ratio'] = budgets.ratio_identity(*budget_args(out, pr))[0]
    assert (checked, skipped) == (256, 0)
    assert_budgets(res, budgets.bounds(pr['opts'], budgets.literal_vr(pr['opts'])), ('c4 chain', integ))
