"""The kernel at step_len != 1 and on a dry reach network, against tables the unmodified reference made (tests/golden/step_len.npz,
tests/golden/dry_network.npz: tests/golden/make_golden.py --only steplen | drynet), against the CPU oracle, and against itself.

run_simply_p(..., step_len=s) integrates every row over [0, s] (reference model.py:345) while the soil-P update and the upstream
routing keep their one-day forms (model.py:44, :524-528); the kernel's damping-aware error weights (lam * T) and its first trial step
(h_carry = step_len / substeps) scale with the span.  Tolerances are test_gpu_parity.py's.
"""

import numpy as np
import pytest

import helpers
import simplyp_amd as sp
from simplyp_amd import marshal

pytestmark = pytest.mark.gpu

CASES = list(range(6))      # tarland_2004_dynamic at 0.5 and 2, chain4_val_2004 at 0.5 and 2, stiff_chain12_2004 at 0.25 and 2
REACH_COLS = helpers.REACH_COLS
FLOOR = 1e-12


def gpu_run(eng, m, **kw):
    out, status, stats = eng.run(m['forcing'], m['doy'], m['member_params'], m['reach_params'],
                                 m['up_ptr'], m['up_idx'], m['opts'], **kw)
    return out.cpu().numpy(), status.cpu().numpy(), stats


def cpu_run(oracle_lib, m, **kw):
    return oracle_lib.run(m['forcing'], m['doy'], m['member_params'], m['reach_params'],
                          m['up_ptr'], m['up_idx'], m['opts'], **kw)


@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('lanes', [1, 4])
def test_default_solver_at_step_len_against_the_reference(engine0, case, lanes):
    """Default solver, one and four lanes per member: north_star's bar on every reach column of every reach (oracle: 5e-8 ... 3.0e-7)."""
    m, tables = helpers.steplen_problem(case, solver=dict(lanes_per_member=lanes))
    got, status, stats = gpu_run(engine0, m)
    assert status.max() == 0 and stats['lanes_per_member'] == lanes
    errs = helpers.steplen_errors(got, m['scs'], tables, marshal.OUT_COLUMNS)
    assert max(errs[c] for c in REACH_COLS) < 1e-6, (m['name'], m['step_len'], errs)


@pytest.mark.parametrize('case', [c for c in CASES if helpers.steplen_cases()[c][0] == 'tarland_2004_dynamic'])
def test_run_simply_p_drop_in_at_step_len(engine0, case):
    """sp.run_simply_p(..., step_len=s) on the reference's inputs: the 25 raw columns the fixture stores, at the drop-in test's bars."""
    name, step_len = helpers.steplen_cases()[case]
    _, tables = helpers.steplen_problem(case)
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(name)
    df_TC, df_R, Kf, output_dict = sp.run_simply_p(met, p_struc, p_SU, p_LU, p_SC, p, dyn, step_len=step_len)
    assert output_dict['member_status'] == 0
    (sc, table), = tables.items()
    assert len(table) == 25
    for c, ref in table.items():
        got = (df_R[sc] if c in df_R[sc].columns else df_TC[sc])[c].values
        tol = 2e-5 if c in ('QsA', 'QsS', 'QsNC') else 1e-6
        assert helpers.max_rel_err(got, ref, floor=1e-9 if c not in REACH_COLS else 1e-300) < tol, (c, step_len)


# RK4 steps per row: stable for h x rate < 2.78.  The reference routes the upstream reach's integral over the row into the next reach as
# a per-day rate (model.py:524-528), so at step_len = 2 the flow doubles from reach to reach: the 4-reach chain needs 128 steps, and the
# stiff chain's outlet reaches ~1e6 mm/d (2 ** 11 x) -- no fixed step count is stable there below ~16 000 (measured with the oracle).
# The literal 12-variable Cash-Karp needs more than its 4000 attempts per row there (the member is flagged).  Neither is run on that
# case; the augmented Cash-Karp and the default scheme (both with the second pair) are.
RK4_SUBSTEPS = {0: 32, 1: 32, 2: 32, 3: 128, 4: 384}
ORACLE_SOLVERS = {
    'rk4': (dict(integrator='rk4'), 1e-10),
    'cashkarp@1e-11': (dict(integrator='cashkarp', rtol=1e-11, atol=1e-13), 1e-9),
    'cashkarp_aug@1e-11': (dict(integrator='cashkarp_aug', rtol=1e-11, atol=1e-13), 1e-9),
    'default': (None, helpers.TOL_WORKING)}


@pytest.mark.parametrize('case,solver', [(c, s) for c in CASES for s in ORACLE_SOLVERS
                                         if not (c == 5 and s in ('rk4', 'cashkarp@1e-11'))])
def test_kernel_matches_oracle_at_step_len(engine0, oracle_lib, case, solver):
    """test_kernel_matches_oracle at step_len != 1: every column within the tolerance, and the same number of right-hand sides to
    0.5 % -- what a kernel-only change to a span-dependent rule (the damping-aware weights' lam * T, the first trial step) would break
    even where the result stays within the bar."""
    solver, tol = ORACLE_SOLVERS[solver]
    if solver and solver['integrator'] == 'rk4':
        solver = dict(solver, substeps=RK4_SUBSTEPS[case])
    m, _ = helpers.steplen_problem(case, E=3, solver=solver)
    m['member_params'][marshal.PM_NAMES.index('fc')] *= np.array([1.0, 0.9, 1.1])
    got, status, stats = gpu_run(engine0, m)
    ref, rstatus, rstats = cpu_run(oracle_lib, m)
    assert status.max() == 0 and rstatus.max() == 0
    for ci, c in enumerate(marshal.OUT_COLUMNS):
        err = helpers.max_rel_err(got[ci], ref[ci], floor=FLOOR)
        assert err < tol, (c, err)
    assert abs(stats['rhs_evals'] - rstats['rhs_evals']) <= 0.005 * rstats['rhs_evals'], (stats['rhs_evals'], rstats['rhs_evals'])


@pytest.mark.parametrize('lanes', [1, 4])
def test_first_trial_step_is_step_len_over_substeps(engine0, oracle_lib, lanes):
    """The first day's first trial step is step_len / substeps (h_carry; later days carry the last accepted step): on a one-day run of
    Tarland at step_len = 2 the number of right-hand sides depends on it (the oracle with 16 substeps takes a different count), and the
    kernel, one and four lanes per member, takes exactly the oracle's count -- which the 0.5 % bar of a year-long run cannot see."""
    m, _ = helpers.steplen_problem(1, E=3, solver=dict(lanes_per_member=lanes))
    assert m['step_len'] == 2.0
    m['member_params'][marshal.PM_NAMES.index('fc')] *= np.array([1.0, 0.9, 1.1])
    m['forcing'] = np.ascontiguousarray(m['forcing'][:, :, :1])
    m['doy'] = np.ascontiguousarray(m['doy'][:1])
    got, status, stats = gpu_run(engine0, m)
    ref, rstatus, rstats = cpu_run(oracle_lib, m)
    assert status.max() == 0 and rstatus.max() == 0 and stats['lanes_per_member'] == lanes
    assert helpers.max_rel_err(got, ref, floor=FLOOR) < helpers.TOL_WORKING
    assert stats['rhs_evals'] == rstats['rhs_evals'], (stats['rhs_evals'], rstats['rhs_evals'])
    m['opts'].substeps *= 2
    _, _, half = cpu_run(oracle_lib, m)
    assert half['rhs_evals'] != rstats['rhs_evals']


@pytest.mark.parametrize('case', [0, 1, 2, 3])
def test_fp32_stage_mode_against_its_oracle_mirror_at_step_len(engine0, oracle_lib, case):
    """test_fp32_stage_mode_against_its_oracle_mirror at step_len != 1 (single reach and the 4-reach chain; the fp32 mode has no second
    pair for the stiff chain): 10 x rtol on 99 % of the values, 5e-4 on all, right-hand sides within 1 %."""
    rtol = 1e-5
    m, _ = helpers.steplen_problem(case, E=3, solver=dict(integrator='cashkarp_aug_f32', rtol=rtol, atol=1e-7))
    m['member_params'][marshal.PM_NAMES.index('fc')] *= np.array([1.0, 0.9, 1.1])
    got, status, stats = gpu_run(engine0, m)
    ref, ref_status, ref_stats = cpu_run(oracle_lib, m)
    assert status.max() == 0 and ref_status.max() == 0
    cols = [marshal.OUT_COLUMNS.index(c) for c in ('Qr', 'Qr_EndOfDay', 'Msus_kg/day', 'TDP_kg/day', 'PP_kg/day', 'Vr', 'VsA', 'VsS', 'Vg')]
    rel = np.abs(got[cols] - ref[cols]) / np.maximum(np.abs(ref[cols]), 1e-12)
    assert np.percentile(rel, 99) < 10 * rtol and rel.max() < 5e-4, (np.percentile(rel, 99), rel.max())
    assert abs(stats['rhs_evals'] - ref_stats['rhs_evals']) < 0.01 * ref_stats['rhs_evals']


@pytest.mark.parametrize('name', ['tarland_2004_dynamic', 'chain4_val_2004', 'stiff_chain12_2004'])
def test_four_lanes_equal_one_lane_at_step_len_2(engine0, name):
    """ck_day_quad against ck_day at step_len = 2, default solver (the second pair on for the networks): bit for bit."""
    m = helpers.marshal_scenario(name, E=20, solver=dict(lanes_per_member=1))
    m['opts'].step_len = 2.0
    m['member_params'][marshal.PM_NAMES.index('a_Q')] *= np.linspace(0.6, 1.6, 20)
    one, s1, st1 = gpu_run(engine0, m)
    m['opts'].lanes_per_member = 4
    four, s4, st4 = gpu_run(engine0, m)
    assert st1['lanes_per_member'] == 1 and st4['lanes_per_member'] == 4 and s1.max() == 0
    assert np.array_equal(one, four, equal_nan=True) and np.array_equal(s1, s4)
    assert st1['rhs_evals'] == st4['rhs_evals'] and st1['rejected'] == st4['rejected']


@pytest.mark.parametrize('name', ['tarland_2004_dynamic', 'chain4_val_2004'])
def test_task_queue_kernel_at_step_len_2_is_bitwise_identical(engine0, name):
    """The task-queue kernel hands a member's state and its next trial step (h_carry, first set to step_len / substeps) over between
    time chunks; at step_len = 2 over 3 chunks of 256 days, with and without the cost-sorted member order: the chain kernel's
    results bit for bit (one reach: the queue of independent members; the 4-reach chain: the pipelined queue)."""
    E = 150
    m = helpers.marshal_scenario(name, E=E, solver=dict(time_chunk_days=-1, balance=0))
    m['opts'].step_len = 2.0
    m['forcing'] = np.ascontiguousarray(np.tile(m['forcing'], (1, 1, 2)))          # 732 days = 3 chunks of 256
    m['doy'] = np.ascontiguousarray(np.tile(m['doy'], 2))
    rng = np.random.default_rng(41)
    for pname, lo, hi in (('a_Q', 0.6, 1.6), ('T_s_A', 0.5, 2.0), ('fc', 0.8, 1.2)):
        m['member_params'][marshal.PM_NAMES.index(pname)] *= rng.uniform(lo, hi, E)
    ref, sref, st0 = gpu_run(engine0, m)
    assert st0['queued'] == 0 and sref.max() == 0
    for balance in (0, 1):
        m['opts'].time_chunk_days = 256
        m['opts'].balance = balance
        m['opts'].balance_pilot_days = 80
        got, sgot, st = gpu_run(engine0, m)
        assert st['queued'] == 1 and st['balanced'] == balance
        assert np.array_equal(got, ref, equal_nan=True) and np.array_equal(sgot, sref), balance
        assert st['rhs_evals'] == st0['rhs_evals']


@pytest.mark.parametrize('lanes', [1, 4])
def test_default_solver_on_a_dry_reach_network_against_the_reference(engine0, lanes):
    """tests/golden/dry_network.npz (members of config C4's draw, upper 32 reaches of its chain, 1981-1982, 0.6 x precipitation and
    PET / 0.6, the unmodified reference at odeint (1e-12, 1e-15)): chain kernel, default solver with the second pair, one and four
    lanes per member -- north_star's bar on every kept reach, each member's worst reach of the selection sweep included (oracle: 6.8e-7).
    The pipelined task queue gives the chain kernel's results bit for bit."""
    pr, tables = helpers.dry_network_problem(solver=dict(lanes_per_member=lanes, time_chunk_days=-1))
    got, status, stats = gpu_run(engine0, pr, out_reaches=pr['out_reaches'])
    assert status.max() == 0 and stats['lanes_per_member'] == lanes and stats['stiff_pair'] == 1 and stats['queued'] == 0
    worst = helpers.c4_members_worst(got, tables)
    assert max(worst.values()) < 1e-6, worst
    pr['opts'].time_chunk_days = 256
    piped, pstatus, pstats = gpu_run(engine0, pr, out_reaches=pr['out_reaches'])
    assert pstats['queued'] == 1 and pstats['stiff_pair'] == 1
    assert np.array_equal(piped, got, equal_nan=True) and np.array_equal(pstatus, status)
    assert pstats['rhs_evals'] == stats['rhs_evals']
