"""The budgets of tests/budgets.py on tables made without a GPU: (a) the CPU oracle in the closable configuration, every integrator and
option that changes how a day is integrated, day 0 included; (b) the ratio identity and the evapotranspiration bracket on the
reference-made tables of the network scenarios at the workbook's own parameters; (c) all four budgets on a reference-made table of the
closable configuration (tests/golden/confluence3_closable_2004.npz, recipe: tests/golden/make_golden.py --only closable).

The bounds of the linear budgets are budgets.BOUND_FP64 / BOUND_F32: ten times what part (a) measures (`PYTHONPATH=. python tests/test_budgets_host.py`
prints the figures the constants were taken from)."""

import os

import numpy as np
import pytest

import budgets
import helpers
from simplyp_amd import abi, marshal

E = 3

# name -> (solver, step_len)
OPTIONS = {
    'rk4': (dict(integrator='rk4', substeps=96, project_vr=0), 1.0),
    'rk4_half_day': (dict(integrator='rk4', substeps=96, project_vr=0), 0.5),
    'cashkarp_literal': (dict(integrator='cashkarp', project_vr=0), 1.0),
    # (two-day rows: a perturbed member of the stiff chain takes more than the default 4000 attempts at its outlet)
    'cashkarp_literal_two_days': (dict(integrator='cashkarp', project_vr=0, max_steps=100000), 2.0),
    'cashkarp_projected': (dict(integrator='cashkarp', project_vr=1), 1.0),
    'aug': (dict(integrator='cashkarp_aug'), 1.0),
    'aug_tight': (dict(integrator='cashkarp_aug', rtol=1e-11, atol=1e-13), 1.0),
    'aug_pair_on': (dict(integrator='cashkarp_aug', stiff_pair=1), 1.0),
    'aug_pair_off': (dict(integrator='cashkarp_aug', stiff_pair=-1), 1.0),
    'aug_half_day': (dict(integrator='cashkarp_aug'), 0.5),
    'aug_two_days': (dict(integrator='cashkarp_aug', max_steps=100000), 2.0),
    'f32': (dict(integrator='cashkarp_aug_f32', rtol=1e-5, atol=1e-7), 1.0),
}


# the stiff chain's outlet relaxes ~700 times a day, the 5 km2 reaches of the branching network under a perturbed a_Q faster still
RK4_SUBSTEPS_PER_DAY = {'stiff_chain12_2004': 384, 'branch': 1536, 'random3': 384}
DAYS = {'branch': 120}              # 22 reaches, and the option sets with many steps cost 40 s a year on them: the first 120 days


def oracle_case(oracle, name, option):
    """(residuals dict, reaches checked, reaches skipped, reaches of the run, opts) of one scenario and option set on the CPU oracle."""
    solver, step_len = OPTIONS[option]
    if solver['integrator'] == 'rk4':             # classical RK4 is stable for h x rate < 2.78: the same h whatever the row's length
        solver = dict(solver, substeps=int(RK4_SUBSTEPS_PER_DAY.get(name, 96) * step_len))
    m = helpers.budget_problem(name, E, solver=solver, step_len=step_len)
    if name in DAYS:
        m['forcing'], m['doy'] = np.ascontiguousarray(m['forcing'][:, :, :DAYS[name]]), np.ascontiguousarray(m['doy'][:DAYS[name]])
    out, status, _ = oracle.run(m['forcing'], m['doy'], m['member_params'], m['reach_params'], m['up_ptr'], m['up_idx'], m['opts'],
                                n_threads=E)
    assert status.max() == 0 and np.isfinite(out).all(), (name, option)
    args = (out, m['columns'], m['forcing'], m['member_params'], m['reach_params'], m['up_ptr'], m['up_idx'], m['opts'])
    res, checked, skipped = budgets.residuals(*args)
    res['ratio'] = budgets.ratio_identity(*args)[0]
    return res, checked, skipped, m['reach_params'].shape[1], m['opts']


def test_the_bounds_are_what_the_issue_allows():
    for table in (budgets.BOUND_FP64, budgets.MEASURED_FP64):
        assert all(0.0 < v <= budgets.CAP for v in table.values()), table
    assert all(budgets.BOUND_FP64[k] == 10.0 * v for k, v in budgets.MEASURED_FP64.items())
    assert all(budgets.BOUND_F32[k] == 10.0 * v for k, v in budgets.MEASURED_F32.items())


@pytest.mark.parametrize('name', helpers.BUDGET_SCENARIOS)
def test_budgets_close_on_the_oracle(oracle_lib, name):
    """Closable configuration, three members (the scenario's own values but alpha and k_M; two perturbed draws), a year: every budget of
    every (day, reach, member) below its bound -- rounding for the linear ones, 10 x rtol where Vr comes from its invariant."""
    for option in OPTIONS:
        res, checked, skipped, S, opts = oracle_case(oracle_lib, name, option)
        assert (checked, skipped) == (S, 0)
        bound = budgets.bounds(opts, budgets.literal_vr(opts))
        worst = budgets.worst(res)
        day0 = {k: float(np.nanmax(v[0])) for k, v in res.items()}
        assert all(v.shape[1:] == (S, E) and v.shape[0] == DAYS.get(name, 366) for v in res.values())
        for k in budgets.BUDGETS + ('ratio',):
            assert worst[k] < bound[k] and day0[k] < bound[k], (name, option, k, worst[k], day0[k], bound[k])


def golden_out(name, label='tight'):
    """[25, D, S, 1]: the reference-made tables of a golden scenario in the engine's layout."""
    tabs = helpers.golden_tables(name, label)
    scs = sorted(tabs['R'])
    return np.stack([np.stack([(tabs['R'][sc] if c in tabs['R'][sc].columns else tabs['TC'][sc])[c].to_numpy(dtype=float) for sc in scs],
                              axis=1) for c in marshal.OUT_COLUMNS])[..., None]


GOLDEN_RTOL = 1e-12       # odeint's rtol = atol of the 'tight' tables


@pytest.mark.parametrize('name', ['confluence3_nc_2004', 'chain4_val_2004', 'stiff_chain12_2004', 'net5_static_2004',
                                  'net5_static_erod_val_2004', 'net5_dynamic_leakA_2004', 'net5_dynamic_leaknone_2004'])
def test_ratio_identity_and_et_bracket_on_the_reference_tables(name):
    """The workbook's alpha = 1 and k_M = 2 (1.7 on the chain): the PP : sediment input ratio at rounding level, ET strictly inside
    (0, alpha x PET) on every reach and day of the reference's own tables."""
    m = helpers.marshal_scenario(name)
    assert not budgets.closable(m['member_params'])
    args = (golden_out(name), marshal.OUT_COLUMNS, m['forcing'], m['member_params'], m['reach_params'], m['up_ptr'], m['up_idx'], m['opts'])
    S = len(m['scs'])
    ratio, checked, skipped = budgets.ratio_identity(*args)
    assert (checked, skipped) == (S, 0) and ratio.shape == (366, S, 1)
    assert np.nanmax(ratio) < budgets.BOUND_FP64['ratio'], np.nanmax(ratio)
    lower, upper, checked, skipped = budgets.et_bracket(*args)
    assert (checked, skipped) == (S, 0)
    assert lower.min() > -10 * GOLDEN_RTOL and upper.min() > -10 * GOLDEN_RTOL, (lower.min(), upper.min())
    assert lower.min() > 0 and upper.min() > 0, (lower.min(), upper.min())       # measured: strictly inside, without the slack


def closable_fixture():
    z = np.load(os.path.join(helpers.GOLDEN, 'confluence3_closable_2004.npz'), allow_pickle=False)
    m = helpers.marshal_scenario(str(z['scenario']))
    for nm, v in zip((str(n) for n in z['names']), z['values']):
        m['member_params'][marshal.PM_NAMES.index(nm)] = v
    assert [str(c) for c in z['columns']] == marshal.OUT_COLUMNS and [int(r) for r in z['reaches']] == m['scs']
    assert int(z['n_days']) == m['forcing'].shape[2] == 366            # the whole year
    return m, z['out'][..., None]


def test_budgets_close_on_the_reference_made_table():
    """confluence3_nc_2004 with alpha = 0 and k_M = 1 through the unmodified reference (LSODA at rtol = atol = 1e-12, Vr a state of
    its own): a linear multistep method keeps linear invariants as a Runge-Kutta method does, so all four budgets sit at the bounds of
    the fp64 paths -- apart from what LSODA's interpolation to the end of the day leaves, which the measured figures include."""
    m, out = closable_fixture()
    assert budgets.closable(m['member_params'])
    res, checked, skipped = budgets.residuals(out, marshal.OUT_COLUMNS, m['forcing'], m['member_params'], m['reach_params'], m['up_ptr'],
                                              m['up_idx'], m['opts'])
    assert (checked, skipped) == (3, 0)
    worst = budgets.worst(res)
    print('reference-made closable table:', worst)
    for k in budgets.BUDGETS:
        assert worst[k] < budgets.BOUND_FP64[k], (k, worst[k])


def test_a_reach_without_its_upstream_columns_is_skipped_and_counted(oracle_lib):
    """out_reaches = the confluence and one of its two tributaries: the tributary is checked, the confluence is not."""
    m = helpers.budget_problem('confluence3_nc_2004', E, solver=dict(integrator='cashkarp', project_vr=0))
    out, status, _ = oracle_lib.run(m['forcing'], m['doy'], m['member_params'], m['reach_params'], m['up_ptr'], m['up_idx'], m['opts'],
                                    out_reaches=[2, 0])
    res, checked, skipped = budgets.residuals(out, m['columns'], m['forcing'], m['member_params'], m['reach_params'], m['up_ptr'],
                                              m['up_idx'], m['opts'], out_reaches=[2, 0])
    assert (checked, skipped) == (1, 1)
    for k in budgets.BUDGETS:
        assert np.isnan(res[k][:, 0]).all() and np.nanmax(res[k][:, 1]) < budgets.BOUND_FP64[k]


def test_the_module_refuses_the_four_budgets_outside_the_closable_configuration():
    m = helpers.marshal_scenario('confluence3_nc_2004')
    with pytest.raises(ValueError):
        budgets.residuals(golden_out('confluence3_nc_2004'), marshal.OUT_COLUMNS, m['forcing'], m['member_params'], m['reach_params'],
                          m['up_ptr'], m['up_idx'], m['opts'])


def measure(oracle, names=None):
    """The figures behind budgets.MEASURED_*: the worst residual per budget over every case of part (a), fp64 paths with a linear budget
    and the fp32 mirror apart; the worst water residual relative to rtol where Vr comes from its invariant; the ratio identity on the
    same tables."""
    fp64, f32, vr = {}, {}, 0.0
    for name in names or helpers.BUDGET_SCENARIOS:
        for option in OPTIONS:
            res, _, _, _, opts = oracle_case(oracle, name, option)
            w = budgets.worst(res)
            is32 = opts.integrator == abi.INTEG_CASHKARP_AUG_F32
            for k, v in w.items():
                if is32:
                    f32[k] = max(f32.get(k, 0.0), v)
                elif k != 'water' or budgets.literal_vr(opts):
                    fp64[k] = max(fp64.get(k, 0.0), v)
                else:
                    vr = max(vr, v / opts.rtol)
            print('%-28s %-26s %s' % (name, option, {k: '%.2e' % v for k, v in w.items()}), flush=True)
    print('fp64, linear budgets:', fp64)
    print('fp32 stages:', f32)
    print('water with Vr from its invariant, worst residual / rtol: %.3g' % vr)


if __name__ == '__main__':
    from oracle import oracle as _oracle
    _oracle.build()
    import sys
    measure(_oracle, sys.argv[1:])
