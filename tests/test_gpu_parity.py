"""Parity tests proper: the HIP engine, called through the C ABI (simplyp_amd.engine -> libsimplyp_hip.so),
against the CPU oracle on the same seeded inputs, against the golden fixtures recorded from the reference,
and -- at BASELINE.json's full sizes -- through size-independent properties.

Tolerances (fp64):
  * kernel vs oracle, fixed-step RK4 (no data-dependent control flow): 1e-10 relative;
  * kernel vs oracle, Cash-Karp (identical step-size rule; an accept/reject decision may flip on a rounding
    difference, after which the two runs are two valid integrations at the same rtol): 1e-9 at rtol 1e-11,
    10 x rtol at working tolerances;
  * kernel vs reference odeint(rtol=atol=1e-12), default solver: 1e-6 relative on every reach output
    (north_star's bar).
Reduced precision (integrator 'cashkarp_aug_f32', BASELINE config C5: fp32 stages, fp64 daily integrals and soil P):
not a parity-grade mode; 5e-4 relative against the reference at rtol 1e-5 (the error is the tolerance's, the fp64
scheme at the same rtol has the same), stated in test_fp32_stage_mode.
"""

import numpy as np
import pandas as pd
import pytest

import helpers
import simplyp_amd as sp
from simplyp_amd import abi, engine, ensemble, marshal, synthetic

pytestmark = pytest.mark.gpu

SCENARIOS = ['tarland_2004_static', 'tarland_2004_dynamic', 'confluence3_nc_2004', 'chain4_val_2004', 'stiff_chain12_2004',
             # five reaches with new land of both kinds: static EPC0 (the EPC0 of new land selected by the reach's own type, constant all
             # year), and S-type new land whose day boundary runs on the hydrology of the last sub-catchment's type ('A' / none)
             'net5_static_2004', 'net5_static_erod_val_2004', 'net5_dynamic_leakA_2004', 'net5_dynamic_leaknone_2004']
REACH_COLS = ['Vr', 'Qr_EndOfDay', 'Qr', 'Msus_EndOfDay', 'Msus_kg/day', 'TDPr_EndOfDay', 'TDP_kg/day',
              'PPr_EndOfDay', 'PP_kg/day']
FLOOR = 1e-12      # columns that are identically 0 (e.g. NC columns without NC land) compare absolutely


def gpu_run(eng, m, **kw):
    out, status, stats = eng.run(m['forcing'], m['doy'], m['member_params'], m['reach_params'],
                                 m['up_ptr'], m['up_idx'], m['opts'], **kw)
    return out.cpu().numpy(), status.cpu().numpy(), stats


def cpu_run(oracle_lib, m, **kw):
    return oracle_lib.run(m['forcing'], m['doy'], m['member_params'], m['reach_params'],
                          m['up_ptr'], m['up_idx'], m['opts'], **kw)


def test_native_library_is_the_one_running(engine0):
    """The ops fail loudly without the extension; here it must be loaded from the tree."""
    import os
    assert os.path.samefile(engine.LIB_PATH, os.path.join(engine.CSRC, 'libsimplyp_hip.so'))
    with open('/proc/self/maps') as fh:
        assert 'libsimplyp_hip.so' in fh.read()
    assert engine.lib().simplyp_device_count() >= 1


@pytest.mark.parametrize('name', SCENARIOS)
@pytest.mark.parametrize('solver,tol', [
    # fixed step: no data-dependent control flow -> rounding-level agreement
    (dict(integrator='rk4', substeps=32), 1e-10),
    (dict(integrator='rk4', substeps=32, project_vr=0), 1e-10),
    # adaptive at a very tight tolerance: an accept/reject flip can only move the result by ~rtol, so this pins
    # the right-hand sides (literal and augmented) and the day driver to 1e-9
    (dict(integrator='cashkarp', rtol=1e-11, atol=1e-13), 1e-9),
    (dict(integrator='cashkarp_aug', rtol=1e-11, atol=1e-13), 1e-9),
    # adaptive at working tolerances: both are valid integrations at rtol, they agree to ~10 rtol
    (None, helpers.TOL_WORKING),
    (dict(integrator='cashkarp'), helpers.TOL_WORKING),
    (dict(integrator='cashkarp_aug', rtol=1e-6, atol=1e-9), 1e-5),
    (dict(integrator='cashkarp', rtol=1e-6, atol=1e-9, project_vr=0), 1e-5)])
def test_kernel_matches_oracle(engine0, oracle_lib, name, solver, tol):
    if name == 'stiff_chain12_2004' and solver and solver.get('integrator') == 'rk4':
        solver = dict(solver, substeps=384)      # the outlet relaxes ~300-700 times a day: classical RK4 is stable for h x rate < 2.78
    m = helpers.marshal_scenario(name, E=3, solver=solver)
    got, status, stats = gpu_run(engine0, m)
    ref, rstatus, rstats = cpu_run(oracle_lib, m)
    assert status.max() == 0 and rstatus.max() == 0
    for ci, c in enumerate(marshal.OUT_COLUMNS):
        err = helpers.max_rel_err(got[ci], ref[ci], floor=FLOOR)
        assert err < tol, (c, err)
    # the step-size controller is mirrored: same number of right-hand-side evaluations
    assert abs(stats['rhs_evals'] - rstats['rhs_evals']) <= 0.005 * rstats['rhs_evals']


@pytest.mark.parametrize('name', SCENARIOS + ['tarland_1981_2010_dynamic'])
def test_kernel_meets_parity_bar_against_reference(engine0, name):
    """Default solver vs the reference's equations integrated by odeint(rtol=atol=1e-12): <= 1e-6 relative on
    all reach outputs, every reach, every day."""
    m = helpers.marshal_scenario(name)
    got, status, _ = gpu_run(engine0, m)
    gold = helpers.golden_tables(name, 'tight')
    assert status.max() == 0
    worst = {}
    for j, sc in enumerate(m['scs']):
        for c in REACH_COLS:
            worst[c] = max(worst.get(c, 0.0), helpers.max_rel_err(got[marshal.OUT_COLUMNS.index(c), :, j, 0],
                                                                  gold['R'][sc][c].values, floor=1e-300))
    assert max(worst.values()) < 1e-6, worst


def test_replicated_ensemble_is_bitwise_identical(engine0):
    """BASELINE config C2 shape: 1024 members with the base parameters -> every member equals the E=1 run
    bit for bit (full 25-column output)."""
    m1 = helpers.marshal_scenario('tarland_2004_dynamic', E=1)
    mE = helpers.marshal_scenario('tarland_2004_dynamic', E=1024)
    o1, _, _ = gpu_run(engine0, m1)
    oE, st, _ = gpu_run(engine0, mE)
    assert st.max() == 0
    assert np.array_equal(oE, np.broadcast_to(o1, oE.shape), equal_nan=True)


@pytest.mark.parametrize('E', [1, 63, 65, 130])
def test_ragged_ensemble_sizes(engine0, oracle_lib, E):
    """E not a multiple of the 64-lane wavefront: tail lanes are masked, nothing is written past E."""
    m = helpers.marshal_scenario('chain4_val_2004', E=E, solver=dict(integrator='rk4', substeps=16))
    rng = np.random.default_rng(E)
    m['member_params'][marshal.PM_NAMES.index('T_g')] *= rng.uniform(0.8, 1.25, E)
    import torch
    ncols, D, S = 25, m['forcing'].shape[2], 4
    guard = torch.full((ncols * D * S * E + 64,), -777.0, dtype=torch.float64, device='cuda')
    out = guard[:ncols * D * S * E].view(ncols, D, S, E)
    got, status, _ = gpu_run(engine0, m, out=out)
    assert (guard[ncols * D * S * E:] == -777.0).all()
    ref, _, _ = cpu_run(oracle_lib, m)
    assert helpers.max_rel_err(got, ref, floor=FLOOR) < 1e-10


@pytest.mark.parametrize('D', [1, 2, 255, 256, 257])
def test_run_lengths_around_the_forcing_tile(engine0, oracle_lib, D):
    """Forcing is staged through LDS in tiles of 256 days: one day, one tile exactly, one day more; chain kernel and
    (forced) task-queue kernel, against the oracle."""
    m = helpers.marshal_scenario('confluence3_nc_2004', E=70, solver=dict(integrator='cashkarp_aug', rtol=1e-10, atol=1e-12))
    m['forcing'] = np.ascontiguousarray(m['forcing'][:, :, :D]); m['doy'] = np.ascontiguousarray(m['doy'][:D])
    m['member_params'][marshal.PM_NAMES.index('T_g')] *= np.linspace(0.7, 1.3, 70)
    got, status, st = gpu_run(engine0, m)
    sub = dict(m, member_params=m['member_params'][:, :3], reach_params=m['reach_params'][:, :, :3])
    ref, _, _ = cpu_run(oracle_lib, sub)
    assert got.shape[1] == D and status.max() == 0
    assert helpers.max_rel_err(got[..., :3], ref, floor=FLOOR) < 1e-8
    m['opts'].time_chunk_days = 256                      # queue kernel needs more than one chunk: falls back when D <= 256
    got2, _, st2 = gpu_run(engine0, m)
    assert st2['queued'] == (1 if D > 256 else 0) and np.array_equal(got2, got, equal_nan=True)


def test_output_selection_is_a_slice_of_the_full_output(engine0):
    full = helpers.marshal_scenario('confluence3_nc_2004', E=5)
    got_full, _, _ = gpu_run(engine0, full)
    cols = ['Qr', 'TDP_kg/day', 'P_labile_NC_kg', 'VsA']
    part = helpers.marshal_scenario('confluence3_nc_2004', E=5, out_mask=marshal.mask_of_columns(cols))
    got_part, _, _ = gpu_run(engine0, part, out_reaches=[2, 0])
    order = marshal.columns_of_mask(marshal.mask_of_columns(cols))      # ascending column id
    for k, c in enumerate(order):
        for slot, reach in enumerate([2, 0]):
            assert np.array_equal(got_part[k, :, slot], got_full[marshal.OUT_COLUMNS.index(c), :, reach]), (c, reach)


def test_per_member_forcing_sets(engine0):
    """n_forcing_sets = 2 with a per-member index: each member equals the single-set run on its forcing."""
    m = helpers.marshal_scenario('tarland_2004_dynamic', E=6)
    f2 = m['forcing'].copy()
    f2[0, 0] *= 1.2
    f2[0, 1] *= 0.9
    both = np.concatenate([m['forcing'], f2])
    fom = np.array([0, 1, 1, 0, 1, 0], dtype=np.int32)
    a, _, _ = gpu_run(engine0, m)
    mb = dict(m, forcing=f2)
    b, _, _ = gpu_run(engine0, mb)
    mm = dict(m, forcing=both)
    c, st, _ = gpu_run(engine0, mm, forcing_of_member=fom)
    assert st.max() == 0
    for e in range(6):
        want = (a if fom[e] == 0 else b)[..., e]
        assert np.array_equal(c[..., e], want, equal_nan=True)


def test_status_flags(engine0):
    m = helpers.marshal_scenario('tarland_2004_static', E=4)
    m['member_params'][marshal.PM_NAMES.index('T_s_A'), 2] = np.nan
    got, status, _ = gpu_run(engine0, m)
    assert status[2] & abi.STATUS_NONFINITE and status[0] == status[1] == status[3] == 0
    assert np.isnan(got[marshal.OUT_COLUMNS.index('Qr'), -1, 0, 2])
    assert np.array_equal(got[..., 0], got[..., 3])
    # a cap of 12 attempts per day cannot hold the tolerance on storm days: the day is finished with one
    # forced step and the member is flagged (and flagged NONFINITE if that step blew up)
    m = helpers.marshal_scenario('tarland_2004_static', E=2, solver=dict(max_steps=12))
    got, status, _ = gpu_run(engine0, m)
    assert (status & abi.STATUS_STEPCAP).all()
    assert bool(np.isfinite(got[:12]).all()) == (not (status & abi.STATUS_NONFINITE).any())


def test_argument_errors_come_back_as_exceptions(engine0):
    m = helpers.marshal_scenario('tarland_2004_static', E=2)
    bad = abi.make_opts(dict(integrator='rk4', substeps=0))
    with pytest.raises(engine.EngineError, match='substeps'):
        engine0.run(m['forcing'], m['doy'], m['member_params'], m['reach_params'], m['up_ptr'], m['up_idx'], bad)
    with pytest.raises(engine.EngineError, match='fp32'):      # default rtol 1e-8 is out of reach of fp32 stages
        engine0.run(m['forcing'], m['doy'], m['member_params'], m['reach_params'], m['up_ptr'], m['up_idx'],
                    abi.make_opts(dict(integrator='cashkarp_aug_f32')))
    with pytest.raises(engine.EngineError, match='upstream'):
        m3 = helpers.marshal_scenario('confluence3_nc_2004', E=2)
        engine0.run(m3['forcing'], m3['doy'], m3['member_params'], m3['reach_params'],
                    np.array([0, 1, 1, 1]), np.array([2]), m3['opts'])
    with pytest.raises(ValueError):
        engine0.run(m['forcing'][:, :, :100], m['doy'], m['member_params'], m['reach_params'],
                    m['up_ptr'], m['up_idx'], m['opts'])
    for step_len in (0.0, -1.0, float('nan'), float('inf')):        # refused by check_args before any launch
        with pytest.raises(engine.EngineError, match='step_len'):
            engine0.run(m['forcing'], m['doy'], m['member_params'], m['reach_params'], m['up_ptr'], m['up_idx'],
                        abi.make_opts(step_len=step_len))


# ---------------------------------------------------------------------------------------------------
# the drop-in API

@pytest.mark.parametrize('name', SCENARIOS + ['tarland_1981_2010_dynamic'])
def test_run_simply_p_drop_in(engine0, name, capsys):
    """run_simply_p on the reference's inputs: same tables (names, order, index), same in-place edits of
    p_LU / p_SC, same Kf, same printed lines as the reference produced for the golden run."""
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs(name)
    df_TC, df_R, Kf, output_dict = sp.run_simply_p(met, p_struc, p_SU, p_LU, p_SC, p, dyn)
    printed = capsys.readouterr().out
    info = helpers.meta()[name]
    gold = helpers.golden_tables(name, 'tight')
    assert Kf == pytest.approx(info['runs']['tight']['Kf'], rel=1e-15)
    assert sorted(df_R.keys()) == sorted(gold['R'].keys())
    for sc in gold['R']:
        assert list(df_R[sc].columns) == list(gold['R'][sc].columns)
        assert list(df_TC[sc].columns) == list(gold['TC'][sc].columns)
        assert df_R[sc].index.equals(met.index)
        for c in gold['R'][sc].columns:       # all 18 reach columns incl. derived concentrations
            assert helpers.max_rel_err(df_R[sc][c].values, gold['R'][sc][c].values, floor=1e-300) < 1e-6, (sc, c)
        for c in gold['TC'][sc].columns:      # soil-water flows sit on the gate's steep flank: 1e-5
            tol = 2e-5 if c in ('QsA', 'QsS', 'QsNC') else 1e-6
            assert helpers.max_rel_err(df_TC[sc][c].values, gold['TC'][sc][c].values, floor=1e-9) < tol, (sc, c)
    for col, rows in info['p_LU_after'].items():
        for k, v in rows.items():
            got = p_LU.loc[k, col]
            assert (np.isnan(got) if v is None else got == pytest.approx(v, rel=1e-15)), (k, col)
    for col, rows in info['p_SC_after'].items():
        for k, v in rows.items():
            got = p_SC.loc[k, int(col)]
            assert (got == v) if isinstance(v, str) else got == pytest.approx(v, rel=1e-15), (k, col)
    assert printed == info['runs']['tight']['stdout']
    assert output_dict['member_status'] == 0 and output_dict['rhs_evals'] > 0


def test_run_simply_p_writes_reference_csvs(engine0, tmp_path):
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs('tarland_2004_static')
    p_SU['save_output_csvs'] = 'y'
    p_SU['output_fpath'] = str(tmp_path)
    df_TC, df_R, _, _ = sp.run_simply_p(met, p_struc, p_SU, p_LU, p_SC, p, dyn)
    r = pd.read_csv(tmp_path / 'Instream_results_Reach1.csv', index_col=0)
    ref = pd.read_csv(helpers.DATA + '/Instream_results_Reach1.csv', index_col=0)
    assert list(r.columns) == list(ref.columns) and len(r) == 366      # the reference's on-disk column set
    tc = pd.read_csv(tmp_path / 'Results_TC_SC1.csv', index_col=0)
    assert set(pd.read_csv(helpers.DATA + '/Results_TC_SC1.csv', index_col=0).columns) <= set(tc.columns) | {'TDPs_NC_kgmm'}


def test_run_simply_p_validation_errors_before_any_launch(engine0):
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs('tarland_2004_static')
    p_SC.loc['f_S', 1] = 0.45
    with pytest.raises(ValueError, match='Land use proportions do not add to 1'):
        sp.run_simply_p(met, p_struc, p_SU, p_LU, p_SC, p, dyn)


def test_run_simply_p_ensemble_with_forcing_scenarios(engine0):
    """A list of met dataframes + forcing_of_member: every member equals a single-scenario run of its own set."""
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs('tarland_2004_dynamic')
    wet = met.copy(); wet['P'] = wet['P'] * 1.2
    warm = met.copy(); warm['PET'] = warm['PET'] * 1.3
    args = lambda m: (m, p_struc.copy(), p_SU.copy(), p_LU.copy(), p_SC.copy(), p.copy(), dyn.copy())
    fom = np.array([0, 1, 2, 1, 0])
    fc = np.array([290.0, 270.0, 310.0, 290.0, 280.0])
    res = sp.run_simply_p_ensemble(*args([met, wet, warm]), overrides={'fc': fc}, forcing_of_member=fom)
    for k, m in enumerate((met, wet, warm)):
        pick = np.flatnonzero(fom == k)
        one = sp.run_simply_p_ensemble(*args(m.copy()), overrides={'fc': fc[pick]})
        assert np.array_equal(res['data'][..., pick], one['data'])
    with pytest.raises(ValueError, match='forcing_of_member'):
        sp.run_simply_p_ensemble(*args([met, wet]), overrides={'fc': fc})
    with pytest.raises(ValueError, match='same dates'):
        sp.run_simply_p_ensemble(*args([met, wet.iloc[:-1]]), overrides={'fc': fc}, forcing_of_member=fom % 2)


def test_run_simply_p_ensemble_overrides(engine0, oracle_lib):
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs('chain4_val_2004')
    E = 10
    rng = np.random.default_rng(3)
    over = {'fc': 290 * rng.uniform(0.8, 1.2, E), 'T_s_A': rng.uniform(1, 4, E),
            'L_reach': np.array([[3000.], [5000.], [7000.], [10000.]]) * rng.uniform(0.7, 1.3, (1, E))}
    res = sp.run_simply_p_ensemble(met, p_struc, p_SU, p_LU, p_SC, p, dyn, overrides=over, out_reaches=[4])
    assert res['columns'] == marshal.REACH5_COLUMNS and res['reaches'] == [4]
    assert res['data'].shape == (5, 366, 1, E) and res['status'].max() == 0
    # same thing by hand on the oracle
    m = helpers.marshal_scenario('chain4_val_2004', E=E, out_mask=marshal.MASK_REACH5)
    m['member_params'][marshal.PM_NAMES.index('fc')] = over['fc']
    m['member_params'][marshal.PM_NAMES.index('T_s_A')] = over['T_s_A']
    m['reach_params'][marshal.PR_NAMES.index('L_reach')] = over['L_reach']
    ref, _, _ = cpu_run(oracle_lib, m, out_reaches=[3])
    assert helpers.max_rel_err(res['data'], ref, floor=FLOOR) < helpers.TOL_WORKING


# ---------------------------------------------------------------------------------------------------
# full-size properties (BASELINE configs C2 / C3: Tarland 1981-2010, 10 957 days)

def test_full_size_monte_carlo_properties(engine0, oracle_lib):
    """70 000-member Monte-Carlo ensemble over the 30-year series: more waves (1094) than the chip has SIMDs (1024), so the
    run takes the path bench.py times -- pilot, cost-ordered lane slots, time-chunk task queue -- here with the table
    scattered back to member order.
    Properties that do not depend on size: no member flagged; members do not interact (a permutation of the
    members permutes the outputs; a shard equals the same members of the unsharded run, bit for bit);
    Vr stays on the invariant of the reference's equations; a seeded sample of members agrees with the oracle."""
    import torch
    E = 70000
    pr = synthetic.c3_problem(E)
    eng = engine0
    out, status, stats = eng.run(pr['forcing'], pr['doy'], pr['member_params'], pr['reach_params'],
                                 pr['up_ptr'], pr['up_idx'], pr['opts'])
    assert stats['queued'] == 1 and stats['balanced'] == 1
    assert int(status.max()) == 0
    assert bool(torch.isfinite(out).all())
    n = E * out.shape[1]
    assert 60 < stats['rhs_evals'] / n < 400
    # sample vs oracle
    rng = np.random.default_rng(42)
    pick = np.sort(rng.choice(E, 8, replace=False))
    sub = dict(pr, member_params=pr['member_params'][:, pick], reach_params=pr['reach_params'][:, :, pick])
    ref, _, _ = cpu_run(oracle_lib, sub, n_threads=8)
    got = out[..., torch.as_tensor(pick, device=out.device)].cpu().numpy()
    assert helpers.max_rel_err(got, ref, floor=FLOOR) < helpers.TOL_WORKING
    # the working tolerance holds across the parameter distribution, not only for the golden members: every 16th member
    # (4375 of them), all 10 957 days, REACH-5 columns, against the same kernel at rtol 1e-11 -- which the golden
    # scenarios pin to the reference's tight solution to 1e-9 (test_kernel_matches_oracle / test_oracle_series)
    tight = dict(pr)
    tight['member_params'] = pr['member_params'][:, ::16]; tight['reach_params'] = pr['reach_params'][:, :, ::16]
    tight['opts'] = abi.make_opts(dict(rtol=1e-11, atol=1e-13), dynamic_epc0=True, out_mask=marshal.MASK_REACH5)
    truth = eng.run(tight['forcing'], tight['doy'], tight['member_params'], tight['reach_params'], tight['up_ptr'], tight['up_idx'],
                    tight['opts'])[0]
    rel = ((out[..., ::16] - truth).abs() / truth.abs()).amax(dim=(0, 1, 2))
    assert float(rel.max()) < 1e-6, (float(rel.max()), int((rel > 1e-6).sum()))
    del truth, rel
    # permutation invariance + shard == unsharded, on a 4096-member slice
    sl = np.arange(4096) * 17
    perm = rng.permutation(len(sl))
    a = eng.run(pr['forcing'], pr['doy'], pr['member_params'][:, sl[perm]], pr['reach_params'][:, :, sl[perm]],
                pr['up_ptr'], pr['up_idx'], pr['opts'])[0]
    assert bool(torch.equal(a, out[..., torch.as_tensor(sl[perm], device=out.device)]))
    for rank in range(8):
        lo, hi = ensemble.shard_bounds(E, 8, rank)
        if rank in (0, 5):
            b = eng.run(pr['forcing'], pr['doy'], pr['member_params'][:, lo:hi], pr['reach_params'][:, :, lo:hi],
                        pr['up_ptr'], pr['up_idx'], pr['opts'])[0]
            assert bool(torch.equal(b, out[..., lo:hi]))
    # Vr on its invariant: Vr = L Qr_end^(1-b) / (a_Q 86400) needs Qr_EndOfDay -> rerun 256 members with it
    m = dict(pr, member_params=pr['member_params'][:, :256], reach_params=pr['reach_params'][:, :, :256])
    m['opts'] = abi.make_opts(dynamic_epc0=True, out_mask=marshal.mask_of_columns(['Vr', 'Qr_EndOfDay']))
    o2 = eng.run(m['forcing'], m['doy'], m['member_params'], m['reach_params'], m['up_ptr'], m['up_idx'], m['opts'])[0]
    o2 = o2.cpu().numpy()
    aQ = m['member_params'][marshal.PM_NAMES.index('a_Q')]
    bQ = m['member_params'][marshal.PM_NAMES.index('b_Q')]
    L = m['reach_params'][marshal.PR_NAMES.index('L_reach'), 0]
    inv = L * o2[1, :, 0, :] ** (1 - bQ) / (aQ * 86400)
    assert helpers.max_rel_err(o2[0, :, 0, :], inv) < 1e-12


def test_one_million_members_on_one_gpu(engine0):
    """BASELINE config C5's ensemble size on a single GPU (5.5 years, annual sums of two columns so that the output stays
    small): 15 625 member groups through the task queue, cost-ordered; no member flagged, every member in exactly one slot,
    and a slice of members run on its own equals the big run bit for bit."""
    import torch
    E = 1000000
    pr = synthetic.c3_problem(E, end_dt='1986-06-30', solver=dict(out_slot_order=1), out_mask=marshal.mask_of_columns(['Qr', 'TDP_kg/day']))
    periods, pod = np.unique(pr['met'].index.year.values, return_inverse=True)
    pod = np.ascontiguousarray(pod, dtype=np.int32)
    pr['opts'].n_periods = len(periods)
    out, status, st = engine0.run(pr['forcing'], pr['doy'], pr['member_params'], pr['reach_params'], pr['up_ptr'], pr['up_idx'], pr['opts'],
                                  period_of_day=pod)
    assert st['queued'] == 1 and st['balanced'] == 1 and int((status != 0).sum()) == 0 and bool(torch.isfinite(out).all())
    mos = st['member_of_slot']
    assert int(torch.unique(mos).numel()) == E and int(mos.min()) == 0 and int(mos.max()) == E - 1
    pick = np.arange(0, E, 9973)[:64]
    sub = dict(pr, member_params=pr['member_params'][:, pick], reach_params=pr['reach_params'][:, :, pick])
    sub['opts'].out_slot_order = 0
    alone = engine0.run(sub['forcing'], sub['doy'], sub['member_params'], sub['reach_params'], sub['up_ptr'], sub['up_idx'], sub['opts'],
                        period_of_day=pod)[0]
    slot_of = torch.empty(E, dtype=torch.long, device=out.device)
    slot_of[mos.long()] = torch.arange(E, device=out.device)
    assert bool(torch.equal(out[..., slot_of[torch.as_tensor(pick, device=out.device)]], alone))


def test_load_balancer_groups_members_with_similar_step_patterns(engine0):
    """What the pilot + ordering is for: lanes of a wavefront that need similar step counts day by day.  On the bench's
    Monte-Carlo distribution the fraction of issued lane-attempts that were needed (stats.simt_efficiency) rises from
    ~0.62 (members as drawn) to ~0.77 (0.82 before the step controller shortened the steps that cross a knee of a gate:
    which lane crosses on which day is not something a pilot run can predict); asserted with margin, on a 3-year slice."""
    pr = synthetic.c3_problem(70000, end_dt='1983-12-31', solver=dict(out_slot_order=1))
    eff = {}
    for balance in (0, 1):
        pr['opts'].balance = balance
        out, status, st = engine0.run(pr['forcing'], pr['doy'], pr['member_params'], pr['reach_params'], pr['up_ptr'], pr['up_idx'], pr['opts'])
        assert st['balanced'] == balance and int(status.max()) == 0
        eff[balance] = st['simt_efficiency']
        mos = st['member_of_slot'].cpu().numpy()
        assert sorted(mos.tolist()) == list(range(70000))
    assert eff[0] < 0.70 and eff[1] > 0.74 and eff[1] - eff[0] > 0.12, eff


@pytest.mark.parametrize('name', ['tarland_2004_dynamic', 'chain4_val_2004', 'confluence3_nc_2004', 'net5_static_2004',
                                  'net5_dynamic_leakA_2004'])
def test_load_balanced_run_is_bitwise_identical(engine0, name):
    """opts.balance = 1 (pilot run + cost-sorted lane slots, routing series kept in slot order): outputs,
    status and per-member work come back in member order and equal the unbalanced run bit for bit."""
    import torch
    E = 333
    m0 = helpers.marshal_scenario(name, E=E, solver=dict(balance=0))
    rng = np.random.default_rng(17)
    for pname, lo, hi in (('a_Q', 0.5, 2.0), ('T_s_A', 0.5, 2.0), ('fc', 0.8, 1.2), ('T_g', 0.6, 1.5)):
        m0['member_params'][marshal.PM_NAMES.index(pname)] *= rng.uniform(lo, hi, E)
    m0['member_params'][marshal.PM_NAMES.index('T_s_A'), 5] = np.nan          # one poisoned member
    m1 = dict(m0, opts=abi.make_opts(dict(balance=1, balance_pilot_days=40),
                                     dynamic_epc0=bool(m0['opts'].dynamic_epc0), dynamic_erod=bool(m0['opts'].dynamic_erod),
                                     run_mode_cal=bool(m0['opts'].run_mode_cal), sc_qr0=m0['opts'].sc_qr0))
    w0 = torch.zeros(E, dtype=torch.int32, device='cuda')
    w1 = torch.zeros(E, dtype=torch.int32, device='cuda')
    a, sa, st_a = gpu_run(engine0, m0, member_rhs=w0)
    b, sb, st_b = gpu_run(engine0, m1, member_rhs=w1)
    assert st_a['balanced'] == 0 and st_b['balanced'] == 1
    assert np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(sa, sb) and sa[5] & abi.STATUS_NONFINITE and (np.delete(sa, 5) == 0).all()
    assert bool(torch.equal(w0, w1)) and st_a['rhs_evals'] == st_b['rhs_evals'] == int(w0.sum())
    assert int(w0.max()) > 1.2 * int(w0[w0 > 0].min())       # the members really do differ in cost


def test_c4_chain_of_256_reaches_in_kernel(engine0, oracle_lib):
    """BASELINE config C4's shape at test size: a 256-reach linear chain walked inside the kernel by one thread
    per member (one launch, two recycled routing slots), 4 land-use classes, dynamic erodibility, 70 members,
    400 days; final reach's five outputs against the oracle."""
    pr = synthetic.c4_problem(70, n_reaches=256, n_days=400)
    pl = engine.plan(pr['up_ptr'], pr['up_idx'])
    assert pl['n_launches'] == 1 and pl['n_slots'] == 2
    out, status, stats = engine0.run(pr['forcing'], pr['doy'], pr['member_params'], pr['reach_params'],
                                     pr['up_ptr'], pr['up_idx'], pr['opts'], out_reaches=pr['out_reaches'])
    got = out.cpu().numpy()
    assert got.shape == (5, 400, 1, 70) and int(status.max()) == 0 and stats['n_launches'] == 1
    pick = [0, 33, 69]
    sub = dict(pr, member_params=pr['member_params'][:, pick], reach_params=pr['reach_params'][:, :, pick])
    ref, rstatus, _ = cpu_run(oracle_lib, sub, out_reaches=pr['out_reaches'], n_threads=3)
    assert rstatus.max() == 0
    assert helpers.max_rel_err(got[..., pick], ref, floor=FLOOR) < helpers.TOL_WORKING
    # flow accumulates down the chain: the outlet carries far more water per unit of its own area than a headwater
    assert got[1].mean() > 5.0


def test_slot_order_output_mode(engine0):
    """opts.out_slot_order = 1: `out` columns are lane slots (coalesced stores); member_of_slot maps them back.
    Same numbers as the member-order run, bit for bit."""
    E = 200
    m = helpers.marshal_scenario('tarland_2004_dynamic', E=E, solver=dict(balance=1, balance_pilot_days=30))
    rng = np.random.default_rng(23)
    m['member_params'][marshal.PM_NAMES.index('a_Q')] *= rng.uniform(0.5, 2.0, E)
    a, sa, _ = gpu_run(engine0, m)
    m['opts'].out_slot_order = 1
    b, sb, st = gpu_run(engine0, m)
    mos = st['member_of_slot'].cpu().numpy()
    assert st['balanced'] == 1 and sorted(mos) == list(range(E)) and not np.array_equal(mos, np.arange(E))
    assert np.array_equal(b, a[..., mos]) and np.array_equal(sa, sb)
    m['opts'].balance = 0                                # no reordering: identity map
    c, _, st = gpu_run(engine0, m)
    assert np.array_equal(st['member_of_slot'].cpu().numpy(), np.arange(E)) and np.array_equal(c, a)


@pytest.mark.parametrize('integrator', ['cashkarp_aug', 'cashkarp', 'cashkarp_aug_f32'])
def test_task_queue_kernel_is_bitwise_identical(engine0, integrator):
    """opts.time_chunk_days > 0: the run is cut into (time chunk x 64-member group) tasks pulled by persistent
    waves, state handed over through memory between chunks.  Same results bit for bit, with and without the
    cost-sorted member order, in member order and in slot order."""
    import torch
    E = 300                                         # 5 groups, the last one ragged (44 lanes)
    name = 'tarland_1981_2010_dynamic'
    tol = dict(rtol=1e-5, atol=1e-7) if integrator.endswith('f32') else {}
    base = helpers.marshal_scenario(name, E=E, out_mask=marshal.MASK_REACH5, solver=dict(tol, integrator=integrator, balance=0, time_chunk_days=-1))
    D = 2200                                        # 9 chunks of 256 days (the last one short)
    base['forcing'] = np.ascontiguousarray(base['forcing'][:, :, :D])
    base['doy'] = np.ascontiguousarray(base['doy'][:D])
    rng = np.random.default_rng(29)
    for pname, lo, hi in (('a_Q', 0.5, 2.0), ('T_s_A', 0.5, 2.0), ('fc', 0.8, 1.2)):
        base['member_params'][marshal.PM_NAMES.index(pname)] *= rng.uniform(lo, hi, E)
    base['member_params'][marshal.PM_NAMES.index('T_s_S'), 77] = np.nan       # a poisoned member rides along
    w0 = torch.zeros(E, dtype=torch.int32, device='cuda')
    ref, sref, st0 = gpu_run(engine0, base, member_rhs=w0)
    assert st0['queued'] == 0
    for balance, slot_order in ((0, 0), (1, 0), (1, 1)):
        m = dict(base)
        m['opts'] = abi.make_opts(dict(tol, integrator=integrator, balance=balance, balance_pilot_days=100, time_chunk_days=256,
                                       out_slot_order=slot_order), dynamic_epc0=True, dynamic_erod=True,
                                  out_mask=marshal.MASK_REACH5)
        w1 = torch.zeros(E, dtype=torch.int32, device='cuda')
        got, sgot, st = gpu_run(engine0, m, member_rhs=w1)
        assert st['queued'] == 1 and st['balanced'] == balance
        if slot_order:
            got_m = np.empty_like(got)
            got_m[..., st['member_of_slot'].cpu().numpy()] = got
            got = got_m
        assert np.array_equal(got, ref, equal_nan=True), (balance, slot_order)
        assert np.array_equal(sgot, sref) and sref[77] & abi.STATUS_NONFINITE
        assert bool(torch.equal(w0, w1)) and st['rhs_evals'] == st0['rhs_evals']


def test_time_reduced_output_equals_sums_of_daily_rows(engine0):
    """opts.n_periods: rows are per-period running sums accumulated in the kernel (chain kernel and task-queue
    kernel, member order and slot order) == the daily rows summed per period on the host."""
    met, p_struc, p_SU, p_LU, p_SC, p, dyn = helpers.scenario_inputs('tarland_1981_2010_dynamic')
    met = met.iloc[:1500]
    E = 130
    rng = np.random.default_rng(31)
    over = {'a_Q': 0.5 * rng.uniform(0.5, 2.0, E), 'fc': 290 * rng.uniform(0.8, 1.2, E)}
    cols = ['Qr', 'Msus_kg/day', 'TDP_kg/day', 'PP_kg/day', 'VsA']
    daily = sp.run_simply_p_ensemble(met, p_struc.copy(), p_SU.copy(), p_LU.copy(), p_SC.copy(), p.copy(), dyn,
                                     overrides=over, outputs=cols, solver=dict(time_chunk_days=-1, balance=0))
    years = np.asarray(met.index.year)
    uy = np.unique(years)
    want = np.stack([daily['data'][:, years == y].sum(axis=1) for y in uy], axis=1)
    for solver in (dict(time_chunk_days=-1, balance=0), dict(time_chunk_days=256, balance=1, balance_pilot_days=60)):
        red = sp.run_simply_p_ensemble(met, p_struc.copy(), p_SU.copy(), p_LU.copy(), p_SC.copy(), p.copy(), dyn,
                                       overrides=over, outputs=cols, reduce='annual', solver=solver)
        assert list(red['periods']) == list(uy) and red['data'].shape == (5, len(uy), 1, E)
        assert red['columns'] == daily['columns'] and red['status'].max() == 0
        np.testing.assert_allclose(red['data'], want, rtol=1e-12)
    with pytest.raises(ValueError):
        sp.run_simply_p_ensemble(met, p_struc.copy(), p_SU.copy(), p_LU.copy(), p_SC.copy(), p.copy(), dyn,
                                 overrides=over, reduce='monthly')


@pytest.mark.parametrize('name', ['chain4_val_2004', 'confluence3_nc_2004', 'net5_static_2004', 'net5_dynamic_leakA_2004'])
def test_pipelined_queue_on_reach_networks_is_bitwise_identical(engine0, name):
    """Multi-reach networks through the task-queue kernel: (reach, chunk, group) tasks in dependency order,
    upstream series through ring buffers of a few chunks, state handed over between chunks.  Same results bit for
    bit as the chain kernel (one thread walking its reaches upstream to downstream)."""
    E = 150
    m = helpers.marshal_scenario(name, E=E, solver=dict(time_chunk_days=-1, balance=0))
    m['forcing'] = np.ascontiguousarray(np.tile(m['forcing'], (1, 1, 4)))          # 1464 days = 6 chunks of 256
    m['doy'] = np.ascontiguousarray(np.tile(m['doy'], 4))
    rng = np.random.default_rng(37)
    for pname, lo, hi in (('a_Q', 0.6, 1.6), ('T_s_A', 0.5, 2.0), ('fc', 0.8, 1.2)):
        m['member_params'][marshal.PM_NAMES.index(pname)] *= rng.uniform(lo, hi, E)
    ref, sref, st0 = gpu_run(engine0, m)
    assert st0['queued'] == 0 and sref.max() == 0
    for balance in (0, 1):
        m['opts'].time_chunk_days = 256
        m['opts'].balance = balance
        m['opts'].balance_pilot_days = 80
        got, sgot, st = gpu_run(engine0, m)
        assert st['queued'] == 1 and st['n_launches'] == 1 and st['balanced'] == balance
        assert np.array_equal(got, ref, equal_nan=True) and np.array_equal(sgot, sref)
        assert st['rhs_evals'] == st0['rhs_evals']


def test_c4_chain_pipelined_matches_chain_kernel_and_oracle(engine0, oracle_lib):
    """BASELINE config C4's shape through the pipelined queue (auto: a 256-reach chain with few members cannot fill
    the chip from one thread per member): 256-deep pipeline, 2-chunk routing rings; equals the in-kernel chain walk
    bit for bit and the oracle to 10 x rtol."""
    pr = synthetic.c4_problem(70, n_reaches=256, n_days=700)
    out, status, st = engine0.run(pr['forcing'], pr['doy'], pr['member_params'], pr['reach_params'],
                                  pr['up_ptr'], pr['up_idx'], pr['opts'], out_reaches=pr['out_reaches'])
    assert st['queued'] == 1 and int(status.max()) == 0
    pr['opts'].time_chunk_days = -1
    ref, _, st0 = engine0.run(pr['forcing'], pr['doy'], pr['member_params'], pr['reach_params'],
                              pr['up_ptr'], pr['up_idx'], pr['opts'], out_reaches=pr['out_reaches'])
    assert st0['queued'] == 0
    import torch
    assert bool(torch.equal(out, ref))
    pick = [5, 64]
    sub = dict(pr, member_params=pr['member_params'][:, pick], reach_params=pr['reach_params'][:, :, pick])
    cref, _, _ = cpu_run(oracle_lib, sub, out_reaches=pr['out_reaches'], n_threads=2)
    assert helpers.max_rel_err(out.cpu().numpy()[..., pick], cref, floor=FLOOR) < helpers.TOL_WORKING


@pytest.mark.parametrize('name', ['tarland_1981_2010_dynamic', 'confluence3_nc_2004'])
def test_fp32_stage_mode(engine0, name):
    """BASELINE config C5's arithmetic: the Runge-Kutta stages in fp32, the four daily integrals (Qr, Msus/TDP/PP
    kg/day), the soil-P update and everything carried from day to day outside the stages in fp64.  Tolerance: 5e-4
    relative on every reach output against the reference at rtol=atol=1e-12, with rtol 1e-5 / atol 1e-7 -- the same
    class of error the fp64 scheme had at that tolerance before its controller learned about the knees of the gates (the
    fp64 scheme now reaches 2e-5 there; the fp32 mode keeps the plain controller -- one float ulp of a soil store of 300 mm
    is 3e-5 mm, the tolerance the knee logic would hold the soil boxes to -- and stays at 1.8e-4), with about as many
    right-hand-side evaluations (10 %).  fp32 cannot resolve rtol below ~3e-6; this mode is for screening ensembles, not
    for parity."""
    solver = dict(rtol=1e-5, atol=1e-7)
    gold = helpers.golden_tables(name, 'tight')
    worst = {}
    for integ in ('cashkarp_aug_f32', 'cashkarp_aug'):
        m = helpers.marshal_scenario(name, E=2, solver=dict(solver, integrator=integ))
        got, status, stats = gpu_run(engine0, m)
        assert status.max() == 0
        assert np.array_equal(got[..., 0], got[..., 1])
        worst[integ] = max(helpers.max_rel_err(got[marshal.OUT_COLUMNS.index(c), :, j, 0], gold['R'][sc][c].values, floor=1e-300)
                           for j, sc in enumerate(m['scs']) for c in REACH_COLS)
        worst[integ + '_rhs'] = stats['rhs_evals']
    assert worst['cashkarp_aug_f32'] < 5e-4 and worst['cashkarp_aug'] < 5e-4, worst
    assert abs(worst['cashkarp_aug_f32_rhs'] - worst['cashkarp_aug_rhs']) < 0.10 * worst['cashkarp_aug_rhs'], worst


@pytest.mark.parametrize('name', ['tarland_2004_dynamic', 'tarland_1981_2010_dynamic', 'chain4_val_2004', 'confluence3_nc_2004',
                                  'net5_static_erod_val_2004'])
def test_fp32_stage_mode_against_its_oracle_mirror(engine0, oracle_lib, name):
    """The fp32-stage kernel against the oracle's same-arithmetic mirror (cashkarp_aug_f32_day: float stages, float step
    control, double daily integrals), daily flux columns, end-of-day flow and the slow stores, all reaches.  What
    separates the two is libm's logf/expf/powf and a true division against v_log_f32 / v_exp_f32 / v_rcp_f32 -- float
    rounding, on which an accept/reject decision can flip; after a flip they are two valid integrations at the same
    tolerance.  Bar: 10 x rtol on 99 % of the values and 5e-4 on all -- each integration's own global error at rtol 1e-5
    is up to 1.8e-4 against the converged reference (test_fp32_stage_mode: the 30-year series, and reach networks, where
    the error of a reach feeds the next), so two of them can be that far apart on their worst day (measured: 1.9e-4 on
    the 4-reach chain, 2.8e-4 on the worst of 10 957 days; the single-reach year stays below 10 x rtol).  The number of
    right-hand-side evaluations must agree to 1 %.  Not a parity-grade mode (no <= 1e-6 claim)."""
    rtol = 1e-5
    m = helpers.marshal_scenario(name, E=3, solver=dict(integrator='cashkarp_aug_f32', rtol=rtol, atol=1e-7))
    m['member_params'][marshal.PM_NAMES.index('fc')] *= np.array([1.0, 0.9, 1.1])
    got, status, stats = gpu_run(engine0, m)
    ref, ref_status, ref_stats = cpu_run(oracle_lib, m)
    assert status.max() == 0 and ref_status.max() == 0
    cols = [marshal.OUT_COLUMNS.index(c) for c in ('Qr', 'Qr_EndOfDay', 'Msus_kg/day', 'TDP_kg/day', 'PP_kg/day', 'Vr', 'VsA', 'VsS', 'Vg')]
    rel = np.abs(got[cols] - ref[cols]) / np.maximum(np.abs(ref[cols]), 1e-12)
    assert np.percentile(rel, 99) < 10 * rtol and rel.max() < 5e-4, (np.percentile(rel, 99), rel.max())
    if name == 'tarland_2004_dynamic':
        assert rel.max() < 10 * rtol, rel.max()
    assert abs(stats['rhs_evals'] - ref_stats['rhs_evals']) < 0.01 * ref_stats['rhs_evals']


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_random_reach_networks_match_the_oracle(engine0, oracle_lib, seed):
    """Random upstream graphs (12 reaches; 0-2 upstream reaches each, a reach may feed several downstream reaches; reaches
    with newly-converted land of either kind, blank TDPeff, varied areas / lengths / slopes), 40 perturbed members,
    one year: chain kernel and pipelined task queue against the CPU oracle (routing of same-day means and fluxes,
    model.py:508-544) -- 1e-9 with RK4 (rounding only: the kernel's hoisted day constants against the oracle's literal
    formulas, carried through up to 7 reaches in series; measured 1.9e-10), 10 x rtol with the default solver -- and bit-identical to each other."""
    import torch
    S, E = 12, 40
    m = helpers.random_network_problem(seed, E)
    for solver, tol in ((dict(integrator='rk4', substeps=96), 1e-9), (None, helpers.TOL_WORKING)):      # (24 substeps are unstable on the big confluences)
        m['opts'] = abi.make_opts(solver, dynamic_epc0=True, dynamic_erod=True, run_mode_cal=True, sc_qr0=S - 1, out_mask=marshal.MASK_ALL)
        ref, ref_status, _ = cpu_run(oracle_lib, m, n_threads=8)
        m['opts'].time_chunk_days = -1
        chain, cs, cst = gpu_run(engine0, m)
        assert cst['queued'] == 0 and cs.max() == 0 and ref_status.max() == 0
        assert helpers.max_rel_err(chain, ref, floor=FLOOR) < tol, (seed, solver)
        if solver is None:
            m['opts'].time_chunk_days = 256
            queue, qs, qst = gpu_run(engine0, m)
            assert qst['queued'] == 1
            assert np.array_equal(queue, chain, equal_nan=True) and np.array_equal(qs, cs)


def test_knee_aware_controller_on_the_members_that_needed_it(engine0, oracle_lib):
    """Six members of the bench's 100 000-member ensemble whose worst day, under a plain relative-tolerance controller, was a step
    across a knee of one of the reference's gates (tests/test_oracle_series.py::KNEE_MEMBERS): the kernel's default solver against
    the same kernel at rtol 1e-11 below 5e-7 on every REACH-5 value of 30 years, one lane and four lanes per member alike, and
    within 10 x rtol of the CPU oracle's run."""
    from test_oracle_series import KNEE_MEMBERS
    pr = synthetic.c3_problem(100000)
    m = dict(pr, member_params=np.ascontiguousarray(pr['member_params'][:, KNEE_MEMBERS]),
             reach_params=np.ascontiguousarray(pr['reach_params'][:, :, KNEE_MEMBERS]))
    rtol, atol = m['opts'].rtol, m['opts'].atol
    m['opts'].rtol, m['opts'].atol = 1e-11, 1e-13
    truth, st, _ = gpu_run(engine0, m)
    assert st.max() == 0
    m['opts'].rtol, m['opts'].atol = rtol, atol
    ref, rst, _ = cpu_run(oracle_lib, m, n_threads=6)
    for lanes in (1, 4):
        m['opts'].lanes_per_member = lanes
        got, st, stats = gpu_run(engine0, m)
        assert st.max() == 0 and stats['lanes_per_member'] == lanes
        worst = (np.abs(got - truth) / np.maximum(np.abs(truth), 1e-300)).max(axis=(0, 1, 2))
        assert worst.max() < 5e-7, (lanes, dict(zip(KNEE_MEMBERS, worst)))
        assert helpers.max_rel_err(got, ref, floor=FLOOR) < helpers.TOL_WORKING


# ---- the default solver across the parameter distribution, pinned to the REFERENCE on the HIP path ------------------------
# Reference-made tables (tests/golden/make_golden.py: the unmodified reference, odeint at rtol=atol=1e-12, one member at a
# time): the six bench members the knee-aware controller's constants were tuned on, over all 30 years (knee_members.npz); 16
# members of a draw nothing was tuned on, seed C3_SEED + 7 = what rank 7 of a weak-scaling bench runs (heldout_members.npz); 8
# members of the bench's own draw (monte_carlo_members.npz); 24 held-out members of a draw with the time constants and rates widened
# x/÷ 2 (wide_members.npz, round 4).  The kernel -- one lane and four lanes per member -- must meet
# north_star's bar, <= 1e-6 relative on all 9 reach outputs, on every one of them (asserted at 5e-7; measured 2.3e-7 / 1.6e-7 / < 5e-7).

def _worst_per_member(got, tables, cols=REACH_COLS):
    return [max(helpers.max_rel_err(got[marshal.OUT_COLUMNS.index(c), :, 0, k], tables[k][:, j], floor=1e-300)
                for j, c in enumerate(cols)) for k in range(len(tables))]


@pytest.mark.parametrize('fname,bar', [('knee_members.npz', 5e-7), ('heldout_members.npz', 5e-7), ('wide_members.npz', 5e-7)])
@pytest.mark.parametrize('lanes', [1, 4])
def test_default_solver_against_reference_tables_of_single_members(engine0, fname, bar, lanes):
    m, tables = helpers.member_fixture_problem(fname, solver=dict(lanes_per_member=lanes))
    assert m['opts'].rtol == abi.DEFAULT_SOLVER['rtol'] == 1e-7 and m['opts'].integrator == abi.INTEG_CASHKARP_AUG
    got, st, stats = gpu_run(engine0, m)
    assert st.max() == 0 and stats['lanes_per_member'] == lanes
    worst = _worst_per_member(got, tables)
    assert max(worst) < bar, dict(zip(m['members'], worst))


@pytest.mark.parametrize('lanes', [1, 4])
def test_default_solver_against_reference_tables_of_the_bench_draw(engine0, lanes):
    """tests/golden/monte_carlo_members.npz (8 members of the bench's own draw x 3 years, made by the reference) through the
    KERNEL (round 2 checked this fixture against the CPU oracle only)."""
    import os
    z = np.load(os.path.join(helpers.GOLDEN, 'monte_carlo_members.npz'), allow_pickle=False)
    years = [str(y) for y in z['years']]
    n = z['values'].shape[1]
    met_df, p_struc, p_SU, p_LU, p_SC, p, dyn = synthetic.tarland_inputs(years[0], years[1], dynamic_epc0='y', dynamic_erod='n')
    over = synthetic.monte_carlo_overrides(p, p_LU, n)
    for k, nm in enumerate(str(x) for x in z['names']):
        np.testing.assert_array_equal(over[nm], z['values'][k])
    marshal.prologue(p_SU, p_LU, p_SC, p)
    up_ptr, up_idx, _ = marshal.topology(p_struc, p)
    forcing, doy = marshal.forcing_arrays(met_df)
    m = dict(forcing=forcing, doy=doy, member_params=marshal.member_params(p, p_LU, n, over), reach_params=marshal.reach_params(p_SC, p, n),
             up_ptr=up_ptr, up_idx=up_idx, opts=abi.make_opts(dict(lanes_per_member=lanes), dynamic_epc0=True, run_mode_cal=True))
    got, st, stats = gpu_run(engine0, m)
    assert st.max() == 0 and stats['lanes_per_member'] == lanes
    rcols = [str(c) for c in z['R/columns']]
    tables = [z['R/%d' % e][:, [rcols.index(c) for c in REACH_COLS]] for e in range(n)]
    worst = _worst_per_member(got, tables)
    assert max(worst) < 5e-7, worst


def test_held_out_seed_ensemble_wide(engine0):
    """8 192 members of a draw nothing was tuned on (seed C3_SEED + 7), 30 years, REACH-5: the default solver against the same
    kernel at rtol 1e-11 (which the fixtures above pin to the reference to ~5e-8).  No member above 5e-7 -- the constants of the
    knee-aware controller (include/simplyp_controller.h), tuned on the seed-20240601 ensemble, are not over-fitted to it."""
    pr = synthetic.c3_problem(8192, seed=synthetic.C3_SEED + 7)
    rtol, atol = pr['opts'].rtol, pr['opts'].atol
    pr['opts'].rtol, pr['opts'].atol = 1e-11, 1e-13
    import torch
    truth, st, _ = engine0.run(pr['forcing'], pr['doy'], pr['member_params'], pr['reach_params'], pr['up_ptr'], pr['up_idx'], pr['opts'])
    assert int(st.max()) == 0
    pr['opts'].rtol, pr['opts'].atol = rtol, atol
    got, st, stats = engine0.run(pr['forcing'], pr['doy'], pr['member_params'], pr['reach_params'], pr['up_ptr'], pr['up_idx'], pr['opts'])
    assert int(st.max()) == 0
    rel = ((got - truth).abs() / truth.abs().clamp_min(1e-300)).amax(dim=(0, 1, 2))
    worst = float(rel.max())
    assert worst < 5e-7, (worst, int(rel.argmax()))
    assert float(rel.median()) < 1e-7


def test_config_c4_full_shape(engine0, oracle_lib):
    """BASELINE config C4's FULL shape except for the ensemble size -- 256-reach chain x 4 land-use classes x 18 262 days (50
    years), 1 000 members (the bench runs 10 000) -- through the path the bench takes: pipelined task queue (256-deep), cost-
    ordered member groups, slot-order table of the outlet reach.  Size-independent properties: no member flagged; every value
    finite and the outlet carries the chain's accumulated flow; the first 384 days equal, bit for bit, what the in-kernel chain
    walk (one thread per member, no queue) computes for the same members; two members against the CPU oracle over the first
    8 years (10 x rtol)."""
    import torch
    E, S, D = 1000, 256, 18262
    pr = synthetic.c4_problem(E, n_reaches=S, n_days=D, solver=dict(out_slot_order=1))
    out, status, st = engine0.run(pr['forcing'], pr['doy'], pr['member_params'], pr['reach_params'],
                                  pr['up_ptr'], pr['up_idx'], pr['opts'], out_reaches=pr['out_reaches'])
    assert tuple(out.shape) == (5, D, 1, E) and st['queued'] == 1 and st['balanced'] == 1
    assert int(status.max()) == 0 and bool(torch.isfinite(out).all())
    assert st['queue_longest_stall_polls'] < 1000000 and st['queue_waits'] > 0
    mos = st['member_of_slot'].long()
    assert int(torch.unique(mos).numel()) == E
    slot_of = torch.empty(E, dtype=torch.long, device=out.device)
    slot_of[mos] = torch.arange(E, device=out.device)
    assert float(out[1].mean()) > 5.0              # mm/d over the outlet's own area: the flow of 256 sub-catchments
    # the chain kernel on a slice: 64 members, the first 384 days (results of a day do not depend on later days)
    sl = np.arange(64) * 15
    short = dict(pr, forcing=np.ascontiguousarray(pr['forcing'][:, :, :384]), doy=np.ascontiguousarray(pr['doy'][:384]),
                 member_params=np.ascontiguousarray(pr['member_params'][:, sl]), reach_params=np.ascontiguousarray(pr['reach_params'][:, :, sl]))
    short['opts'] = abi.make_opts(dict(time_chunk_days=-1, balance=0), dynamic_epc0=True, dynamic_erod=True, run_mode_cal=True,
                                  sc_qr0=pr['opts'].sc_qr0, out_mask=pr['opts'].out_mask)
    ref, rs, rst = engine0.run(short['forcing'], short['doy'], short['member_params'], short['reach_params'],
                               short['up_ptr'], short['up_idx'], short['opts'], out_reaches=pr['out_reaches'])
    assert rst['queued'] == 0 and int(rs.max()) == 0
    assert bool(torch.equal(ref, out[:, :384][..., slot_of[torch.as_tensor(sl, device=out.device)]]))
    # two members against the CPU oracle over the first 8 years (the oracle takes ~5 s per member and decade of this network)
    pick, Dc = [7, 512], 2922
    sub = dict(pr, forcing=np.ascontiguousarray(pr['forcing'][:, :, :Dc]), doy=np.ascontiguousarray(pr['doy'][:Dc]),
               member_params=pr['member_params'][:, pick], reach_params=pr['reach_params'][:, :, pick])
    cref, cstatus, _ = cpu_run(oracle_lib, sub, out_reaches=pr['out_reaches'], n_threads=2)
    assert cstatus.max() == 0
    got = out[:, :Dc][..., slot_of[torch.as_tensor(pick, device=out.device)]].cpu().numpy()
    assert helpers.max_rel_err(got, cref, floor=FLOOR) < helpers.TOL_WORKING


def dry_climate_members(n=256, seed=synthetic.C3_SEED + 12, pscale=0.6):
    """The n members of a 100 000-member C3 draw with the smallest Qg_min, on a climate with `pscale` x the precipitation and
    1 / pscale x the PET of Tarland's: reaches that nearly dry up and are wetted again -- where the flow equation amplifies errors
    (include/simplyp_controller.h: SIMPLYP_CTRL_EXPAND)."""
    pr = synthetic.c3_problem(100000, seed=seed)
    pr['forcing'] = pr['forcing'].copy()
    pr['forcing'][:, 0] *= pscale
    pr['forcing'][:, 1] /= pscale
    sel = np.argsort(pr['member_params'][marshal.PM_NAMES.index('Qg_min')])[:n]
    return dict(pr, member_params=np.ascontiguousarray(pr['member_params'][:, sel]),
                reach_params=np.ascontiguousarray(pr['reach_params'][:, :, sel])), sel


@pytest.mark.parametrize('lanes', [1, 4])
def test_expansive_reach_on_a_drier_climate(engine0, lanes):
    """Round 3: on a climate with 0.6 x Tarland's precipitation 31 of 100 000 members were above 1e-6 (worst 8.6e-6), all among those
    with Qg_min ~ 0 on days when a nearly dry reach is wetted.  With the controller's expansive-reach rule the 256 driest members stay
    below 1e-6 against the same kernel at rtol 1e-11 (measured 4.2e-7), one lane and four lanes per member."""
    m, sel = dry_climate_members()
    m['opts'].lanes_per_member = lanes
    rtol, atol = m['opts'].rtol, m['opts'].atol
    m['opts'].rtol, m['opts'].atol = 1e-11, 1e-13
    truth, st, _ = gpu_run(engine0, m)
    assert st.max() == 0
    m['opts'].rtol, m['opts'].atol = rtol, atol
    got, st, stats = gpu_run(engine0, m)
    assert st.max() == 0 and stats['lanes_per_member'] == lanes
    worst = (np.abs(got - truth) / np.maximum(np.abs(truth), 1e-300)).max(axis=(0, 1, 2))
    assert worst.max() < 1e-6, (float(worst.max()), int(sel[worst.argmax()]))
    assert float(truth[1].min()) < 1e-3          # the reach does nearly dry up (Qr in mm/d)


@pytest.mark.parametrize('lanes', [1, 4])
def test_default_solver_in_the_dry_reach_regime_against_the_reference(engine0, lanes):
    """tests/golden/dry_members.npz: ten members of the dry-reach regime (0.6 x precipitation, Qg_min ~ 0, one draw with the time
    constants widened x/÷ 2) run through the unmodified reference at rtol=atol=1e-12 -- the regime of the controller's expansive-reach
    rule, pinned to the reference and not only to the kernel's own converged solution (VERDICT r3 / ADVICE r3).  Default solver,
    one and four lanes per member, north_star's bar on all 9 reach outputs over the two years around each member's worst day."""
    m, tables = helpers.dry_fixture_problem(solver=dict(lanes_per_member=lanes))
    got, st, stats = gpu_run(engine0, m)
    assert st.max() == 0 and stats['lanes_per_member'] == lanes
    worst = helpers.dry_worst_per_member(got, tables, marshal.OUT_COLUMNS)
    assert max(worst) < 1e-6, dict(zip(m['members'], worst))


@pytest.mark.parametrize('lanes', [1, 4])
def test_second_pair_on_a_stiff_reach_chain(engine0, oracle_lib, lanes):
    """opts.stiff_pair on the device (ck_day<SysAug, true>, ck_day_quad<true>): attempts bound by Cash-Karp's stability interval go, lane
    by lane, to the stability-optimised 4(3) pair, and the estimate of what a fast reach forgets is discounted (SIMPLYP_DAMP_*).  Config
    C4's chain (256 reaches, 16 members, 300 days): auto = on for a network; a third fewer right-hand sides than Cash-Karp alone, both
    within the bar against the converged solution; kernel == oracle (same rules, same counts up to accept/reject flips); one lane == four
    lanes bit for bit."""
    pr = synthetic.c4_problem(16, n_reaches=256, n_days=300, solver=dict(lanes_per_member=lanes))

    def run(stiff, rtol=None, atol=None, n_lanes=lanes):
        o = pr['opts']
        r0, a0 = o.rtol, o.atol
        if rtol:
            o.rtol, o.atol = rtol, atol
        o.stiff_pair, o.lanes_per_member = stiff, n_lanes
        try:
            out, status, stats = engine0.run(pr['forcing'], pr['doy'], pr['member_params'], pr['reach_params'], pr['up_ptr'], pr['up_idx'], o,
                                             out_reaches=pr['out_reaches'])
        finally:
            o.rtol, o.atol, o.stiff_pair, o.lanes_per_member = r0, a0, 0, lanes
        assert int(status.max()) == 0 and stats['lanes_per_member'] == n_lanes
        return out.cpu().numpy(), stats
    truth, _ = run(-1, 1e-11, 1e-13)
    off, s_off = run(-1)
    on, s_on = run(1)
    auto, s_auto = run(0)
    assert s_off['stiff_pair'] == 0 and s_on['stiff_pair'] == 1 and s_auto['stiff_pair'] == 1
    assert np.array_equal(auto, on, equal_nan=True) and s_auto['rhs_evals'] == s_on['rhs_evals']
    err = lambda a: float((np.abs(a - truth) / np.maximum(np.abs(truth), 1e-300)).max())
    assert err(off) < 5e-7 and err(on) < 5e-7, (err(off), err(on))
    # (a fifth fewer with the second pair alone; a third fewer with the damping-aware error weights the same switch turns on)
    assert s_on['rhs_evals'] < 0.75 * s_off['rhs_evals'], (s_on['rhs_evals'], s_off['rhs_evals'])
    # the CPU oracle mirrors the rule: two members of the run
    pick = [3, 11]
    sub = dict(pr, member_params=np.ascontiguousarray(pr['member_params'][:, pick]), reach_params=np.ascontiguousarray(pr['reach_params'][:, :, pick]))
    sub['opts'].stiff_pair = 1
    cref, cst, cstats = cpu_run(oracle_lib, sub, out_reaches=pr['out_reaches'], n_threads=2)
    sub['opts'].stiff_pair = 0
    assert cst.max() == 0 and helpers.max_rel_err(on[..., pick], cref, floor=FLOOR) < helpers.TOL_WORKING
    if lanes == 4:        # bit-identical to the one-lane kernel, second pair included
        one, s_one = run(1, n_lanes=1)
        assert np.array_equal(one, on, equal_nan=True) and s_one['rhs_evals'] == s_on['rhs_evals'] and s_one['rejected'] == s_on['rejected']


@pytest.mark.parametrize('fname', ['c4_members.npz', 'c4_deep.npz'])
@pytest.mark.parametrize('lanes', [1, 4])
def test_default_solver_on_members_of_the_c4_distribution_against_the_reference(engine0, lanes, fname):
    """tests/golden/c4_members.npz (4 members of config C4's own distribution on the upper 16 reaches of its chain, made by the
    unmodified reference at rtol=atol=1e-12) through the KERNEL, default solver with the second pair, one and four lanes per member:
    north_star's bar on all 9 reach columns.  c4_deep.npz: 2 members on the WHOLE 256-reach chain, reaches 32 / 64 / 128 / 192 / 256 --
    where a reach relaxes hundreds of times a day and the network scheme (second pair, damping-aware weights) does its work
    (oracle: 1.9e-7; Cash-Karp alone 2.7e-7)."""
    pr, tables = helpers.c4_members_problem(solver=dict(lanes_per_member=lanes), fname=fname)
    out, status, stats = engine0.run(pr['forcing'], pr['doy'], pr['member_params'], pr['reach_params'], pr['up_ptr'], pr['up_idx'], pr['opts'],
                                     out_reaches=pr['out_reaches'])
    assert int(status.max()) == 0 and stats['lanes_per_member'] == lanes and stats['stiff_pair'] == 1
    worst = helpers.c4_members_worst(out.cpu().numpy(), tables)
    assert max(worst.values()) < (5e-7 if fname == 'c4_deep.npz' else 1e-6), worst
