"""Per-member phosphorus and erosion parameters under static EPC0 and under the mixed new-land pairings.

The ensembles of the other GPU tests perturb the hydrological parameters (fc, T_g, a_Q, b_Q, k_M, T_s, beta, Qg_min); the soil-P and
erosion parameters reach the kernel with the workbook's one value in every lane.  Here 70 members of the two five-reach scenarios --
net5_static_2004 (static EPC0: EPC0 and the soil-water concentration of new land selected by the reach's own type and constant all
year, labile P of S-type new land starting from the agricultural value) and net5_dynamic_leakA_2004 (both dynamic options, S-type new
land on a last sub-catchment of type 'A') -- differ in exactly those: the initial EPC0 and soil P concentration of both land classes, the
net P inputs, E_PP, TDPg, the soil mass, the cover factor and the two days of maximum erodibility, the latter shifted by whole and half
days so that the erosion window's membership test (a whole number of days from its start) is never true for some members.

Bars: the file-wide ones of tests/test_gpu_parity.py -- kernel against the CPU oracle under fixed-step RK4 (no data-dependent control
flow) 1e-10 relative on all 25 columns; one lane against four lanes per member and chain kernel against task-queue kernel bit for bit
under the default solver."""

import numpy as np
import pytest

import helpers
from simplyp_amd import marshal

E = 70                  # one full wave of 64 lanes and a ragged one; 18 quads (the last wave of four-lane members ragged too)
FLOOR = 1e-12           # columns that are identically 0 compare absolutely (tests/test_gpu_parity.py)
SCALED = ['EPC0_init_mgl_A', 'EPC0_init_mgl_S', 'SoilPconc_A', 'SoilPconc_S', 'P_netInput_A', 'P_netInput_NC', 'E_PP', 'TDPg', 'Msoil_m2',
          'C_cover_A']
SHIFTED = ['d_maxE_spr', 'd_maxE_aut']
NAMES = ['net5_static_2004', 'net5_dynamic_leakA_2004']


def problem(name, solver=None):
    """The scenario with E members: member 0 keeps the workbook's values, the others have every parameter of SCALED multiplied by a
    seeded factor in [0.7, 1.4] and the two days of SHIFTED moved by a seeded multiple of half a day in [-20, 20]."""
    m = helpers.marshal_scenario(name, E=E, solver=solver)
    rng = np.random.default_rng(NAMES.index(name) + 61)
    mp = m['member_params']
    for par in SCALED:
        mp[marshal.PM_NAMES.index(par), 1:] *= rng.uniform(0.7, 1.4, E - 1)
    for par in SHIFTED:
        mp[marshal.PM_NAMES.index(par), 1:] += rng.integers(-40, 41, E - 1) / 2.0
    # Agricultural soil at or below the P concentration of semi-natural soil is outside the model's domain: a negative labile pool and, in
    # calibration mode, a negative Kf, on which dynamic EPC0 diverges within days (the oracle flags such members STATUS_NONFINITE).  About
    # one draw in thirty lands there; its two factors change places, which puts the larger one on the agricultural soil.
    a, s = mp[marshal.PM_NAMES.index('SoilPconc_A')], mp[marshal.PM_NAMES.index('SoilPconc_S')]
    a0, s0 = a[0], s[0]
    swap = a <= s
    a[swap], s[swap] = s[swap] / s0 * a0, a[swap] / a0 * s0
    marshal.validate_ensemble(mp, m['reach_params'], m['scs'])
    return m


def run(eng, m, **kw):
    out, status, stats = eng.run(m['forcing'], m['doy'], m['member_params'], m['reach_params'], m['up_ptr'], m['up_idx'], m['opts'], **kw)
    return out.cpu().numpy(), status.cpu().numpy(), stats


def test_the_members_differ_where_they_should():
    """What the draws hold (no GPU involved)."""
    for name in NAMES:
        mp = problem(name)['member_params']
        assert (mp[marshal.PM_NAMES.index('SoilPconc_A')] > mp[marshal.PM_NAMES.index('SoilPconc_S')]).all()
        for par in SHIFTED:
            d = mp[marshal.PM_NAMES.index(par)]
            half = d != np.floor(d)
            assert 10 < half.sum() < E - 10 and np.abs(d - d[0]).max() <= 20.0, par          # whole and half days, both well represented
        for par in SCALED:
            if mp[marshal.PM_NAMES.index(par), 0] == 0.0:          # the workbook's EPC0 of semi-natural land, where the scenario keeps it
                assert par == 'EPC0_init_mgl_S' and name == 'net5_dynamic_leakA_2004'
                continue
            r = mp[marshal.PM_NAMES.index(par)] / mp[marshal.PM_NAMES.index(par), 0]
            assert 0.7 <= r.min() < 0.8 and 1.3 < r.max() <= 1.4 and len(np.unique(r)) == E, par
    assert problem(NAMES[0])['opts'].dynamic_epc0 == 0 and problem(NAMES[1])['opts'].dynamic_epc0 == 1


@pytest.mark.gpu
@pytest.mark.parametrize('name', NAMES)
def test_kernel_matches_oracle_member_by_member_under_rk4(engine0, oracle_lib, name):
    m = problem(name, solver=dict(integrator='rk4', substeps=32))
    got, status, _ = run(engine0, m)
    ref, rstatus, _ = oracle_lib.run(m['forcing'], m['doy'], m['member_params'], m['reach_params'], m['up_ptr'], m['up_idx'], m['opts'],
                                     n_threads=8)
    assert status.max() == 0 and rstatus.max() == 0 and np.isfinite(ref).all()
    col = marshal.OUT_COLUMNS.index
    # the parameters do reach the columns they feed: new land's EPC0 on the S-type reach 1 and the A-type reach 2, labile P of new land,
    # the cover factor and the PP flux differ from member to member
    for c, reach in (('EPC0_NC_kgmm', 0), ('EPC0_NC_kgmm', 1), ('P_labile_NC_kg', 0), ('conc_TDPs_NC_kgmm', 1), ('C_cover_A', 4),
                     ('PP_kg/day', 4), ('TDP_kg/day', 4)):
        v = ref[col(c), -1, reach]
        assert len(np.unique(v)) > E // 2 and (v != 0).all(), (c, reach)
    worst = {c: helpers.max_rel_err(got[ci], ref[ci], floor=FLOOR) for ci, c in enumerate(marshal.OUT_COLUMNS)}
    print('%s, rk4 x 32, kernel vs oracle: worst %.2e (%s)' % (name, max(worst.values()), max(worst, key=worst.get)))
    assert max(worst.values()) < 1e-10, worst


@pytest.mark.gpu
@pytest.mark.parametrize('name', NAMES)
def test_lanes_and_kernels_agree_bit_for_bit_under_the_default_solver(engine0, name):
    import torch
    res = {}
    for lanes, chunk in ((1, -1), (4, -1), (1, 64), (4, 64)):
        m = problem(name, solver=dict(lanes_per_member=lanes, time_chunk_days=chunk, balance=0))
        rhs = torch.zeros(E, dtype=torch.int32, device='cuda')
        out, status, stats = run(engine0, m, member_rhs=rhs)
        assert stats['lanes_per_member'] == lanes and stats['queued'] == (chunk > 0) and status.max() == 0
        res[lanes, chunk] = (out, rhs.cpu().numpy(), (stats['rhs_evals'], stats['steps'], stats['rejected']))
    ref = res[1, -1]
    assert np.isfinite(ref[0]).all() and len(np.unique(ref[1])) > E // 2          # the members do take different steps
    for key, got in res.items():
        assert np.array_equal(got[0], ref[0]), (key, float(np.abs(got[0] - ref[0]).max()))
        assert np.array_equal(got[1], ref[1]) and got[2] == ref[2], key
