"""The plain statement of the right-hand side (tests/rhs_model.py: mpmath, 40 digits) against the vectors the unmodified reference
produced, and the CPU oracle's three statements -- ode_f, ode_aug, ode_aug_f32 -- against it on every row the device is held to
(tests/test_gpu_rhs.py), under the same bound  |got_i - want_i| <= K u M_i + G_i  (rhs_model.py; K = 64).  No GPU.

What the statement must reproduce before it judges anything: the reference-made ode_dy within 8 u M_i without any gate allowance
(measured 2.8; a statement of other equations would miss by many orders of magnitude), and the oracle's ode_f at a few u M_i
(measured 2.0 on the fixture rows, 3.1 on the dry-reach and knee rows, again without allowance)."""

import numpy as np

import rhs_model as rm


def _oracle(fn, R):
    return np.array([fn(rm.y12_of(x), x[8:]) for x in R])


def test_statement_states_the_reference_equations():
    R, labels, _, _ = rm.rows()
    r = rm.truth().ratios(rm.V['ode_dy'], rm.ORACLE_F, rm.U64, rows=range(96), allowance=False)
    w = rm.worst(r, rm.ORACLE_F, labels[:96])
    print('reference ode_dy against the statement: worst %.2f u M in %s at %s (no gate allowance)' % w)
    assert w[0] <= 8.0, w


def test_oracle_ode_f_on_all_rows(oracle_lib):
    R, labels, _, _ = rm.rows()
    got = _oracle(oracle_lib.ode_f, R)
    bare = rm.truth().ratios(got, rm.ORACLE_F, rm.U64, allowance=False)
    print('oracle ode_f: worst %.2f u M on the fixture rows, %.2f in %s at %s on all rows (no gate allowance)'
          % ((float(np.nanmax(bare[:96])),) + rm.worst(bare, rm.ORACLE_F, labels)))
    w = rm.worst(rm.truth().ratios(got, rm.ORACLE_F, rm.U64), rm.ORACLE_F, labels)
    assert w[0] <= rm.K, w


def test_oracle_ode_aug_on_all_rows(oracle_lib):
    R, labels, _, _ = rm.rows()
    w = rm.worst(rm.truth().ratios(_oracle(oracle_lib.ode_aug, R), rm.AUG, rm.U64), rm.AUG, labels)
    print('oracle ode_aug: worst %.2f u M in %s at %s' % w)
    assert w[0] <= rm.K, w


def test_oracle_ode_aug_f32_on_all_rows(oracle_lib):
    R, labels, _, _ = rm.rows_f32()
    w = rm.worst(rm.truth_f32().ratios(_oracle(oracle_lib.ode_aug_f32, R), rm.AUG, rm.U32), rm.AUG, labels)
    print('oracle ode_aug_f32: worst %.2f u M (u = 2^-24) in %s at %s' % w)
    assert w[0] <= rm.K, w


def test_rows_cover_the_edges():
    R, labels, inv, below = rm.rows()
    assert 300 <= len(R) <= 900                                   # a few hundred: seconds on the device
    s = rm.truth().s
    for gate in range(3):                                         # every gate below / inside / above its zone, and on both knees
        col = s[:, gate]
        assert (col < 0).any() and ((col > 0) & (col < 1)).any() and (col > 1).any(), gate
        assert (np.abs(col) < 1e-10).any() and (np.abs(col - 1) < 1e-10).any(), gate
    assert set(R[:, 8 + rm.IX['NC_type']].astype(int)) == {0, 1, 2}
    nz = (R[:, 8 + rm.IX['f_NC_Ar']] > 0) & (R[:, 8 + rm.IX['f_NC_IG']] > 0) & (R[:, 8 + rm.IX['f_NC_S']] > 0)
    assert {int(t) for t in R[nz, 8 + rm.IX['NC_type']]} == {0, 1, 2}
    assert (R[:, 4] <= 1e-5).any() and (R[:, 4] >= 50.0).any()
    step = R[:, 8 + rm.IX['Qg_min']] == 0.0                       # Qg_min = 0: a plain step, rows on both sides of 0 and at 0
    assert (R[step, 2] < 0).any() and (R[step, 2] == 0).any() and (R[step, 2] > 0).any()
    assert ((R[:, 8 + rm.IX['P']] == 0) & (R[:, 8 + rm.IX['E']] == 0)).any() and (R[:, 8 + rm.IX['P']] == 80.0).any()
    up = R[:, 8 + rm.IX['Qr_US']]
    assert (up == 0).any() and (up > 0).any()
    assert inv.sum() > 300 and (~inv[96:]).sum() >= 40 and below.sum() == 12
    # the fp32 rows are the same rows as the fp32 form sees them
    R32 = rm.rows_f32()[0]
    assert np.array_equal(R32, R32.astype(np.float32).astype(np.float64)) and R32.shape == R.shape
