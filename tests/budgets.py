"""Mass balance: water, sediment and phosphorus budgets of a result table, from its 25 columns and the parameters alone -- no second integration.

Every budget is a list of signed terms, each an array [D, n_out, E] built from table columns, forcing and parameters; its residual is
|sum of the terms| / sum of |terms|, per (day, reach, member).  A state difference counts as two terms (the end value and the start
value), an integral that is itself derived from a store's budget as the terms it is made of: the residual is relative to the largest
quantity that takes part, which is what rounding can be held against.

Start-of-day values of day d are the row of day d - 1 (reference model.py:648-658, :702-703), except Vg, which restarts from Qg[d-1] * T_g
(:668-670); day 0 starts from the initial conditions (:377-459, restated in `initial_state`) or from a given state [S, 16, E]
(abi.STATE_ROWS, the layout of simplyp_set_state).

In the closable configuration (alpha = 0: no evapotranspiration, so the soil boxes' outflow integrals follow from their stores; k_M = 1:
sediment delivery is linear in Qr, so its integral is the Qr column) `residuals` closes water, sediment, PP and TDP per reach.  At any
parameters `ratio_identity` (PP and sediment inputs are both proportional to the integral of Qr^k_M) and `et_bracket` (what left as
evapotranspiration lies between 0 and alpha * PET) hold.

Pure NumPy; reads no oracle, no engine."""

import numpy as np

from simplyp_amd import abi, marshal

BUDGETS = ('water', 'sediment', 'PP', 'TDP')
ROW = {r: i for i, r in enumerate(abi.STATE_ROWS)}

# Bounds of the linear budgets (and of water where Vr is integrated literally): 10 x the CPU oracle's worst residual over every case of
# tests/test_budgets_host.py part (a) on its fp64 integrators (the measured value beside each; the factor allows for the kernel's
# reciprocals standing in for divisions, its fused day constants and more accepted steps per day).  None may exceed 1e-11.
MEASURED_FP64 = {'water': 6.94e-15, 'sediment': 8.97e-15, 'PP': 6.35e-15, 'TDP': 8.23e-15, 'ratio': 5.56e-15}
BOUND_FP64 = {k: 10.0 * v for k, v in MEASURED_FP64.items()}
# fp32 stages (integrator cashkarp_aug_f32): sediment and PP, measured on the oracle's same-arithmetic mirror; water and TDP get
# 10 x opts.rtol like every path that takes Vr from its invariant.
MEASURED_F32 = {'sediment': 5.25e-7, 'PP': 5.63e-7, 'ratio': 9.21e-8}
BOUND_F32 = {k: 10.0 * v for k, v in MEASURED_F32.items()}
CAP = 1e-11


def closable(member_params):
    """True when every member has alpha = 0 and k_M = 1."""
    mp = np.asarray(member_params)
    return bool((mp[marshal.PM_NAMES.index('alpha')] == 0.0).all() and (mp[marshal.PM_NAMES.index('k_M')] == 1.0).all())


def make_closable(member_params):
    """The same members with alpha = 0 and k_M = 1 (a copy)."""
    mp = np.array(member_params, dtype=np.float64)
    mp[marshal.PM_NAMES.index('alpha')] = 0.0
    mp[marshal.PM_NAMES.index('k_M')] = 1.0
    return mp


def bounds(opts, literal_vr):
    """{budget: bound on the relative residual} for a run with `opts`: BOUND_FP64 / BOUND_F32, and 10 x opts.rtol where the residual is
    the integrator's own error (water with Vr from its invariant; water and TDP under fp32 stages).  literal_vr: Vr is integrated as a
    state of its own and not re-imposed (rk4 or cashkarp with project_vr = 0)."""
    b = dict(BOUND_FP64)
    if opts.integrator == abi.INTEG_CASHKARP_AUG_F32:
        b.update(BOUND_F32, water=10.0 * opts.rtol, TDP=10.0 * opts.rtol)
    elif not literal_vr:
        b['water'] = 10.0 * opts.rtol
    return b


def literal_vr(opts):
    return opts.integrator in (abi.INTEG_RK4, abi.INTEG_CASHKARP) and not opts.project_vr


def initial_state(member_params, reach_params, opts):
    """[S, 16, E]: the reference's initial conditions (model.py:377-459) in the rows of abi.STATE_ROWS (h_next left 0)."""
    mp, rp = np.asarray(member_params, dtype=np.float64), np.asarray(reach_params, dtype=np.float64)
    M = lambda n: mp[marshal.PM_NAMES.index(n)][None, :]
    R = lambda n: rp[marshal.PR_NAMES.index(n)]
    S, E = rp.shape[1:]
    st = np.zeros((S, abi.N_STATE, E))
    A = R('A_catch')
    Qr0 = M('Qr0_init') * 86400 / (1000 * A[opts.sc_qr0][None, :])                       # :386
    st[:, ROW['VsA']] = st[:, ROW['VsS']] = M('fc')                                       # :377-378
    st[:, ROW['Vg']] = M('beta') * Qr0 * M('T_g')                                         # :389-390
    st[:, ROW['Qr']] = Qr0
    st[:, ROW['Vr']] = R('L_reach') / (M('a_Q') * Qr0 ** M('b_Q') * 8.64e4) * Qr0         # :457-459
    Msoil = M('Msoil_m2') * 10 ** 6 * A                                                   # :404
    epc0_A = M('EPC0_init_mgl_A') * A                                                     # :412
    plab_A = 1e-6 * (M('SoilPconc_A') - M('SoilPconc_S')) * Msoil                         # :415
    nc_S = (_f_NC_A(R) <= 0) & (R('f_NC_S') > 0)                                          # NC_type == 'S' (:321-335)
    st[:, ROW['Plab_A']] = plab_A
    st[:, ROW['TDPs_A']] = epc0_A * M('fc')                                               # :420
    st[:, ROW['Plab_NC']] = np.where(nc_S, plab_A, 0.0)                                   # :429-434
    st[:, ROW['TDPs_NC']] = np.where(nc_S, epc0_A * M('fc'), 0.0)
    st[:, ROW['conc_TDPs_A']] = epc0_A + 0.0 * M('fc')                                    # :438
    st[:, ROW['conc_TDPs_NC']] = np.where(nc_S, epc0_A, 0.0)                              # :446
    st[:, ROW['D_snow']] = M('D_snow_0') if opts.snow else 0.0
    return st


def _f_NC_A(R):
    return R('f_Ar') * R('f_NC_Ar') + R('f_NC_IG') * R('f_IG')                            # :319


class _Table(object):
    """A result table with its parameters lined up on the table's axes [D, n_out, E]: columns by name, start-of-day values, the
    per-day inputs, and which reaches have their upstream columns in the table."""

    def __init__(self, out, columns, forcing, member_params, reach_params, up_ptr, up_idx, opts, forcing_of_member=None,
                 out_reaches=None, member_of_slot=None, start=None):
        out = np.asarray(out, dtype=np.float64)
        mp, rp = np.asarray(member_params, dtype=np.float64), np.asarray(reach_params, dtype=np.float64)
        forcing = np.asarray(forcing, dtype=np.float64)
        S, E = rp.shape[1:]
        start = initial_state(mp, rp, opts) if start is None else np.asarray(start, dtype=np.float64)
        assert start.shape == (S, abi.N_STATE, E), start.shape
        fom = np.zeros(E, dtype=np.int64) if forcing_of_member is None else np.asarray(forcing_of_member, dtype=np.int64)
        if member_of_slot is not None:            # the table's member axis holds member mos[j] at position j
            mos = np.asarray(member_of_slot, dtype=np.int64)
            assert sorted(mos.tolist()) == list(range(E))
            mp, rp, start, fom = mp[:, mos], rp[:, :, mos], start[:, :, mos], fom[mos]
        reaches = list(range(S)) if out_reaches is None else [int(r) for r in out_reaches]
        columns = list(columns)
        assert out.shape[0] == len(columns) and out.shape[2] == len(reaches) and out.shape[3] == E, (out.shape, len(columns), len(reaches), E)
        self.D, self.n_out, self.E = out.shape[1:]
        self.T = float(opts.step_len)
        self.out, self.columns, self.reaches = out, columns, reaches
        self.rp, self.start = rp, start[reaches]
        self._mp = mp
        pos = {s: j for j, s in enumerate(reaches)}
        self.ups = [[int(u) for u in up_idx[up_ptr[s]:up_ptr[s + 1]]] for s in reaches]
        self.closed = np.array([all(u in pos for u in ups) for ups in self.ups], dtype=bool)
        self.up_pos = [[pos[u] for u in ups] if ok else [] for ups, ok in zip(self.ups, self.closed)]
        self.n_checked, self.n_skipped = int(self.closed.sum()), int((~self.closed).sum())
        # the hydrological input of every member and day [D, 1, E], and PET
        rain = forcing[fom, 0, :].T[:, None, :]
        self.PET = forcing[fom, 1, :].T[:, None, :]
        if opts.snow:                             # P = Precipitation - (D_snow[d] - D_snow[d-1]), reference inputs.py:183-208
            snow = self.col('D_snow')
            self.P = rain - (snow - self.prev(snow, 'D_snow'))
        else:
            self.P = rain + np.zeros((1, self.n_out, 1))

    def M(self, name):
        return self._mp[marshal.PM_NAMES.index(name)][None, None, :]

    def R(self, name):
        return self.rp[marshal.PR_NAMES.index(name)][self.reaches][None]

    def col(self, name):
        return self.out[self.columns.index(name)]

    def prev(self, x, state_row):
        """x of the day before; day 0 from the start state."""
        return np.concatenate([self.start[:, ROW[state_row]][None], x[:-1]], axis=0)

    def upstream(self, name, area_ratio=False):
        """sum over the directly upstream reaches of column `name` (x A_u / A for the flow, model.py:524-528)."""
        x, tot = self.col(name), np.zeros((self.D, self.n_out, self.E))
        A = self.rp[marshal.PR_NAMES.index('A_catch')]
        for j, ups in enumerate(self.up_pos):
            for u in ups:
                tot[:, j] += x[:, u] * (A[self.reaches[u]] / A[self.reaches[j]])[None] if area_ratio else x[:, u]
        return tot

    # ---- per-day coefficients ----
    def Esus(self):
        """(A, IG, S) sediment input coefficients, model.py:591-594, with the arable cover factor from its column."""
        k = self.M('E_M') * self.R('S_reach')
        return (k * self.R('S_Ar') * self.col('C_cover_A') * (1 - self.M('C_measures_A')),
                k * self.R('S_IG') * self.M('C_cover_IG') * (1 - self.M('C_measures_IG')),
                k * self.R('S_SN') * self.M('C_cover_S') * (1 - self.M('C_measures_S')))

    def Esum(self):
        eA, eIG, eS = self.Esus()
        return self.R('f_Ar') * eA + self.R('f_IG') * eIG + self.R('f_S') * eS           # model.py:141-143

    def cPP(self):
        """The PP input per unit Qr^k_M, model.py:171-176, with the labile P the day started from."""
        eA, eIG, eS = self.Esus()
        Msoil = self.M('Msoil_m2') * 10 ** 6 * self.R('A_catch')
        Pin = 1e-6 * self.M('SoilPconc_S') * Msoil
        plA = self.prev(self.col('P_labile_A_kg'), 'Plab_A')
        plNC = self.prev(self.col('P_labile_NC_kg'), 'Plab_NC')
        fAr, fIG, fS = self.R('f_Ar'), self.R('f_IG'), self.R('f_S')
        nAr, nIG, nS = self.R('f_NC_Ar'), self.R('f_NC_IG'), self.R('f_NC_S')
        return self.M('E_PP') * (fAr * (1 - nAr) * eA * (plA + Pin) / Msoil + fIG * (1 - nIG) * eIG * (plA + Pin) / Msoil
                                 + fS * (1 - nS) * eS * Pin / Msoil + fAr * nAr * eA * (plNC + Pin) / Msoil
                                 + fIG * nIG * eIG * (plNC + Pin) / Msoil + fS * nS * eS * (plNC + Pin) / Msoil)

    def reach_input(self, end, flux, state_row):
        """terms of (end-of-day mass - start-of-day mass + the day's outflow - T x what the upstream reaches sent)."""
        x = self.col(end)
        return [x, -self.prev(x, state_row), self.col(flux), -self.T * self.upstream(flux)]

    def relative(self, terms):
        terms = [np.broadcast_to(t, (self.D, self.n_out, self.E)) for t in terms]
        tot, scale = sum(terms), sum(np.abs(t) for t in terms)
        with np.errstate(divide='ignore', invalid='ignore'):
            r = np.where(scale > 0, np.abs(tot) / scale, 0.0)
        r[:, ~self.closed] = np.nan
        return r, scale


def _scaled(terms, c):
    return [c * t for t in terms]


def residuals(out, columns, forcing, member_params, reach_params, up_ptr, up_idx, opts, **kw):
    """({'water' | 'sediment' | 'PP' | 'TDP': relative residual [D, n_out, E]}, reaches checked, reaches skipped) of a table
    out[n_cols, D, n_out, E] in the closable configuration.  A reach whose upstream columns are not in the table (`out_reaches`) has NaN
    residuals and is counted as skipped.  Keywords: forcing_of_member, out_reaches (positions among the run's reaches), member_of_slot
    (the table's member axis is in slot order), start (the state [S, 16, E] the run started from; default: the initial conditions)."""
    if not closable(member_params):
        raise ValueError("the four budgets close only with alpha = 0 and k_M = 1 for every member")
    t = _Table(out, columns, forcing, member_params, reach_params, up_ptr, up_idx, opts, **kw)
    T, P, fq, beta = t.T, t.P, t.M('f_quick'), t.M('beta')
    fA, fS = t.R('f_Ar') + t.R('f_IG'), t.R('f_S')
    VsA, VsS, Vg, Vr = t.col('VsA'), t.col('VsS'), t.col('Vg'), t.col('Vr')
    # the integrals of the soil boxes' outflows and of Qg over the day, from their stores' own budgets (alpha = 0)
    IQsA = [T * P * (1 - fq), -VsA, t.prev(VsA, 'VsA')]
    IQsS = [T * P * (1 - fq), -VsS, t.prev(VsS, 'VsS')]
    IQsum = _scaled(IQsA, fA) + _scaled(IQsS, fS)
    Vg_start = np.concatenate([t.start[:, ROW['Vg']][None], (t.col('Qg') * t.M('T_g'))[:-1]], axis=0)    # model.py:668-670
    IQg = _scaled(IQsum, beta) + [-Vg, Vg_start]
    res = {}
    water = [Vr, -t.prev(Vr, 'Vr'), t.col('Qr'), -T * fq * P, -T * t.upstream('Qr', area_ratio=True)] \
        + _scaled(IQsum, -(1 - beta)) + _scaled(IQg, -1.0)
    res['water'], _ = t.relative(water)
    Qr = t.col('Qr')
    res['sediment'], _ = t.relative(t.reach_input('Msus_EndOfDay', 'Msus_kg/day', 'Msus') + [-t.Esum() * Qr])
    res['PP'], _ = t.relative(t.reach_input('PPr_EndOfDay', 'PP_kg/day', 'PPr') + [-t.cPP() * Qr])
    # TDP, model.py:154-166
    f_NC_A = _f_NC_A(lambda n: t.R(n))
    wA, wNC = fA * (1 - f_NC_A), fA * f_NC_A + fS * t.R('f_NC_S')
    cA = t.prev(t.col('conc_TDPs_A_kgmm'), 'conc_TDPs_A')
    cNC = t.prev(t.col('conc_TDPs_NC_kgmm'), 'conc_TDPs_NC')
    nc_A = f_NC_A > 0                                                                     # QsNC = QsA on NC type 'A', else QsS (:68)
    IQsNC = [np.where(nc_A, a, s) for a, s in zip(IQsA, IQsS)]
    tdpeff = np.nan_to_num(t.R('TDPeff'), nan=0.0)                                        # :462-463
    tdp = t.reach_input('TDPr_EndOfDay', 'TDP_kg/day', 'TDPr') \
        + _scaled(IQsA, -(1 - beta) * wA * cA) + _scaled(IQsNC, -(1 - beta) * wNC * cNC) \
        + [-T * fq * P * wA * cA, -T * fq * P * wNC * cNC, -T * tdpeff + 0.0 * P] \
        + _scaled(IQg, -t.M('TDPg') * t.R('A_catch'))
    res['TDP'], _ = t.relative(tdp)
    return res, t.n_checked, t.n_skipped


def ratio_identity(out, columns, forcing, member_params, reach_params, up_ptr, up_idx, opts, **kw):
    """(relative residual [D, n_out, E] of (PP input) x Esum - (sediment input) x cPP, reaches checked, reaches skipped): both inputs are
    their coefficient times the integral of Qr^k_M, at any parameters."""
    t = _Table(out, columns, forcing, member_params, reach_params, up_ptr, up_idx, opts, **kw)
    terms = _scaled(t.reach_input('PPr_EndOfDay', 'PP_kg/day', 'PPr'), t.Esum()) \
        + _scaled(t.reach_input('Msus_EndOfDay', 'Msus_kg/day', 'Msus'), -t.cPP())
    return t.relative(terms)[0], t.n_checked, t.n_skipped


def et_bracket(out, columns, forcing, member_params, reach_params, up_ptr, up_idx, opts, **kw):
    """(lower, upper, reaches checked, reaches skipped): the water that left as evapotranspiration, ET, and T x alpha x PET - ET, each
    [D, n_out, E] relative to the sum of the absolute terms of ET's budget; both are > 0 (to the integrator's tolerance) at any
    parameters."""
    t = _Table(out, columns, forcing, member_params, reach_params, up_ptr, up_idx, opts, **kw)
    T, P, fq = t.T, t.P, t.M('f_quick')
    fA, fS = t.R('f_Ar') + t.R('f_IG'), t.R('f_S')
    VsA, VsS, Vg, Vr = t.col('VsA'), t.col('VsS'), t.col('Vg'), t.col('Vr')
    Vg_start = np.concatenate([t.start[:, ROW['Vg']][None], (t.col('Qg') * t.M('T_g'))[:-1]], axis=0)
    terms = [T * P * ((fA + fS) * (1 - fq) + fq), -fA * VsA, fA * t.prev(VsA, 'VsA'), -fS * VsS, fS * t.prev(VsS, 'VsS'),
             -Vg, Vg_start, -Vr, t.prev(Vr, 'Vr'), -t.col('Qr'), T * t.upstream('Qr', area_ratio=True)]
    terms = [np.broadcast_to(x, (t.D, t.n_out, t.E)) for x in terms]
    et, scale = sum(terms), sum(np.abs(x) for x in terms)
    cap = T * t.M('alpha') * t.PET * (fA + fS)
    lower, upper = et / scale, (cap - et) / scale
    lower[:, ~t.closed] = np.nan
    upper[:, ~t.closed] = np.nan
    return lower, upper, t.n_checked, t.n_skipped


def worst(res):
    """{budget: max over the checked (day, reach, member)}"""
    return {k: float(np.nanmax(v)) for k, v in res.items()}
