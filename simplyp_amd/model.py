"""SimplyP model entry points on the MI355X engine.

Drop-in for the reference's ``Current_Release/v0-2A/simplyP/model.py``:
``run_simply_p`` keeps the signature, return types, column names, in-place
edits of ``p_LU``/``p_SC``, printed lines and error cases of model.py:193-827,
but the sub-catchment x day loop nest (model.py:365-724) runs as one batched HIP
launch sequence behind the C ABI (``engine.py``).  ``run_simply_p_ensemble`` is
the batched entry the reference does not have.

The three scalar helpers ``f_x``, ``discretized_soilP`` and ``ode_f`` are kept
as plain Python for API compatibility (``__init__.py`` of the reference exports
them); they are not used by ``run_simply_p``.
"""

import os
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pandas as pd

from . import abi, engine, ensemble, marshal, request, residuals, weighted
from . import forcing as forcing_rules
from . import helper_functions as hf, pareto as pareto_rules, score as score_rules, visualise_results as vr


# ------------------------------------------------------------------------------------------
# scalar helpers kept for API compatibility (reference model.py:23-187)

def f_x(x, threshold, reld):
    """Smooth 0..1 gate above ``threshold`` (reference model.py:23-37)."""
    d = threshold * reld
    if x < threshold:
        return 0
    if x > threshold + d:
        return 1
    s = (x - threshold) / d
    return -2 * s**3 + 3 * s**2


def discretized_soilP(P_netInput, catchment_area, SC, Kf, Msoil, EPC0, Qs, Qq, Vs, TDPs, Plab):
    """One-day closed-form update of soil-water TDP and labile soil P (reference model.py:39-56)."""
    a = P_netInput * catchment_area * 100 / 365. + Kf * Msoil * EPC0
    b = (Kf * Msoil + Qs + Qq) / Vs
    TDPs = a / b + (TDPs - a / b) * np.exp(-b)
    b0 = b * Vs
    if Vs > 0:
        sorp = Kf * Msoil * (a / b0 - EPC0 + (1 / b) * (TDPs / Vs - a / b0) * (1 - np.exp(-b)))
    else:
        sorp = 0.
    Plab = Plab + sorp
    return (TDPs, Plab)


def ode_f(y, t, ode_params):
    """Right-hand side of the 12-variable daily system, same argument tuple as the reference
    (model.py:58-187).  Python convenience only; the engine evaluates this on the GPU."""
    (P, E, mu, Qq_i, Qr_US_i, Esus_i, Msus_US_i, TDPr_US_i, PPr_US_i,
     f_A, f_Ar, f_IG, f_S, f_NC_A, f_NC_Ar, f_NC_IG, f_NC_S, NC_type,
     f_quick, alpha, beta, T_s, T_g, fc, L_reach, A_catch,
     a_Q, b_Q, E_M, k_M, conc_TDPs_A, conc_TDPs_NC, PlabA_i, PlabNC_i,
     Msoil, TDPeff, TDPg, E_PP, P_inactive, dynamic_EPC0, Qg_min) = ode_params
    VsA, VsS, Vg, Vr, Qr = y[0], y[1], y[2], y[3], y[4]
    Msus, TDPr, PPr = y[6], y[8], y[10]
    QsA = (VsA - fc) * f_x(VsA, fc, 0.01) / T_s['A']
    dVsA = P * (1 - f_quick) - alpha * E * (1 - np.exp(-mu * VsA)) - QsA
    QsS = (VsS - fc) * f_x(VsS, fc, 0.01) / T_s['S']
    dVsS = P * (1 - f_quick) - alpha * E * (1 - np.exp(-mu * VsS)) - QsS
    QsNC = QsA if NC_type == 'A' else QsS
    f_Qg = f_x(Vg / T_g, Qg_min, 0.01)
    Qg = (1 - f_Qg) * Qg_min + f_Qg * (Vg / T_g)
    Qsum = f_A * QsA + f_S * QsS
    dVg = beta * Qsum - Qg
    inflow = Qq_i + (1 - beta) * Qsum + Qg + Qr_US_i - Qr
    dQr = inflow * a_Q * (Qr**b_Q) * 86400. / ((1 - b_Q) * L_reach)
    QrkM = Qr**k_M
    MA, MS, MIG = Esus_i['A'] * QrkM, Esus_i['S'] * QrkM, Esus_i['IG'] * QrkM
    out_M, out_T, out_P = (Msus / Vr) * Qr, Qr * (TDPr / Vr), Qr * PPr / Vr
    dMsus = f_Ar * MA + f_IG * MIG + f_S * MS + Msus_US_i - out_M
    dTDPr = ((1 - beta) * (f_A * (1 - f_NC_A) * QsA * conc_TDPs_A + f_A * f_NC_A * QsNC * conc_TDPs_NC
                           + f_S * f_NC_S * QsNC * conc_TDPs_NC)
             + f_A * (1 - f_NC_A) * Qq_i * conc_TDPs_A + f_A * f_NC_A * Qq_i * conc_TDPs_NC
             + f_S * f_NC_S * Qq_i * conc_TDPs_NC
             + Qg * hf.UC_Cinv(TDPg, A_catch) + TDPeff + TDPr_US_i - out_T)
    dPPr = (E_PP * (f_Ar * (1 - f_NC_Ar) * MA * (PlabA_i + P_inactive) / Msoil
                    + f_IG * (1 - f_NC_IG) * MIG * (PlabA_i + P_inactive) / Msoil
                    + f_S * (1 - f_NC_S) * MS * P_inactive / Msoil
                    + f_Ar * f_NC_Ar * MA * (PlabNC_i + P_inactive) / Msoil
                    + f_IG * f_NC_IG * MIG * (PlabNC_i + P_inactive) / Msoil
                    + f_S * f_NC_S * MS * (PlabNC_i + P_inactive) / Msoil)
            + PPr_US_i - out_P)
    return np.array([dVsA, dVsS, dVg, inflow, dQr, Qr, dMsus, out_M, dTDPr, out_T, dPPr, out_P])


# ------------------------------------------------------------------------------------------
# post-processing (reference model.py:831-900)

def derived_P_species(df_R, f_TDP):
    """TP = TDP + PP and SRP = f_TDP * TDP, for fluxes and concentrations (reference model.py:831-847)."""
    df_R['TP_mgl'] = df_R['TDP_mgl'] + df_R['PP_mgl']
    df_R['TP_kg/day'] = df_R['TDP_kg/day'] + df_R['PP_kg/day']
    df_R['SRP_mgl'] = df_R['TDP_mgl'] * f_TDP
    df_R['SRP_kg/day'] = df_R['TDP_kg/day'] * f_TDP
    return df_R


def sum_to_waterbody(p_struc, n_SC, df_R_dict, f_TDP):
    """Sum the reaches flagged 'In_final_flux?' into one series (reference model.py:851-900)."""
    vars_to_sum = ['Q_cumecs', 'Msus_kg/day', 'TDP_kg/day', 'PP_kg/day']
    reaches_in_final_flux = p_struc['In_final_flux?'][p_struc['In_final_flux?'] == 1].index.values
    if len(reaches_in_final_flux) > n_SC:
        raise ValueError("Mismatch between the number of subcatchments in the 'Setup' parameter sheet \n(parameter 'n_SC') and in the 'Reach_structure' parameter sheet")
    print('Sub-catchments flowing directly into receiving waterbody: %s' % reaches_in_final_flux)
    if len(reaches_in_final_flux) > 1:
        index = df_R_dict[reaches_in_final_flux[0]].index
        df_summed = pd.DataFrame(
            {var: np.sum([df_R_dict[r][var].to_numpy(dtype=float) for r in reaches_in_final_flux], axis=0)
             for var in vars_to_sum}, index=index, columns=vars_to_sum)
        df_summed['SS_mgl'] = (df_summed['Msus_kg/day'] / df_summed['Q_cumecs']) * (1000. / 86400.)
        df_summed['TDP_mgl'] = (df_summed['TDP_kg/day'] / df_summed['Q_cumecs']) * (1000. / 86400.)
        df_summed['PP_mgl'] = (df_summed['PP_kg/day'] / df_summed['Q_cumecs']) * (1000. / 86400.)
        df_summed = derived_P_species(df_summed, f_TDP)
        return df_summed
    else:
        print('One or fewer reaches were selected to be included in the sum, check your reach structure parameters')
        return None


# ------------------------------------------------------------------------------------------
# the hot path

def _engine_opts(p_SU, p, dynamic_options, step_len, solver, out_mask, n_periods=0, snow=False):
    scs = marshal.sc_list(p)
    return abi.make_opts(solver,
                         dynamic_epc0=(dynamic_options['Dynamic_EPC0'] == 'y'),
                         dynamic_erod=(dynamic_options['Dynamic_erodibility'] == 'y'),
                         run_mode_cal=(p_SU.run_mode == 'cal'),
                         sc_qr0=scs.index(int(p['SC_Qr0'])),
                         out_mask=out_mask, step_len=step_len, n_periods=n_periods, snow=snow)


class _DeviceEnsemble(object):
    """An ensemble of ``E`` workbook members, marshalled and uploaded once -- forcing, ``doy``, ``member_params``, ``reach_params``,
    ``f_tdp`` -- with the options of a table of ``columns``.  Its callers keep members in their own order: ``out_slot_order`` is refused."""

    def __init__(self, order, met_df, p_SU, p_LU, p_SC, p, dynamic_options, step_len, solver, device, E, columns, snow, n_periods=0):
        self.mask = marshal.mask_of_columns(columns)
        self.opts = _engine_opts(p_SU, p, dynamic_options, step_len, solver, self.mask, n_periods=n_periods, snow=snow)
        if self.opts.out_slot_order:
            raise ValueError("%s: solver['out_slot_order'] must stay 0" % order)
        self.eng = eng = engine.get_engine(device)
        self.torch = torch = eng.torch
        self.f64 = dict(dtype=torch.float64, device=eng.tdev)
        forcing, doy = marshal.forcing_arrays(met_df, snow=snow)
        self.f_d, self.doy_d = eng.to_device(forcing, torch.float64), eng.to_device(doy, torch.int32)
        self.mp_d = eng.to_device(marshal.member_params(p, p_LU, E), torch.float64)
        self.rp_d = eng.to_device(marshal.reach_params(p_SC, p, E), torch.float64)
        self.ft_d = torch.full((E,), float(p['f_TDP']), **self.f64)

    def write_positions(self, theta_d, target):
        """The positions ``theta_d[n_dim, E]`` into the run's arrays: row ``target[d]`` of ``member_params``, or ``f_tdp``."""
        for d in range(len(target)):
            if target[d] >= 0:
                self.mp_d[int(target[d])].copy_(theta_d[d])
            elif target[d] == abi.MCMC_TARGET_F_TDP:
                self.ft_d.copy_(theta_d[d])


def _kf_last(p_SU, p_LU, p_SC, p):
    """Kf as the reference returns it: the value of the last sub-catchment (model.py:449-453, :827)."""
    SC = marshal.sc_list(p)[-1]
    if p_SU.run_mode == 'cal':
        return 10**-6 * (p_LU['A']['SoilPconc'] - p_LU['S']['SoilPconc']) / \
            hf.UC_Cinv(p_LU['A']['EPC0_init_mgl'], p_SC.loc['A_catch', SC])
    return p['Kf']


def _output_dict(stats, status, solver):
    """The 4th return value.  The reference hands back LSODA's infodict of its LAST odeint call (model.py:640, :827: last
    sub-catchment, last day) -- arrays of one element under 'nst', 'nfe', 'nje', 'hu', ..., and 'message'.  LSODA is not what
    integrates here, so the engine's own statistics are returned, and the keys a caller of the reference could have read are
    kept as aliases with the same types: 'nfe' (right-hand-side evaluations), 'nst' (accepted steps), 'nje' (Jacobian
    evaluations: none, the pair is explicit) as one-element int32 arrays -- totals over the whole run, not the last day's
    call; saturating at 2**31 - 1 (a large network exceeds int32: the exact totals are under 'rhs_evals' / 'steps') --,
    'mused' (1 = non-stiff method) and 'message' ('Integration successful.' unless the member was flagged)."""
    msg = 'Integration successful.'
    if status & abi.STATUS_NONFINITE:
        msg = 'Non-finite state met (member status %d); results from that day on are NaN.' % status
    elif status & abi.STATUS_STEPCAP:
        msg = 'Excess work done on a day (max_steps attempts; member status %d).' % status
    d = dict(stats, member_status=status, solver=dict(abi.DEFAULT_SOLVER, **(solver or {})), engine='MI355X batched engine',
             message=msg)
    i32max = np.iinfo(np.int32).max
    d['nfe'] = np.array([min(int(stats['rhs_evals']), i32max)], dtype=np.int32)
    d['nst'] = np.array([min(int(stats['steps']), i32max)], dtype=np.int32)
    d['nje'] = np.array([0], dtype=np.int32)
    d['mused'] = np.array([1], dtype=np.int32)
    return d

def _state_blocks(initial_state, scs, E, index, bounds):
    """Checks an ``initial_state`` (the ``'state'`` dict of an earlier result, or a bare array / device tensor [S, 16, E], or
    a list of per-block tensors split as ``bounds``) against the run it is to start -- host only, before any device call --
    and returns one array per member block of ``bounds``."""
    S = len(scs)
    data = initial_state
    if isinstance(initial_state, dict):
        data = initial_state['data']
        if [int(r) for r in initial_state['reaches']] != [int(r) for r in scs]:
            raise ValueError("initial_state holds reaches %s, the run has %s" % (list(initial_state['reaches']), list(scs)))
        if list(initial_state.get('rows', abi.STATE_ROWS)) != list(abi.STATE_ROWS):
            raise ValueError("initial_state rows %s are not abi.STATE_ROWS" % (list(initial_state['rows']),))
        end = initial_state.get('end')
        if end is not None:
            first, want = pd.Timestamp(index[0]), pd.Timestamp(end) + pd.Timedelta(days=1)
            if first != want:
                raise ValueError("initial_state ends on %s, so the run must start on %s; met_df starts on %s"
                                 % (pd.Timestamp(end).date(), want.date(), first.date()))
    if isinstance(data, (list, tuple)):
        blocks = list(data)
        if len(blocks) != len(bounds) or any(tuple(b.shape) != (S, abi.N_STATE, hi - lo) for b, (lo, hi) in zip(blocks, bounds)):
            raise ValueError("initial_state blocks %s do not match [S=%d, %d, members of each device block %s]"
                             % ([tuple(b.shape) for b in blocks], S, abi.N_STATE, [hi - lo for lo, hi in bounds]))
        return blocks
    if tuple(data.shape) != (S, abi.N_STATE, E):
        raise ValueError("initial_state must have shape [S, %d, E] = %s, got %s" % (abi.N_STATE, (S, abi.N_STATE, E), tuple(data.shape)))
    if len(bounds) == 1:
        return [data]
    return [data[..., lo:hi] for lo, hi in bounds]


def _noise_blocks(initial_state, E, bounds):
    """The forcing noise state an ``initial_state`` dict carries under ``'forcing_noise'`` ([6, E], or a list of per-block
    tensors split as ``bounds``) as one table per member block of ``bounds``; None -- a stationary start -- for a dict without
    it, a bare array or None.  Host only."""
    noise = initial_state.get('forcing_noise') if isinstance(initial_state, dict) else None
    if noise is None:
        return None
    n = len(abi.FORCING_NOISE_ROWS)
    if isinstance(noise, (list, tuple)):
        blocks = list(noise)
        if len(blocks) != len(bounds) or any(tuple(b.shape) != (n, hi - lo) for b, (lo, hi) in zip(blocks, bounds)):
            raise ValueError("initial_state['forcing_noise'] blocks %s do not match [%d, members of each device block %s]"
                             % ([tuple(b.shape) for b in blocks], n, [hi - lo for lo, hi in bounds]))
        return blocks
    if tuple(noise.shape) != (n, E):
        raise ValueError("initial_state['forcing_noise'] must have shape [%d, E] = %s, got %s" % (n, (n, E), tuple(noise.shape)))
    if len(bounds) == 1:
        return [noise]
    return [noise[:, lo:hi] for lo, hi in bounds]


def run_simply_p(met_df, p_struc, p_SU, p_LU, p_SC, p, dynamic_options, step_len=1., solver=None, device=0,
                 initial_state=None, return_state=False):
    """Simple hydrology, sediment and phosphorus model (reference model.py:193-827).

    Same arguments and 4-tuple return ``(df_TC_dict, df_R_dict, Kf, output_dict)`` as the
    reference.  Extra keyword arguments: ``solver`` (dict overriding ``abi.DEFAULT_SOLVER``:
    integrator 'cashkarp'|'rk4', rtol, atol, substeps, max_steps, project_vr) and ``device``.
    ``output_dict`` holds the engine's solver statistics, with LSODA's infodict keys ``nfe``, ``nst``, ``nje``, ``mused``,
    ``message`` kept as aliases (``_output_dict``).  ``initial_state`` / ``return_state``: warm start, as in
    ``run_simply_p_ensemble`` -- the model state after the last day comes back as ``output_dict['state']``, and a later
    call over the following dates given that dict as ``initial_state`` continues the run bit for bit.
    """

    # derived parameters, validation, in-place edits of p_LU / p_SC (model.py:311-361)
    with marshal.reference_edits(p_SU, p_LU, p_SC, p):
        scs = marshal.sc_list(p)
        up_ptr, up_idx, up_lists = marshal.topology(p_struc, p)
        mp = marshal.member_params(p, p_LU, 1)
        rp = marshal.reach_params(p_SC, p, 1)
        forcing, doy = marshal.forcing_arrays(met_df)
        opts = _engine_opts(p_SU, p, dynamic_options, step_len, solver, marshal.MASK_ALL)
        st_in = None if initial_state is None else _state_blocks(initial_state, scs, 1, met_df.index, [(0, 1)])[0]

        eng = engine.get_engine(device)          # raises when the HIP library / device is missing
        out_d, status_d, stats = eng.run(forcing, doy, mp, rp, up_ptr, up_idx, opts, state_in=st_in,
                                         state_out=True if return_state else None)
        state_d = stats.pop('state', None)
        out = out_d.cpu().numpy()                # [25, D, S, 1]
        status = int(status_d.cpu().numpy()[0])

    df_TC_dict, df_R_dict = {}, {}
    for j, SC in enumerate(scs):
        print('Starting model run for sub-catchment: %s' % SC)                               # :367
        if len(up_lists[SC]) > 0:
            print('Reaches directly upstream of this reach: %s' % up_lists[SC])              # :512
        else:
            print('No reaches directly upstream of this reach')                              # :542
        A_catch = p_SC.loc['A_catch', SC]
        df_ODE = pd.DataFrame(out[:12, :, j, 0].T, columns=marshal.ODE_COLUMNS, index=met_df.index)       # :736-740
        df_nonODE = pd.DataFrame(out[12:, :, j, 0].T, columns=marshal.NONODE_COLUMNS, index=met_df.index)  # :742-746

        df_TC = pd.concat([df_ODE[['VsA', 'VsS', 'Vg']], df_nonODE], axis=1)                  # :755
        df_TC['TDPs_A_mgl'] = hf.UC_C(df_TC['conc_TDPs_A_kgmm'], A_catch)                     # :758
        df_TC['EPC0_A_mgl'] = hf.UC_C(df_TC['EPC0_A_kgmm'], A_catch)                          # :759
        df_TC['Plabile_A_mgkg'] = (10**6 * df_TC['P_labile_A_kg'] / (p['Msoil_m2'] * 10**6 * A_catch))   # :760-761
        if p_SC.loc['NC_type', SC] != 'None':                                                # :764-773
            if p_SC.loc['NC_type', SC] == 'A':
                df_TC['VsNC'] = df_TC['VsA']
                df_TC['QsNC'] = df_TC['QsA']
            else:
                df_TC['VsNC'] = df_TC['VsS']
                df_TC['QsNC'] = df_TC['QsS']
            df_TC['TDPs_NC_mgl'] = hf.UC_C(df_TC['conc_TDPs_NC_kgmm'], A_catch)
            df_TC['Plabile_NC_mgkg'] = (10**6 * df_TC['P_labile_NC_kg'] / (p['Msoil_m2'] * 10**6 * A_catch))
        if p_SU.inc_snowmelt == 'y':                                                         # :775-776
            df_TC['D_snow'] = met_df['D_snow_end']

        df_R = df_ODE.drop(['VsA', 'VsS', 'Vg'], axis=1)                                      # :779
        df_R['Q_cumecs'] = df_R['Qr'] * A_catch * 1000 / 86400                                # :784
        df_R['SS_mgl'] = hf.UC_C(df_R['Msus_kg/day'] / df_R['Qr'], A_catch)                   # :788
        df_R['TDP_mgl'] = hf.UC_C(df_R['TDP_kg/day'] / df_R['Qr'], A_catch)                   # :789
        df_R['PP_mgl'] = hf.UC_C(df_R['PP_kg/day'] / df_R['Qr'], A_catch)                     # :790
        df_R = derived_P_species(df_R, p['f_TDP'])                                            # :793

        df_TC_dict[SC] = df_TC.sort_index(axis=1)                                             # :797-800
        df_R_dict[SC] = df_R.sort_index(axis=1)
        print('Finished!\n')                                                                  # :802

    Kf = _kf_last(p_SU, p_LU, p_SC, p)
    if p_SU.run_mode == 'cal':                                                               # :809-812
        print("Running in calibration mode; the soil P sorption coefficient has been estimated as %s mm/kg\n" % Kf)
    else:
        print("Running in validation or scenario mode, so the soil P sorption coefficient has been read from the parameter file")

    if p_SU.save_output_csvs == 'y':                                                         # :815-825
        out_dir = p_SU.output_fpath.replace('\\', os.sep) if isinstance(p_SU.output_fpath, str) else p_SU.output_fpath
        for SC in df_R_dict.keys():
            df_TC_dict[SC].to_csv(os.path.join(out_dir, "Results_TC_SC%s.csv" % SC))
            df_R_toSave = df_R_dict[SC].drop(['Msus_EndOfDay', 'PPr_EndOfDay', 'Qr',
                                              'Qr_EndOfDay', 'TDPr_EndOfDay', 'Vr'], axis=1)
            df_R_toSave.to_csv(os.path.join(out_dir, "Instream_results_Reach%s.csv" % SC))
        print('Results saved to csv\n')

    output_dict = _output_dict(stats, status, solver)
    if state_d is not None:
        output_dict['state'] = dict(rows=list(abi.STATE_ROWS), reaches=list(scs), data=state_d.cpu().numpy(), end=met_df.index[-1])
    return (df_TC_dict, df_R_dict, Kf, output_dict)                                          # :827


def _host_table(shape, pin):
    """Host array that receives an ensemble's output table: page-locked (the streamed copies then run at PCIe speed beside the
    kernel) when the host can lock that much -- not more than 60 % of what it has available, the guard bench.py applies --
    else an ordinary pageable array, which ``simplyp_stream_out`` accepts too (slower copies, same table)."""
    nbytes = int(np.prod(shape, dtype=np.int64)) * 8
    avail = None
    try:
        with open('/proc/meminfo') as fh:
            for line in fh:
                if line.startswith('MemAvailable:'):
                    avail = int(line.split()[1]) * 1024
    except OSError:
        pass
    if avail is None or nbytes <= 0.6 * avail:
        try:
            return pin(shape)
        except engine.EngineError:
            pass
    return np.empty(shape, dtype=np.float64)

# ------------------------------------------------------------------------------------------
# run_simply_p_ensemble in stages: request (keywords, then inputs) -> block pass per device -> assembly

class _Request(object):
    """What one ``run_simply_p_ensemble`` call asks for: its arguments under their own names (``_request``) and what the inputs make
    of them (``_bind_*``).  Once bound it is read-only: the block passes, one host thread per device, share it and nothing else."""

    def __init__(self, **kw):
        self.__dict__.update(kw, bound=False)

    def __setattr__(self, name, value):
        if self.bound:
            raise AttributeError("the request is read-only once bound (%s)" % name)
        self.__dict__[name] = value


class _Bands(namedtuple('_Bands', 'q weighted to_host')):
    """The one adapter of bands across the members, weighted or not -- of the table's rows, the waterbody series, the per-member
    time quantiles and the predictive series: ``select`` is the device call, ``result`` the dict the caller gets."""

    def select(self, eng, table, include, weights, series=None, mask=None, **kw):
        """(lower, upper, info) of ``table``'s rows, or of the predictive ``series`` made from it; under ``weights`` one array, twice."""
        if series is not None:
            got = eng.predictive_bands(table, mask, self.q, series, include=include, weights=weights, **kw)
        elif weights is None:
            got = eng.quantiles(table, self.q, include=include, **kw)
        else:
            got = eng.weighted_quantiles(table, self.q, weights, include=include, **kw)
        return got if weights is None else (got[0], got[0], got[1])

    def result(self, lower, upper, info):
        lo_h, up_h = lower.cpu().numpy(), upper.cpu().numpy()
        # under weights there is one value per probability: nothing to interpolate
        data = lo_h if self.weighted else engine.interpolate_quantiles(lo_h, up_h, self.q, info['n_used'])
        res = dict(q=list(self.q), data=data, lower=lo_h if self.to_host else lower, upper=up_h if self.to_host else upper,
                   n_members=info['n_used'], info=info)
        return dict(res, rule='inverted_cdf', weight_total=int(info['T'])) if self.weighted else res


def _request(**kw):
    """Request, part 1: every check that needs nothing but the keyword arguments -- no input is read, no device touched."""
    r = _Request(**kw)
    if r.quantiles is not None:
        if r.devices is not None:
            raise ValueError("quantiles cannot be combined with devices=[...]: a quantile of the whole ensemble is not a function "
                             "of the member blocks' quantiles -- run the band on one device")
        r.quantiles = request.probabilities('quantiles', r.quantiles)
    elif r.quantile_members is not None and not r.score and r.pareto is None:
        raise ValueError("quantile_members given without quantiles")
    if r.score:
        if r.obs_dict is None:
            raise ValueError("score needs obs_dict: the observations the forecast is judged against")
        if r.reduce is not None:
            raise ValueError("score needs the daily series: it cannot be combined with reduce")
        if r.devices is not None:
            raise ValueError("score cannot be combined with devices=[...]: a score of the whole ensemble is not a function of the "
                             "member blocks' scores -- run it on one device")
    if r.residual_lag and r.obs_dict is None:
        raise ValueError("residual_lag needs obs_dict: the observations the residuals are taken against")
    if r.pareto is not None:
        if r.obs_dict is None:
            raise ValueError("pareto needs obs_dict: the objectives are rows of the goodness-of-fit table")
        if r.devices is not None:
            raise ValueError("pareto cannot be combined with devices=[...]: dominance spans the whole ensemble, it is not a "
                             "function of the member blocks' results -- run it on one device")
        r.pareto_max_fronts = int(r.pareto_max_fronts)
        if r.pareto_max_fronts < 0:
            raise ValueError("pareto_max_fronts must be >= 0")
    if r.quantile_weights is not None and r.quantile_log_weights is not None:
        raise ValueError("quantile_weights and quantile_log_weights are mutually exclusive")
    r.weighted_band = r.quantile_weights is not None or r.quantile_log_weights is not None
    if r.weighted_band and r.quantiles is None and not r.score:
        raise ValueError("quantile_weights / quantile_log_weights given without quantiles")
    r.tq_names = r.tq_ids = r.tq_pod = r.tq_labels = r.pr_names = r.pr_ids = None
    r.tq_needs = r.pr_needs = []
    if r.time_quantiles is None:
        if r.time_quantile_series is not None or r.time_quantile_periods is not None:
            raise ValueError("time_quantile_series / time_quantile_periods given without time_quantiles")
    else:
        if r.reduce is not None:
            raise ValueError("time_quantiles needs the daily series: it cannot be combined with reduce")
        r.time_quantiles = request.probabilities('time_quantiles', r.time_quantiles)
        names = list(r.time_quantile_series) if r.time_quantile_series is not None else \
            (list(r.outputs) if r.outputs is not None else list(marshal.REACH5_COLUMNS))
        r.tq_names, r.tq_ids, r.tq_needs = request.series_ids('time_quantile_series', names)
        r.tq_labels, r.tq_pod = request.skipping_periods('time_quantile_periods', r.time_quantile_periods)
    if r.predictive_series is None:
        if r.predictive_m is not None and not r.score:
            raise ValueError("predictive_m given without predictive_series")
    else:
        if r.quantiles is None and not r.score:
            raise ValueError("predictive_series needs quantiles: the probabilities of the bands")
        if r.reduce is not None:
            raise ValueError("predictive_series needs the daily series: it cannot be combined with reduce")
        if r.devices is not None:
            raise ValueError("predictive_series cannot be combined with devices=[...]: a band across the whole ensemble is not a "
                             "function of the member blocks' bands")
        r.pr_names, r.pr_ids, r.pr_needs = request.series_ids('predictive_series', r.predictive_series)
        if isinstance(r.predictive_m, dict) and [c for c in r.predictive_m if c not in r.pr_names]:
            raise ValueError("predictive_m names series that predictive_series does not: %s"
                             % [c for c in r.predictive_m if c not in r.pr_names])
    if r.pr_names is not None or r.score:
        r.predictive_seed, r.predictive_day0 = int(r.predictive_seed), int(r.predictive_day0)
        if not 0 <= r.predictive_seed < 1 << 64 or not 0 <= r.predictive_day0 < 1 << 31:
            raise ValueError("predictive_seed must be in [0, 2^64) and predictive_day0 in [0, 2^31)")
    if r.score and isinstance(r.predictive_m, dict) and r.pr_names is None and \
            [c for c in r.predictive_m if c not in abi.TQ_DERIVED_SERIES]:
        raise ValueError("predictive_m names series that are not df_R series: %s"
                         % [c for c in r.predictive_m if c not in abi.TQ_DERIVED_SERIES])
    r.pr_bands = r.pr_names is not None and r.quantiles is not None
    r.bands = None if r.quantiles is None else _Bands(r.quantiles, r.weighted_band, r.to_host)
    # the caller's product is a reduction of the table: keep_daily=False then drops the table itself
    r.reduced_on_device = r.obs_dict is not None or r.quantiles is not None or r.time_quantiles is not None
    r.want_host_table = r.to_host and (r.keep_daily or not r.reduced_on_device)
    return r


def _bind_members(r):
    """Request, part 2a: the ensemble -- size, band members and weights, the blocks of ``devices``, start states, parameters, forcing."""
    r.scs, r.up_ptr, r.up_idx = marshal.catchment(r.p_struc, r.p)[:3]
    overrides = dict(r.overrides or {})
    f_tdp = overrides.pop('f_TDP', None)
    m_over, r_over = marshal.split_member_reach_overrides(overrides)
    sizes = {np.asarray(v).shape[-1] for v in list(m_over.values()) + list(r_over.values()) + [f_tdp] if v is not None and np.ndim(v) > 0}
    if r.n_members is None:
        if len(sizes) != 1:
            raise ValueError("cannot infer the ensemble size: give n_members or override arrays of one length")
        r.n_members = sizes.pop()
    r.E = E = int(r.n_members)
    if r.quantile_members is not None:
        r.quantile_members = np.ascontiguousarray(np.asarray(r.quantile_members) != 0)
        if r.quantile_members.shape != (E,):
            raise ValueError("quantile_members needs one flag per member")
    r.q_lin = r.lw_all = r.pr_m = None
    if r.quantile_weights is not None:               # the filter's integers, on the host
        w_ = np.asarray(r.quantile_weights, dtype=np.float64)
        if w_.shape != (E,):
            raise ValueError("quantile_weights needs one weight per member")
        r.q_lin = weighted.linear_weights(w_).astype(np.int64)
    if r.quantile_log_weights is not None:           # ... on the device, where the run lies
        r.lw_all = np.ascontiguousarray(np.asarray(r.quantile_log_weights, dtype=np.float64))
        if r.lw_all.shape != (E,):
            raise ValueError("quantile_log_weights needs one log weight per member")
        if not np.isfinite(r.lw_all).any():
            raise ValueError("quantile_log_weights: no log weight is finite, so all weights are zero")
    if r.predictive_m is not None and r.pr_names is not None:
        r.pr_m = request.error_model_rows(r.predictive_m, r.pr_names, E)
    met_sets = list(r.met_df) if isinstance(r.met_df, (list, tuple)) else [r.met_df]
    r.met_df = met_sets[0]
    if r.snow_in_kernel is None:
        r.snow_in_kernel = 'f_DDSM' in m_over or 'D_snow_0' in m_over
    r.forcing_error = forcing_rules.resolve(r.forcing_error, r.met_df.index, E, r.snow_in_kernel, r.forcing_seed)
    if r.devices is None:
        r.bounds = [(0, E)]
    else:
        if not list(r.devices):
            raise ValueError("devices must name at least one GPU")
        r.bounds = [b_ for b_ in (ensemble.shard_bounds(E, len(r.devices), k) for k in range(len(r.devices))) if b_[1] > b_[0]]
    r.state_blocks = None if r.initial_state is None else _state_blocks(r.initial_state, r.scs, E, r.met_df.index, r.bounds)
    r.noisy = forcing_rules.any_rho(r.forcing_error)             # autocorrelated forcing errors: a noise state travels with the model's
    r.noise_blocks = _noise_blocks(r.initial_state, E, r.bounds) if r.noisy else None
    # the SoA arrays are marshalled straight into page-locked host memory: the uploads are asynchronous DMA transfers
    r.pin = engine.pinned_empty
    r.mp = marshal.member_params(r.p, r.p_LU, E, m_over, alloc=r.pin)
    r.rp = marshal.reach_params(r.p_SC, r.p, E, r_over, alloc=r.pin)
    if m_over or r_over:
        marshal.validate_ensemble(r.mp, r.rp, r.scs)       # the reference's checks, for every member (model.py:321-335, :355-357)
    for m in met_sets:
        if r.snow_in_kernel and not {'Precipitation', 'T_air'} <= set(m.columns):
            raise ValueError("the in-kernel snow module needs met_df columns 'Precipitation' and 'T_air'")
        if not m.index.equals(r.met_df.index):
            raise ValueError("all forcing sets must cover the same dates")
    if len(met_sets) > 1:
        if r.forcing_of_member is None:
            raise ValueError("several forcing sets need forcing_of_member (one set index per member)")
        fom = r.forcing_of_member = np.ascontiguousarray(r.forcing_of_member, dtype=np.int32)
        if fom.shape != (E,) or fom.min() < 0 or fom.max() >= len(met_sets):
            raise ValueError("forcing_of_member needs one index in [0, %d) per member" % len(met_sets))
    elif r.forcing_of_member is not None:
        raise ValueError("forcing_of_member given but met_df is a single forcing set")
    sets = [marshal.forcing_arrays(m, snow=r.snow_in_kernel) for m in met_sets]
    r.forcing, r.doy = np.ascontiguousarray(np.concatenate([f for f, _ in sets], axis=0)), sets[0][1]
    r.ft_all = r.p['f_TDP'] if f_tdp is None else f_tdp


def _bind_outputs(r):
    """Request, part 2b: the table (columns, ``mask``, waterbody, periods, options, reaches) and what is held against it; then read-only."""
    index, scs = r.met_df.index, r.scs
    cols = list(r.outputs) if r.outputs is not None else list(marshal.REACH5_COLUMNS)
    r.wb_reaches, out_reaches = None, r.out_reaches
    if r.waterbody is not None and r.waterbody is not False:
        if r.reduce is not None:
            raise ValueError("the waterbody sum needs the daily series: waterbody cannot be combined with reduce")
        if r.waterbody is True:
            flags = r.p_struc['In_final_flux?']
            r.wb_reaches = [int(x) for x in flags[flags == 1].index.values]                    # model.py:867
            if len(r.wb_reaches) > len(scs):                                                     # :871-872
                raise ValueError("Mismatch between the number of subcatchments in the 'Setup' parameter sheet \n(parameter 'n_SC') and in the 'Reach_structure' parameter sheet")
        else:
            r.wb_reaches = sorted(int(x) for x in r.waterbody)
        print('Sub-catchments flowing directly into receiving waterbody: %s' % np.asarray(r.wb_reaches))   # :874
        if out_reaches is not None:
            out_reaches = list(out_reaches) + [x for x in r.wb_reaches if x not in out_reaches]
    if r.obs_dict is not None or r.wb_reaches is not None:
        if r.reduce is not None:
            raise ValueError("goodness of fit needs the daily series: obs_dict cannot be combined with reduce")
        cols += [c for c in marshal.FLUX_COLUMNS if c not in cols]
    cols += [c for c in r.tq_needs if c not in cols]
    if isinstance(r.time_quantile_periods, str):
        r.tq_labels, r.tq_pod = request.annual_periods(index)
    if r.tq_pod is not None and r.tq_pod.shape != (len(index),):
        raise ValueError("time_quantile_periods needs one period index per day")
    cols += [c for c in r.pr_needs if c not in cols]
    r.mask = marshal.mask_of_columns(cols)
    if r.mask & marshal.MASK_D_SNOW and not r.snow_in_kernel:
        raise ValueError("output 'D_snow' is the per-member snow depth of the in-kernel snow module: needs snow_in_kernel=True "
                         "(without it every member shares met_df['D_snow_end'])")
    r.periods, r.period_of_day = (None, None) if r.reduce is None else request.reduce_periods(r.reduce, index)
    r.opts = _engine_opts(r.p_SU, r.p, r.dynamic_options, r.step_len, r.solver, r.mask,
                          n_periods=0 if r.periods is None else len(r.periods), snow=r.snow_in_kernel)
    r.reaches = scs if out_reaches is None else list(out_reaches)            # the waterbody may have added to them since
    r.oreach = None if out_reaches is None else [scs.index(int(x)) for x in out_reaches]
    r.table_shape = (bin(r.mask).count('1'), len(index) if r.periods is None else len(r.periods), len(r.reaches))
    r.wb_sum = r.wb_reaches is not None and len(r.wb_reaches) > 1
    r.obs = None if r.obs_dict is None else vr.observation_array(r.obs_dict, r.reaches, index)
    r.wobs = vr.observation_array({0: r.waterbody_obs}, [0], index)[0] if r.wb_sum and r.waterbody_obs is not None else None
    r.sc_names = r.sc_ids = r.sc_obs = r.sc_m = r.pa_resolved = None
    if r.score:                                      # [n_series, D, n_reaches]: the layout simplyp_predictive_scores takes
        r.sc_names, r.sc_ids, r.sc_obs = request.observed_series(r.obs_dict, r.reaches, r.obs, r.pr_names)
        if r.sc_names and r.predictive_m is not None:
            r.sc_m = request.error_model_rows(r.predictive_m, r.sc_names, r.E)
    if r.pareto is not None:
        r.pa_resolved = pareto_rules.resolve_objectives(r.pareto, n_reaches=len(r.reaches), has_spearman=bool(r.spearman))
    r.bound = True


def _block_pass(r, eng, lo, hi):
    """Members [lo, hi) on one engine context: the run, then the reductions that want the table where it lies."""
    mask, to_host = r.mask, r.to_host
    keep = (lambda t: t.cpu().numpy()) if to_host else (lambda t: t)                         # a device result as the caller gets it
    whole = (lo == 0 and hi == r.E)
    st_in = None
    if r.state_blocks is not None:
        st_in = r.state_blocks[r.bounds.index((lo, hi))]
        st_in = st_in.contiguous() if hasattr(st_in, 'contiguous') else np.ascontiguousarray(st_in, dtype=np.float64)
    nz_in = None
    if r.noise_blocks is not None:
        nz_in = r.noise_blocks[r.bounds.index((lo, hi))]
        nz_in = nz_in.contiguous() if hasattr(nz_in, 'contiguous') else np.ascontiguousarray(nz_in, dtype=np.float64)
    mp_b = r.mp if whole else np.ascontiguousarray(r.mp[:, lo:hi])
    rp_b = r.rp if whole else np.ascontiguousarray(r.rp[:, :, lo:hi])
    fom_b = None if r.forcing_of_member is None else np.ascontiguousarray(r.forcing_of_member[lo:hi])
    ft = r.ft_all if np.ndim(r.ft_all) == 0 else np.ascontiguousarray(np.asarray(r.ft_all, dtype=np.float64)[lo:hi])
    rp_d = eng.to_device(rp_b)
    # to_host: the table is delivered into page-locked host memory while the kernel runs (simplyp_stream_out) -- unless the
    # caller only wants the statistics (keep_daily=False)
    host_out = _host_table(r.table_shape + (hi - lo,), r.pin) if r.want_host_table else None
    out_d, status_d, stats = eng.run(r.forcing, r.doy, mp_b, rp_d, r.up_ptr, r.up_idx, r.opts, out_reaches=r.oreach,
                                     period_of_day=r.period_of_day, forcing_of_member=fom_b, host_out=host_out,
                                     state_in=st_in, state_out=True if r.return_state else None,
                                     forcing_error=forcing_rules.member_block(r.forcing_error, lo, hi),
                                     forcing_noise_in=nz_in, forcing_noise_out=True if r.return_state and r.noisy else None)
    state_d = stats.pop('state', None)
    part = dict(stats=stats, state=state_d, status=keep(status_d), host_out=host_out, device=eng.device,
                noise=stats.pop('forcing_noise', None))
    mos = stats.get('member_of_slot') if r.opts.out_slot_order else None
    tkw = dict(f_tdp=ft, reach_params=rp_d, out_reaches=r.oreach, member_of_slot=mos)       # how a reduction reads the table
    if r.obs is not None:
        gof_d, info = eng.gof(out_d, mask, r.obs, spearman=r.spearman, **tkw)
        rho = info.pop('spearman', None)
        part['gof'] = (keep(gof_d), info, None if rho is None else keep(rho))
        if r.residual_lag:
            lag_d, linfo = eng.gof_lag(out_d, mask, r.obs, **tkw)
            part['lag'] = (keep(lag_d), linfo)
    if r.wb_sum:
        wb_d, winfo = eng.waterbody(out_d, mask, [r.scs.index(x) for x in r.wb_reaches], **tkw)
        part['wb'] = (keep(wb_d), winfo)
        if r.wobs is not None:
            g_d, ginfo = eng.gof_waterbody(wb_d, winfo['columns'], r.wobs, ft, member_of_slot=mos)
            part['wb_gof'] = (keep(g_d), ginfo)
    if r.quantiles is not None or r.score or r.pareto is not None:
        # who takes part: a mask in member order, built where the status lies; and with which weight
        inc = (status_d & abi.STATUS_NONFINITE) == 0
        if r.quantile_members is not None:
            inc = inc & eng.to_device(r.quantile_members[lo:hi])
        q_w = None if r.q_lin is None else eng.to_device(r.q_lin)
        if r.lw_all is not None:
            q_w = eng.pf_weights(eng.to_device(r.lw_all))[1]
    if r.pa_resolved is not None:                # the goodness-of-fit table is in member order whatever the run's is
        part['pareto'] = eng.pareto(pareto_rules.objective_rows(gof_d, rho, r.pa_resolved), [o['sense'] for o in r.pa_resolved],
                                    include=inc, max_fronts=r.pareto_max_fronts)
    if r.quantiles is not None:
        part['quant'] = r.bands.select(eng, out_d, inc, q_w, member_of_slot=mos)
        if 'wb' in part:
            part['wb_quant'] = r.bands.select(eng, wb_d, inc, q_w, member_of_slot=mos)
    if r.time_quantiles is not None:
        lo_d, up_d, tinfo = eng.time_quantiles(out_d, mask, r.time_quantiles, series=r.tq_ids, period_of_day=r.tq_pod,
                                               n_periods=None if r.tq_labels is None else len(r.tq_labels), **tkw)
        if mos is not None:                      # member order, undone on the small result: slot j holds member mos[j]
            idx = mos.long()
            lo_d, up_d = lo_d.new_empty(lo_d.shape).index_copy_(-1, idx, lo_d), up_d.new_empty(up_d.shape).index_copy_(-1, idx, up_d)
        lo_h, up_h = lo_d.cpu().numpy(), up_d.cpu().numpy()
        tdata = engine.interpolate_time_quantiles(lo_h, up_h, r.time_quantiles, tinfo['n_days'])
        part['tq'] = (lo_h if to_host else lo_d, up_h if to_host else up_d, tdata, tinfo)
        if r.quantiles is not None:              # the band across the members of the per-member statistics
            part['tq_quant'] = r.bands.select(eng, eng.to_device(tdata), inc, q_w)
    pkw = dict(tkw, seed=r.predictive_seed, day0=r.predictive_day0)
    if r.sc_ids is not None:                     # the scores of the observed rows: parameter-only, and with the error model drawn
        skw = dict(pkw, include=inc, weights=q_w)
        part['scores'] = (eng.predictive_scores(out_d, mask, r.sc_ids, r.sc_obs, **skw),
                          None if r.sc_m is None else eng.predictive_scores(out_d, mask, r.sc_ids, r.sc_obs, err_m=r.sc_m, **skw))
    if r.pr_bands:                               # the bands of the named series: parameter-only, and with the error model drawn
        part['pred'] = (r.bands.select(eng, out_d, inc, q_w, series=r.pr_ids, mask=mask, **pkw),
                        None if r.pr_m is None else r.bands.select(eng, out_d, inc, q_w, series=r.pr_ids, mask=mask, err_m=r.pr_m, **pkw))
    part['out_d'] = None if (r.reduced_on_device and not r.keep_daily) else out_d
    return part


def _run_blocks(r):
    """One ``_block_pass`` per member block: on ``device``, or at the same time on the entries of ``devices``."""
    if r.devices is None:
        return [_block_pass(r, engine.get_engine(r.device), 0, r.E)]
    devs = [int(d) for d in r.devices]
    if r.opts.out_slot_order:
        raise ValueError("devices=[...] returns tables in member order: solver['out_slot_order'] must stay 0")
    all_bounds = [ensemble.shard_bounds(r.E, len(devs), k) for k in range(len(devs))]
    # one context per list entry (a repeated id gets a context of its own: contexts are not re-entrant)
    engs = [engine.get_engine(d, replica=devs[:k].count(d)) for k, d in enumerate(devs)]
    live = [(eng, lo, hi) for eng, (lo, hi) in zip(engs, all_bounds) if hi > lo]
    if len(live) == 1:
        return [_block_pass(r, *live[0])]
    with ThreadPoolExecutor(max_workers=len(live)) as pool:
        return list(pool.map(lambda a_: _block_pass(r, *a_), live))


def _merged_stats(parts, bounds):
    """``res['stats']``: the one block's, or sums / maxima over the blocks with the per-block dicts under ``'per_device'``."""
    per = [pt['stats'] for pt in parts]
    stats = per[0]
    if len(per) > 1:
        stats = {k: sum(d_[k] for d_ in per) for k in ('rhs_evals', 'steps', 'rejected', 'n_launches', 'streamed_chunks',
                                                         'queue_waits')}
        stats.update({k: max(d_[k] for d_ in per) for k in ('kernel_ms', 'pilot_ms', 'wall_ms', 'd2h_tail_ms',
                                                            'queue_longest_wait_polls', 'queue_longest_stall_polls')})
        for k in ('balanced', 'queued', 'lanes_per_wave', 'lanes_per_member'):
            stats[k] = per[0][k]
        stats['simt_efficiency'] = float(np.mean([d_['simt_efficiency'] for d_ in per]))
        stats['per_device'] = [dict(d_, device=int(pt['device']), members=[int(lo), int(hi)])
                               for d_, pt, (lo, hi) in zip(per, parts, bounds)]
    stats['bounds'] = [[int(lo), int(hi)] for lo, hi in bounds]
    return stats


def _assemble(r, parts):
    """The result dict from the blocks' parts: per-member products joined along the member axis, bands through ``r.bands``."""
    to_host, first = r.to_host, parts[0]
    cat = (lambda xs: np.concatenate(xs, axis=-1)) if to_host else (lambda xs: xs[0] if len(xs) == 1 else _torch_cat(xs))
    gof_result = lambda key: dict(stats=list(abi.GOF_STATS), variables=list(abi.GOF_VARS), info=first[key][1],
                                  data=cat([pt[key][0] for pt in parts]))
    res = dict(columns=marshal.columns_of_mask(r.mask), reaches=r.reaches, periods=r.periods,
               stats=_merged_stats(parts, r.bounds), status=cat([pt['status'] for pt in parts]))
    if r.obs is not None:
        res['gof'] = gof_result('gof')
        if first['gof'][2] is not None:          # Spearman's r [6, n_reaches, E]: the rank statistic of the reference's table (:444-445)
            res['gof']['spearman'] = cat([pt['gof'][2] for pt in parts])
        if r.residual_lag:
            lag = cat([pt['lag'][0] for pt in parts])
            tail, cross = lag[abi.LAG_STATS.index('sq_tail')], lag[abi.LAG_STATS.index('cross')]
            res['residual_lag'] = dict({k: lag[i] for i, k in enumerate(abi.LAG_STATS)}, variables=list(abi.GOF_VARS),
                                       phi_hat=residuals.phi_hat(tail, cross) if to_host else cross / tail, info=first['lag'][1])
    if r.wb_sum:
        winfo = first['wb'][1]
        res['waterbody'] = dict(columns=winfo['columns'], reaches=r.wb_reaches, info=winfo, data=cat([pt['wb'][0] for pt in parts]))
        if r.wobs is not None:
            res['waterbody']['gof'] = gof_result('wb_gof')
    elif r.wb_reaches is not None:
        print('One or fewer reaches were selected to be included in the sum, check your reach structure parameters')   # :896
        res['waterbody'] = None
    if r.quantiles is not None:
        res['quantiles'] = r.bands.result(*first['quant'])
        if r.wb_sum:
            res['waterbody']['quantiles'] = r.bands.result(*first['wb_quant'])
    if r.pa_resolved is not None:
        res['pareto'] = pareto_rules.result(first['pareto'], r.pa_resolved)
    if r.score:
        res['scores'] = _scores_result(r.sc_names, r.reaches, r.sc_obs, len(r.met_df), first.get('scores'), r.predictive_seed,
                                       r.predictive_day0)
    if r.pr_bands:
        po, ov = first['pred']
        po_b, ov_b = r.bands.result(*po), None if ov is None else r.bands.result(*ov)
        info = dict(param_only=po_b.pop('info'), overall=None if ov_b is None else ov_b.pop('info'))
        extra = dict(rule=po_b['rule'], weight_total=po_b['weight_total']) if r.weighted_band else {}
        for b_ in (po_b, ov_b):
            if b_ is not None:
                del b_['q'], b_['n_members']
        res['predictive'] = dict(q=list(r.quantiles), series=list(r.pr_names), param_only=po_b, overall=ov_b,
                                 n_members=po[2]['n_used'], seed=r.predictive_seed, day0=r.predictive_day0, info=info, **extra)
    if r.time_quantiles is not None:
        tinfo = first['tq'][3]
        res['time_quantiles'] = dict(q=list(r.time_quantiles), series=list(r.tq_names), periods=r.tq_labels,
                                     lower=cat([pt['tq'][0] for pt in parts]), upper=cat([pt['tq'][1] for pt in parts]),
                                     data=np.concatenate([pt['tq'][2] for pt in parts], axis=-1),
                                     n_days=np.asarray(tinfo['n_days']), info=tinfo)
        if r.quantiles is not None:
            res['time_quantiles']['quantiles'] = r.bands.result(*first['tq_quant'])
    if r.return_state:
        sts = [pt['state'] for pt in parts]
        if r.return_state == 'device':
            sdata = sts[0] if len(sts) == 1 else sts
        elif to_host:
            sdata = np.concatenate([t.cpu().numpy() for t in sts], axis=-1)
        else:
            sdata = cat(sts)
        res['state'] = dict(rows=list(abi.STATE_ROWS), reaches=list(r.scs), data=sdata, end=r.met_df.index[-1])
        if r.noisy:                                  # the forcing noise state, delivered as the model state is
            nzs = [pt['noise'] for pt in parts]
            if r.return_state == 'device':
                res['state']['forcing_noise'] = nzs[0] if len(nzs) == 1 else nzs
            elif to_host:
                res['state']['forcing_noise'] = np.concatenate([t.cpu().numpy() for t in nzs], axis=-1)
            else:
                res['state']['forcing_noise'] = cat(nzs)
    if r.reduced_on_device and not r.keep_daily:
        res['data'] = None
    elif not to_host:
        res['data'] = first['out_d'] if len(parts) == 1 else [pt['out_d'] for pt in parts]
    elif len(parts) == 1:
        res['data'] = first['host_out']
    else:                                        # one table in member order: every block's copied into its member range, then freed
        res['data'] = np.empty(r.table_shape + (r.E,), dtype=np.float64)

        def place(pt, lo, hi):
            res['data'][..., lo:hi] = pt.pop('host_out')
        with ThreadPoolExecutor(max_workers=len(parts)) as pool:
            list(pool.map(place, parts, *zip(*r.bounds)))
    return res


def run_simply_p_ensemble(met_df, p_struc, p_SU, p_LU, p_SC, p, dynamic_options, overrides=None, n_members=None,
                          outputs=None, out_reaches=None, step_len=1., solver=None, device=0, to_host=True,
                          reduce=None, obs_dict=None, keep_daily=True, snow_in_kernel=None, forcing_of_member=None,
                          waterbody=None, waterbody_obs=None, spearman=False, devices=None, quantiles=None,
                          quantile_members=None, initial_state=None, return_state=False, time_quantiles=None,
                          time_quantile_series=None, time_quantile_periods=None, predictive_series=None, predictive_m=None,
                          predictive_seed=0, predictive_day0=0, quantile_weights=None, quantile_log_weights=None, score=False,
                          pareto=None, pareto_max_fronts=0, forcing_error=None, forcing_seed=0, residual_lag=False):
    """Run an ensemble of parameter sets through the engine in one call.

    ``overrides``: dict name -> array[E] (member parameters, see ``marshal.PM_NAMES``) or
    array broadcastable to [S, E] (reach parameters, ``marshal.PR_NAMES``); parameters not
    listed take the workbook value for every member.  ``outputs``: list of reference column
    names (default: the five documented reach outputs, model.py:272-277); with the in-kernel snow module also ``'D_snow'``,
    every member's snow depth at the end of the day (what the reference returns as ``df_TC['D_snow']``, model.py:775-776).  ``out_reaches``:
    sub-catchment ids to return (default all).  ``reduce``: None for daily rows, ``'annual'`` for one row
    per calendar year holding the sum of that year's daily values (e.g. annual fluxes), or an int array
    [D] of period indices; the periods are returned under ``'periods'``.
    ``met_df`` may also be a list of met dataframes over the same dates (forcing scenarios: climate members, bias-corrected
    series ...) with ``forcing_of_member`` [E] giving each member's scenario; all sets sit in HBM once and members read theirs.
    ``snow_in_kernel``: run the degree-day snow module (reference ``snow_hydrol_inputs``, inputs.py:159-210) per member
    inside the kernel from ``met_df['Precipitation']`` / ``['T_air']`` instead of taking ``met_df['P']``; default: on when
    ``overrides`` perturbs ``f_DDSM`` or ``D_snow_0`` (with the workbook values the result is bit-identical either way).
    ``obs_dict``: observations as returned by ``read_input_data`` (dict SC -> DataFrame with columns among
    Q, SS, TDP, PP, TP, SRP): every member's goodness-of-fit table (the reference's ``goodness_of_fit_stats``,
    visualise_results.py:387-474, minus Spearman's r, plus the two sums of its Gaussian likelihood) is reduced on the
    device from the daily series and returned under ``'gof'`` = dict(stats, variables, data[n_stats, 6, n_reaches, E],
    info); needs daily rows (``reduce=None``); the four flux columns are added to ``outputs`` when missing.  ``SRP``
    uses ``p['f_TDP']`` or ``overrides['f_TDP']`` (array[E]).  ``spearman=True`` adds the table's rank statistic under
    ``['gof']['spearman']`` [6, n_reaches, E] (counted on the device, ~0.1-0.2 s for 100 000 members).  ``keep_daily=False`` drops the daily table once the
    statistics exist (``data`` is None): the 44 GB of a 100 000-member run never leave the device.
    ``residual_lag=True`` (needs ``obs_dict``): the autocorrelation check the reference's calibration notebook ends with
    (Development/2016/MCMC.ipynb cell 21), for every member and without a table transfer -- the lag-one sums of the relative
    residuals ``obs / sim - 1`` over the days whose predecessor is observed too (``simplyp_gof_lag``; ``simplyp_amd.residuals``
    states them) under ``'residual_lag'`` = dict(variables, n_link, sq_head, sq_tail, cross -- each [6, n_reaches, E] --,
    phi_hat = cross / sq_tail, the conditional maximum-likelihood lag-one coefficient, info).  A device reduction like the
    goodness of fit: it works with ``keep_daily=False`` and with ``devices=[...]``, and per window in
    ``run_simply_p_ensemble_windows``, where a link does not cross a window's edge (a window's first day has no predecessor).

    ``waterbody``: the reference's ``sum_to_waterbody`` (model.py:851-900) for every member, on the device: ``True`` sums
    the sub-catchments flagged ``p_struc['In_final_flux?'] == 1``, a list sums the given sub-catchment ids.  Like the
    reference, fewer than two reaches give ``None`` (:872, :895).  The result comes back under ``'waterbody'`` =
    dict(columns (the reference's 11: ``abi.WB_COLUMNS``), reaches, data[11, D, E], info); needs daily rows and adds the
    four flux columns / the summed reaches to the outputs when missing.  ``waterbody_obs``: DataFrame of observations
    at the waterbody's inflow (columns among Q, SS, TDP, PP, TP, SRP): the members' goodness-of-fit table of the summed
    series under ``['waterbody']['gof']``.

    ``devices``: a list of GPU ids, e.g. ``[0, 1, ..., 7]`` -- the ensemble is split into contiguous member blocks
    (``ensemble.shard_bounds``), one per entry, and the blocks run at the same time from this one process: one engine context and
    one host thread per entry (ctypes releases the GIL), every block's table streamed over its own GPU's PCIe link, the
    goodness-of-fit / waterbody reductions done where the block's table lies.  No process group, no ``torchrun``: a notebook call
    (SURVEY.md section 8b's ``devices=`` argument; what the reference's only ensemble caller did with an ``IPython.parallel`` pool,
    Development/2016/MCMC.ipynb:30-31, :379-385).  Members are independent, so every table is bit-identical to the one-device
    run's.  An id may repeat (``[0, 0]``: two contexts on one GPU).  ``device`` is ignored when ``devices`` is given.
    ``stats`` then holds sums / maxima over the blocks and the per-block dicts under ``'per_device'``; with ``to_host=False``
    ``data`` is the list of the blocks' device tensors (member axis split as ``stats['bounds']``).

    ``quantiles``: a list of at most 16 probabilities, e.g. ``[0.025, 0.5, 0.975]`` -- the percentile band across the members
    for every row of the table, what the reference's ensemble caller makes of its runs (Development/2016/MCMC.ipynb,
    get_uncertainty_intervals: ``param_only.T.describe(percentiles=[0.025, 0.5, 0.975])``), selected exactly on the device
    (``simplyp_quantiles``) so that the table need not leave it.  The result gains ``'quantiles'`` = dict(q,
    data[K, n_cols, D or n_periods, n_reaches], lower, upper, n_members, info): ``lower`` / ``upper`` are the two order
    statistics that bracket each quantile, ``data`` numpy's ``method='linear'`` value interpolated from them on the host
    (``engine.interpolate_quantiles``).  Members whose status carries ``STATUS_NONFINITE`` never take part (``STEPCAP``
    members do: their rows are finite); ``quantile_members``, a bool array [E], restricts the band further (e.g. the
    members whose NSE in ``['gof']`` exceeds a threshold); ``n_members`` is how many took part (all NaN when none did).
    Works on daily rows and with ``reduce`` (bands of annual sums); with ``waterbody`` the summed series get their own band
    under ``['waterbody']['quantiles']``.  ``keep_daily=False`` together with ``quantiles`` drops the daily table exactly as
    with ``obs_dict``: no host table is allocated or streamed and ``data`` is None.  ``devices=[...]`` together with
    ``quantiles`` raises ValueError: a quantile of the whole ensemble is not a function of the member blocks' quantiles, so
    the band cannot be assembled from per-device results.

    ``time_quantiles``: a list of at most 16 probabilities -- order statistics PER MEMBER OVER TIME, what one
    ``DataFrame.quantile()`` call on the reference's frames gives for a single run: the flow-duration curve
    (``[0.05, 0.5, 0.9]`` of ``'Q_cumecs'``: Q95, Q50, Q10), annual maxima (``[1.0]`` with ``time_quantile_periods='annual'``),
    the annual 90th percentile of ``'SRP_mgl'``, the same for a season only -- selected exactly on the device
    (``simplyp_time_quantiles``) where the daily table lies.  ``time_quantile_series``: reference column names or the six
    ``df_R`` names ``Q_cumecs``, ``SS_mgl``, ``TDP_mgl``, ``PP_mgl``, ``TP_mgl``, ``SRP_mgl`` (computed on the fly; they add
    the four flux columns to the outputs as ``obs_dict`` does; a named column missing from ``outputs`` is added too);
    default: every column of ``outputs``.  ``time_quantile_periods``: None = the whole run, ``'annual'`` = calendar years,
    or an int array [D] of period indices, -1 = the day takes part in no period (a season: ``np.where(month in (6, 7, 8),
    year - year0, -1)``), the others non-decreasing.  The result gains ``'time_quantiles'`` = dict(q, series, periods,
    data[K, n_series, P, n_reaches, E], lower, upper, n_days[P], info), in member order: ``lower`` / ``upper`` the two order
    statistics that bracket each quantile, ``data`` numpy's ``method='linear'`` value
    (``engine.interpolate_time_quantiles``); a period without days is NaN; a member that went non-finite has its NaN sorted
    last.  A device reduction like ``obs_dict``: with ``keep_daily=False`` no host table is allocated or streamed.  Needs
    daily rows (``ValueError`` with ``reduce``).  Per member, so it works with ``devices=[...]`` (every block selects where
    its table lies) and per window in ``run_simply_p_ensemble_windows``.  Together with ``quantiles`` the band across the
    members of these per-member statistics -- e.g. the ensemble's uncertainty band of the flow-duration curve -- comes back
    under ``['time_quantiles']['quantiles']`` (same members as the daily band: ``quantile_members``, non-finite ones left out).

    ``predictive_series``: a list of 1 to 32 names -- columns of the table or the six ``df_R`` names ``Q_cumecs`` ... ``SRP_mgl``
    (``abi.TQ_DERIVED_SERIES``, what ``obs_dict`` holds observations of) -- whose bands ACROSS THE MEMBERS are selected on the
    device for every day and reach (``simplyp_predictive_bands``): the two frames of the reference's
    ``get_uncertainty_intervals`` (Development/2016/MCMC.ipynb).  Needs ``quantiles`` (the probabilities) and takes
    ``quantile_members`` as given; non-finite members are left out as for ``quantiles``; the flux columns and named columns
    missing from ``outputs`` are added.  ``predictive_m``: the error model's ``m`` of ``sigma = m * sim`` -- None (no overall
    band), a float, an array [E], or a dict name -> float or array [E] (a series the dict does not name gets 0); finite and
    >= 0 (``ValueError``).  With it every member's series has ``norm(0, m * sim)`` added before the percentiles are taken,
    drawn on the device as a pure function of (``predictive_seed``, member, ``predictive_day0`` + day, reach, series):
    ``simplyp_amd.predictive`` restates the stream, ``Engine.predictive_series`` returns the realisations themselves.  The
    result gains ``'predictive'`` = dict(q, series, param_only = dict(data[K, n_series, D, n_reaches], lower, upper), overall =
    the same or None without ``predictive_m``, n_members, seed, day0, info); ``visualise_results.band_coverage`` takes
    ``overall``.  A device reduction: ``keep_daily=False`` behaves as for ``quantiles``.  ``ValueError`` with ``reduce``, with
    ``devices=[...]`` (same reason as ``quantiles``) and for unknown names.  ``run_simply_p_ensemble_windows`` passes each
    window its ``day0 = predictive_day0 + lo``, so the windows' bands laid end to end are the single call's, bit for bit.

    ``quantile_weights`` / ``quantile_log_weights``: one value per member -- non-negative finite linear weights, or log weights
    such as the per-member log-likelihood ``['gof']`` gives (GLUE: weight the members by their likelihood) --, mutually exclusive.
    With either, EVERY band across the members this call returns is weighted and selected on the device
    (``simplyp_weighted_quantiles``, ``simplyp_predictive_bands_weighted``): the daily / reduced rows, the waterbody series, the
    band of the per-member ``time_quantiles``, and ``predictive_series`` parameter-only and overall.  The weights become the
    particle filter's integers -- linear ones through ``weighted.linear_weights`` on the host, log weights through
    ``Engine.pf_weights`` on the device (``particle.weights`` restates it) -- and the band is numpy's ``method='inverted_cdf'``
    with ``weights=``, exactly: for probability ``p`` the value of the first member, in sorted order, whose running weight reaches
    ``max(1, ceil(p T))`` (``simplyp_amd.weighted``).  One value per probability, so ``lower``, ``upper`` and ``data`` are the same
    array; every such result keeps its shape and gains ``rule='inverted_cdf'`` and ``weight_total`` = ``T``.  Non-finite members
    and ``quantile_members`` are left out as without weights; a member of weight 0 takes no part.  ``ValueError`` for a wrong
    shape, negative or non-finite linear weights, weights that are all zero, weights without ``quantiles``, and ``devices=[...]``.

    ``score=True``: the forecast is judged against the observations of ``obs_dict`` on the device (``simplyp_predictive_scores``;
    ``simplyp_amd.score`` states the rule): the continuous ranked probability score in its two terms and the counts of the
    probability integral transform, for every observed (series, day, reach).  The scored series are the ``df_R`` names of
    ``predictive_series`` that have an observation at some output reach -- without ``predictive_series``, every ``df_R`` series
    that has one.  ``quantiles`` is not needed; ``quantile_members``, ``quantile_weights`` / ``quantile_log_weights``,
    ``predictive_m``, ``predictive_seed`` and ``predictive_day0`` mean what they mean for the bands, and non-finite members are
    left out in the same way, so the scores and the (weighted) bands describe one distribution.  The result gains
    ``['scores']`` = dict(series, reaches, param_only, overall, weight_total, n_members, seed, day0, info) with ``param_only``
    = dict(crps, abs_err, spread, below, at_or_below, pit -- each [n_series, D, n_reaches], NaN (counts 0) where nothing was
    observed --, n_obs, mean_crps [n_series, n_reaches]: the NaN-skipping mean over the days) and ``overall`` the same with the
    error model drawn (``predictive_m``), else None; ``score.pit_histogram(below, at_or_below, weight_total, n_bins,
    observed=~np.isnan(crps))`` turns the counts of the observed rows into a rank histogram.  Only the
    observed rows are generated and sorted.  A device reduction: ``keep_daily=False`` behaves as for ``quantiles``.
    ``ValueError`` without ``obs_dict``, with ``reduce`` and with ``devices=[...]``, before any device call.
    ``run_simply_p_ensemble_windows`` passes each window its ``day0``: the windows' scores laid end to end are the single
    call's, bit for bit.

    ``pareto=[...]``: the members are compared on several goodness-of-fit criteria at once, on the device and before the table
    goes to the host (``simplyp_pareto``; ``simplyp_amd.pareto`` states the rule).  Each objective is ``(stat, variable)``,
    ``(stat, variable, reach_index)`` or ``(stat, variable, reach_index, sense)`` over ``abi.GOF_STATS`` (or ``'spearman'`` with
    ``spearman=True``) and ``abi.GOF_VARS``, at most 8; NSE, log NSE, r2 and Spearman's r are maximised, nRMSD (%) is minimised,
    Bias (%) is minimised in absolute value, and the other rows need an explicit sense (``pareto.resolve_objectives``).  The
    result gains ``['pareto']`` = dict(rank, dominated_by, dominates -- int32 [E]: the non-dominated rank NSGA-II sorts by (0 =
    the Pareto front), the members that dominate each one and the members it dominates --, front = the member ids of rank 0,
    objectives, sense, n_members, n_fronts, info).  Non-finite members, members outside ``quantile_members`` and members with a
    NaN objective take no part and get -1; ``pareto_max_fronts=F`` resolves the ranks below F only (deeper members get -2, their
    counts stay exact) -- a totally ordered ensemble has E fronts and one host round trip each.  ``sp.pareto_ranks(res['gof'],
    ...)`` gives the same from a table already returned.  ``ValueError`` without ``obs_dict`` and with ``devices=[...]``.

    ``forcing_error``: forcing uncertainty -- every member gets rainfall, PET and air temperature of its own, drawn on the device
    from the shared sets as part of the run (``simplyp_amd.forcing`` states the error model; nothing per member crosses PCIe)::

        forcing_error={'P':     {'sigma': 0.3, 'groups': 'day' | 'month' | 'year' | int_array[D], 'scale': float | [E]},
                       'PET':   {'sigma': 0.1, 'groups': ..., 'scale': ...},
                       'T_air': {'sigma': 0.5, 'groups': ..., 'offset': float | [E]}}      # T_air needs snow_in_kernel=True

    ``sigma`` (in [0, 2]): the standard deviation of a mean-one lognormal multiplier of P and PET, of an additive normal error of
    T_air; the days of one group share one draw per member (``'day'``, the default: daily errors; ``'month'`` / ``'year'``: one per
    calendar month / year; an int array of ids in [0, 2^31): storm events, seasons, or a single id for one constant multiplier
    per member).  ``scale`` / ``offset``: a delta-change ensemble -- each member's precipitation factor and temperature offset.
    With several forcing sets each member's own set is perturbed.  A draw is a pure function of (``forcing_seed``, member, group
    id, row): ``devices=[...]`` and ``run_simply_p_ensemble_windows`` give the single call's tables bit for bit.  The table of
    the members' sets, [E, 2 or 3, D] fp64, lives on the device beside the output table for the length of the call
    (``ValueError`` naming its size when it does not fit).  ``ValueError`` before any device call for an unknown key, a ``sigma``
    outside [0, 2], an array of the wrong length, group ids outside [0, 2^31) and ``'T_air'`` without the in-kernel snow module.
    ``'rho'`` (in [0, 0.999], needs ``sigma > 0``): autocorrelated errors -- the lag-one correlation of a row's normal between
    consecutive groups along the days (AR(1), stationary at the start; ``simplyp_amd.forcing`` defines it).  The noise state
    ``[6, E]`` (``abi.FORCING_NOISE_ROWS``) then travels with the model state: with ``return_state`` the result's ``'state'``
    gains ``'forcing_noise'`` (delivered as ``data`` is; per block under ``devices=[...]`` with ``'device'``), and an
    ``initial_state`` dict that carries it continues the noise -- a dict without it, or a bare array, is a stationary start --, so
    windows laid end to end still give the one call's tables bit for bit, wherever they cut a month.  Without a ``rho`` no key is
    added.  ``'scale_groups'`` (``'offset_groups'`` of T_air) = ``'month_of_year'`` | int array [D] of ids in [0, G), G <= 4096:
    seasonal change factors -- ``scale`` / ``offset`` is then [G, E] or [G], one entry per shift group (12 calendar months:
    wetter winters, drier summers); the rows share one array of shift groups.
    ``'PET': {'model': 'thornthwaite', 'latitude': 57.1, ...}`` (needs ``snow_in_kernel=True``): every member's PET is derived on
    the device from that member's own final air temperature -- base + offset + error -- by Thornthwaite's 1948 rule as the
    reference's ``daily_PET`` has it (``simplyp_amd.forcing.thornthwaite_rows``), so a warmer member also evaporates more; the
    met data's PET column is not read, and ``sigma`` / ``groups`` / ``rho`` / ``scale`` / ``scale_groups`` of the PET entry
    multiply the derived PET as they multiply the column otherwise.  The record must cover whole calendar years, at most 64
    (``ValueError``, as for a latitude outside [-90, 90]); a year whose monthly mean temperatures are all <= 0 gives NaN, as in
    the reference, and that member the non-finite status.  Not offered in ``run_simply_p_ensemble_windows`` and ``assimilate``
    (``ValueError``): the daily interpolation crosses year boundaries.

    ``return_state=True``: the result gains ``'state'`` = dict(rows (``abi.STATE_ROWS``), reaches (all sub-catchments),
    data[S, 16, E], end = ``met_df.index[-1]``): the model state after the last day, in member order (numpy, or a device
    tensor with ``to_host=False``; ``return_state='device'`` keeps it on the device whatever ``to_host`` says -- with
    ``devices=[...]`` as the list of the blocks' tensors, split as ``stats['bounds']``).  ``initial_state`` takes that dict,
    or a bare array [S, 16, E]: every (member, reach) then starts from it instead of the reference's cold initial conditions
    (model.py:377-459), and a run of D1 days followed by a run of the next D2 days started from its state gives the same
    tables, status bits (OR over the pieces) and right-hand-side counts as the run of D1 + D2 days, bit for bit -- whatever
    solver, lane layout, kernel path or member order either piece uses.  Given the dict, ``met_df`` must start on the day after ``end`` and the reaches must
    match (``ValueError``, before any device call); a bare array skips the date check.  A member flagged non-finite
    carries the NaN in its state and stays flagged.  ``run_simply_p_ensemble_windows`` threads the state through
    consecutive time windows of one ensemble.

    Returns ``dict(columns, reaches, data[n_cols, D or n_periods, n_reaches, E], status[E], stats)``; ``data``
    and ``status`` are numpy arrays, or device tensors when ``to_host`` is False.
    The caller's ``p_LU``/``p_SC`` are edited in place exactly as by ``run_simply_p``.
    """
    rq = _request(**locals())
    with marshal.reference_edits(p_SU, p_LU, p_SC, p):
        _bind_members(rq)
        _bind_outputs(rq)
        return _assemble(rq, _run_blocks(rq))


def _mean_crps(crps):
    """(n_obs, mean_crps) [n_series, n_reaches] of crps [n_series, D, n_reaches]: the NaN-skipping mean over the days."""
    n_obs = (~np.isnan(crps)).sum(axis=1)
    with np.errstate(invalid='ignore', divide='ignore'):
        return n_obs, np.where(n_obs > 0, np.nansum(crps, axis=1) / n_obs, np.nan)


def _scores_result(series, reaches, obs, D, got, seed, day0):
    """``res['scores']`` from the two ``Engine.predictive_scores`` results (parameter-only, overall or None); ``got`` None: no
    series has an observation."""

    def one(sums, counts, info):
        sums, counts = sums.cpu().numpy(), counts.cpu().numpy()
        T = int(info['T'])
        seen = ~np.isnan(obs)                                    # the scored rows
        pit = np.full(sums[0].shape, np.nan)
        if T > 0 and T < 1 << 52:                                # (L + M) and 2 T are exact in fp64: one rounding
            pit[seen] = (counts[0][seen] + counts[1][seen]).astype(np.float64) / float(2 * T)
        elif T > 0:
            pit[seen] = score_rules.pit(counts[0][seen], counts[1][seen], T)
        crps = sums[0] - sums[1]
        n_obs, mean_crps = _mean_crps(crps)
        return dict(crps=crps, abs_err=sums[0], spread=sums[1], below=counts[0].astype(np.uint64), at_or_below=counts[1].astype(np.uint64),
                    pit=pit, n_obs=n_obs, mean_crps=mean_crps), info
    if got is None:
        empty = lambda dt: np.zeros((0, D, len(reaches)), dtype=dt)
        po = dict(crps=empty(np.float64), abs_err=empty(np.float64), spread=empty(np.float64), below=empty(np.uint64),
                  at_or_below=empty(np.uint64), pit=empty(np.float64), n_obs=np.zeros((0, len(reaches)), dtype=np.int64),
                  mean_crps=np.zeros((0, len(reaches))))
        return dict(series=[], reaches=list(reaches), param_only=po, overall=None, weight_total=0, n_members=0, seed=seed, day0=day0,
                    info=dict(param_only=None, overall=None))
    po, po_info = one(*got[0])
    ov, ov_info = (None, None) if got[1] is None else one(*got[1])
    return dict(series=list(series), reaches=list(reaches), param_only=po, overall=ov, weight_total=int(po_info['T']),
                n_members=int(po_info['n_used']), seed=seed, day0=day0, info=dict(param_only=po_info, overall=ov_info))


def _torch_cat(xs):
    import torch
    return torch.cat([x.to(xs[0].device) for x in xs], dim=-1)


def run_simply_p_ensemble_windows(met_df, p_struc, p_SU, p_LU, p_SC, p, dynamic_options, window='annual', initial_state=None,
                                  **kwargs):
    """One ensemble run cut into consecutive time windows: a generator of ``run_simply_p_ensemble`` results, one per window.

    Same arguments as ``run_simply_p_ensemble`` plus ``window`` (``'annual'`` = calendar years, an int = that many days, or
    a list of start dates: ``ensemble.window_bounds``).  The model state is threaded from window to window on the device
    (``simplyp_set_state``), so the windows' tables laid end to end ARE the table of the single call, bit for bit, and so
    are the summed ``rhs_evals`` / ``steps`` / ``rejected``; a window's table exists only while the caller holds its item, so
    the peak device and host footprint is one window's: the daily series, per-year goodness of fit or percentile bands of
    an ensemble whose whole table would not fit anywhere.  ``obs_dict`` / ``waterbody`` / ``quantiles`` / ``time_quantiles`` / ``predictive_series`` apply per window
    (an array ``time_quantile_periods`` covers the whole run and is cut with the days).
    With ``reduce``, window boundaries must fall on period boundaries (``ValueError``).

    Each item also carries ``'window'`` = (first day, last day, lo, hi) and ``'state'`` (on the device; the last item's is
    where a later run continues).  ``status`` is per window: the status of the whole run is the OR over the items (a
    member that went non-finite carries the NaN in its state and is flagged in every later window too).  Bad arguments
    raise when the generator is created, not at its first item."""
    met_sets = list(met_df) if isinstance(met_df, (list, tuple)) else [met_df]
    index = met_sets[0].index
    reduce = kwargs.get('reduce')
    bounds = ensemble.window_bounds(index, window, reduce=reduce)
    if 'return_state' in kwargs:
        raise ValueError("run_simply_p_ensemble_windows always returns the state (on the device)")
    if kwargs.get('forcing_error') is not None:
        forcing_rules.refuse_pet_model(kwargs['forcing_error'], 'run_simply_p_ensemble_windows')
        forcing_rules.cut_group_arrays(kwargs['forcing_error'], len(index), 0, len(index))

    def gen():
        state = initial_state
        for lo, hi in bounds:
            kw = dict(kwargs)
            if reduce is not None and not isinstance(reduce, str):
                part = np.asarray(reduce)[lo:hi]
                kw['reduce'] = part - part.min()
            tqp = kw.get('time_quantile_periods')
            if tqp is not None and not isinstance(tqp, str):         # the window's days, its periods numbered from 0
                part = np.asarray(tqp)[lo:hi]
                kw['time_quantile_periods'] = np.where(part >= 0, part - (part[part >= 0].min() if (part >= 0).any() else 0), -1)
            if kw.get('predictive_series') is not None or kw.get('score'):     # the stream is indexed by the run's day, not the window's
                kw['predictive_day0'] = int(kwargs.get('predictive_day0', 0)) + lo
            if kw.get('forcing_error') is not None:                  # group arrays cover the whole run; calendar ids are absolute anyway
                kw['forcing_error'] = forcing_rules.cut_group_arrays(kw['forcing_error'], len(index), lo, hi)
            mets = [m.iloc[lo:hi] for m in met_sets]
            res = run_simply_p_ensemble(mets if isinstance(met_df, (list, tuple)) else mets[0], p_struc, p_SU, p_LU, p_SC, p,
                                        dynamic_options, initial_state=state, return_state='device', **kw)
            state = res['state']
            res['window'] = (index[lo], index[hi - 1], lo, hi)
            yield res
            del res
    return gen()
