"""ctypes mirror of include/simplyp.h (structs, enums, default options)."""

import ctypes as C

ABI_VERSION = 18

INTEG_RK4 = 0
INTEG_CASHKARP = 1
INTEG_CASHKARP_AUG = 2
INTEG_CASHKARP_AUG_F32 = 3
INTEGRATORS = {'rk4': INTEG_RK4, 'cashkarp': INTEG_CASHKARP, 'ck45': INTEG_CASHKARP,
               'cashkarp_aug': INTEG_CASHKARP_AUG, 'cashkarp_aug_f32': INTEG_CASHKARP_AUG_F32}

# SIMPLYP_STATE_*: rows of the model state [S, N_STATE, E] (simplyp_set_state), in the header's order
STATE_ROWS = ['VsA', 'VsS', 'Vg', 'Vr', 'Qr', 'Msus', 'TDPr', 'PPr', 'Plab_A', 'TDPs_A', 'Plab_NC', 'TDPs_NC',
              'conc_TDPs_A', 'conc_TDPs_NC', 'h_next', 'D_snow']
N_STATE = len(STATE_ROWS)

FORCING_STREAM = 0x464F5243                  # SIMPLYP_FORCING_STREAM ("FORC"): the fourth counter word of a forcing draw
FORCING_ROWS = ['P', 'PET', 'T_air']         # rows of a forcing set ('P' is Precipitation with the in-kernel snow module)
# rows of the forcing noise state [6, E] (simplyp_opts.forcing_noise_in / _out): z of each row, then each row's last group id
# as an exact float64 (-1.0: none)
FORCING_NOISE_ROWS = ['z_P', 'z_PET', 'z_T_air', 'group_P', 'group_PET', 'group_T_air']
FORCING_RHO_MAX, FORCING_SHIFT_GROUPS_MAX = 0.999, 4096
FORCING_PET_MODELS = {'thornthwaite': 1}     # simplyp_opts.forcing_pet_model
FORCING_PET_YEARS_MAX = 64                   # SIMPLYP_FORCING_PET_YEARS_MAX


def forcing_pet_plan_bytes(D):
    """SIMPLYP_FORCING_PET_PLAN_BYTES: the plan behind the forcing table, daylight[M], month[2][M], day[3][D], M = 12 (D // 365)."""
    return 16 * 12 * (D // 365) + 12 * D

STATUS_NONFINITE = 1
STATUS_STEPCAP = 2


# The C types of the header's prototypes as ctypes (engine.prototypes reads the header with them).  A pointer to one of the structs
# below is POINTER(its class) -- each class names its struct in ``c_name``, the one place the pairing is written -- and every other
# pointer (data, simplyp_ctx*, simplyp_ctx**, void*) is a c_void_p.
C_SCALARS = {'int': C.c_int, 'int32_t': C.c_int32, 'uint32_t': C.c_uint32, 'int64_t': C.c_int64, 'uint64_t': C.c_uint64,
             'double': C.c_double}
C_RETURNS = dict(C_SCALARS, **{'const char*': C.c_char_p, 'void*': C.c_void_p, 'void': None})


def structs():
    """{C name: class} of the mirrors in this module."""
    return {cls.c_name: cls for cls in globals().values()
            if isinstance(cls, type) and issubclass(cls, C.Structure) and 'c_name' in vars(cls)}


class Dims(C.Structure):
    c_name = 'simplyp_dims'
    _fields_ = [('E', C.c_int32), ('S', C.c_int32), ('D', C.c_int32), ('n_forcing_sets', C.c_int32)]


class Opts(C.Structure):
    c_name = 'simplyp_opts'
    _fields_ = [('integrator', C.c_int32), ('substeps', C.c_int32),
                ('rtol', C.c_double), ('atol', C.c_double),
                ('max_steps', C.c_int32), ('dynamic_epc0', C.c_int32), ('dynamic_erod', C.c_int32),
                ('run_mode_cal', C.c_int32), ('sc_qr0', C.c_int32), ('out_mask', C.c_uint32),
                ('step_len', C.c_double), ('project_vr', C.c_int32), ('balance', C.c_int32),
                ('balance_pilot_days', C.c_int32), ('out_slot_order', C.c_int32),
                ('time_chunk_days', C.c_int32), ('n_periods', C.c_int32), ('snow', C.c_int32), ('lanes_per_wave', C.c_int32),
                ('lanes_per_member', C.c_int32), ('stiff_pair', C.c_int32),
                # forcing uncertainty (all zero = off); Engine.run(forcing_error=) fills them on a copy of the caller's options
                ('forcing_error', C.c_int32), ('forcing_member0', C.c_uint32), ('forcing_seed', C.c_uint64),
                ('forcing_sigma', C.c_double * 3), ('forcing_group_of_day', C.c_void_p * 3), ('forcing_shift', C.c_void_p),
                ('forcing_shift_rows', C.c_int32), ('forcing_pet_model', C.c_int32), ('forcing_table', C.c_void_p),
                # autocorrelated errors and seasonal change factors (all zero = off)
                ('forcing_rho', C.c_double * 3), ('forcing_noise_in', C.c_void_p), ('forcing_noise_out', C.c_void_p),
                ('forcing_shift_group_of_day', C.c_void_p), ('forcing_shift_groups', C.c_int32), ('forcing_reserved2', C.c_int32)]

    def copy(self):
        o = Opts()
        C.memmove(C.byref(o), C.byref(self), C.sizeof(Opts))
        return o


class _Info(C.Structure):
    """What the library reports of a call: a struct of include/simplyp.h read back as a dict (reserved fields left out)."""

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith('reserved')}


class Stats(_Info):
    c_name = 'simplyp_stats'
    _fields_ = [('rhs_evals', C.c_uint64), ('steps', C.c_uint64), ('rejected', C.c_uint64),
                ('kernel_ms', C.c_double), ('pilot_ms', C.c_double), ('simt_efficiency', C.c_double), ('n_launches', C.c_int32), ('balanced', C.c_int32),
                ('queued', C.c_int32), ('lanes_per_wave', C.c_int32), ('lanes_per_member', C.c_int32), ('streamed_chunks', C.c_int32),
                ('d2h_tail_ms', C.c_double), ('wall_ms', C.c_double), ('stream_gbs', C.c_double),
                ('queue_waits', C.c_uint64), ('queue_longest_wait_polls', C.c_uint32), ('pack_overflow_blocks', C.c_uint32), ('queue_longest_stall_polls', C.c_uint64),
                ('stiff_pair', C.c_int32), ('packed_records', C.c_int32)]


class GofInfo(_Info):
    c_name = 'simplyp_gof_info'
    _fields_ = [('kernel_ms', C.c_double), ('bytes_read', C.c_int64), ('n_q_days', C.c_int32), ('n_chem_days', C.c_int32),
                ('n_chunks_q', C.c_int32), ('n_chunks_chem', C.c_int32)]


class WbInfo(_Info):
    c_name = 'simplyp_wb_info'
    _fields_ = [('kernel_ms', C.c_double), ('bytes_moved', C.c_int64)]


class QuantileInfo(_Info):
    c_name = 'simplyp_quantile_info'
    _fields_ = [('kernel_ms', C.c_double), ('bytes_table', C.c_int64), ('n_used', C.c_int32), ('n_passes', C.c_int32)]


class WqInfo(_Info):
    c_name = 'simplyp_wq_info'
    _fields_ = [('kernel_ms', C.c_double), ('bytes_table', C.c_int64), ('T', C.c_uint64), ('n_used', C.c_int32), ('n_passes', C.c_int32)]


class ScoreInfo(_Info):
    c_name = 'simplyp_score_info'
    _fields_ = [('kernel_ms', C.c_double), ('gen_ms', C.c_double), ('sort_ms', C.c_double), ('bytes_read', C.c_int64),
                ('bytes_workspace', C.c_int64), ('T', C.c_uint64), ('n_used', C.c_int32), ('n_rows_scored', C.c_int32),
                ('n_chunks', C.c_int32), ('reserved', C.c_int32)]


SCORE_TILE = 4096               # (key, weight) pairs the scores' LDS sort takes at once (simplyp_score.h)


class ParetoInfo(_Info):
    c_name = 'simplyp_pareto_info'
    _fields_ = [('kernel_ms', C.c_double), ('pair_tests', C.c_int64), ('n_used', C.c_int32), ('n_fronts', C.c_int32),
                ('n_front0', C.c_int32), ('n_unranked', C.c_int32)]


PARETO_MAX_OBJ = 8              # objectives per call (SIMPLYP_PARETO_MAX_OBJ)
PARETO_EXCLUDED = -1            # every output of a member that takes no part
PARETO_UNRANKED = -2            # the rank of a participant deeper than max_fronts
PARETO_THREADS = 256            # members per workgroup of the all-pairs kernel (simplyp_pareto.hip.h)
PARETO_JTILE = 512              # the other side of the pairs: keys staged in LDS at a time
PARETO_JSPLIT = 2048            # and the stretch of them one workgroup takes; the grid's second axis splits the rest


class TqInfo(_Info):
    c_name = 'simplyp_tq_info'
    _fields_ = [('kernel_ms', C.c_double), ('bytes_read', C.c_int64), ('n_sweeps', C.c_int32), ('n_periods', C.c_int32)]


class PredInfo(_Info):
    c_name = 'simplyp_pred_info'
    _fields_ = [('kernel_ms', C.c_double), ('gen_ms', C.c_double), ('bytes_read', C.c_int64), ('bytes_workspace', C.c_int64),
                ('n_used', C.c_int32), ('n_passes', C.c_int32), ('n_chunks', C.c_int32), ('reserved', C.c_int32)]


class McmcInfo(_Info):
    c_name = 'simplyp_mcmc_info'
    _fields_ = [('kernel_ms', C.c_double), ('n_inside', C.c_int32), ('n_accepted', C.c_int32), ('n_nan', C.c_int32),
                ('reserved', C.c_int32)]


MCMC_TARGET_F_TDP = -1          # simplyp_mcmc_propose: the dimension goes to f_tdp
MCMC_TARGET_NONE = -2           # ... nowhere: an error-model m


class NmInfo(_Info):
    c_name = 'simplyp_nm_info'
    _fields_ = [('kernel_ms', C.c_double), ('n_active', C.c_int32), ('n_converged', C.c_int32), ('n_shrinking', C.c_int32),
                ('n_nonfinite_start', C.c_int32), ('n_inside', C.c_int32), ('reserved', C.c_int32)]


class SobolInfo(_Info):
    c_name = 'simplyp_sobol_info'
    _fields_ = [('kernel_ms', C.c_double), ('counts_ms', C.c_double), ('contract_ms', C.c_double), ('flops', C.c_int64),
                ('bytes_workspace', C.c_int64), ('n_valid', C.c_int32), ('n_resamples', C.c_int32)]


class PfInfo(_Info):
    c_name = 'simplyp_pf_info'
    _fields_ = [('kernel_ms', C.c_double), ('lw_max', C.c_double), ('sum_w', C.c_double), ('sum_w2', C.c_double),
                ('T', C.c_uint64), ('n_alive', C.c_int32), ('n_nan', C.c_int32), ('n_unique', C.c_int32), ('n_bad', C.c_int32),
                ('n_outside', C.c_int32), ('reserved', C.c_int32)]

PF_MAX_LOG2_E = 22              # the particle filter's entries take 1 <= E <= 2^22
PF_WEIGHT_BITS = 40             # ... and resolve normalised weights to 2^-40


# SIMPLYP_NM_*: the rows of istate [NM_N_ISTATE, S] (simplyp_amd.neldermead names the phases and the status values)
NM_ISTATE = ['phase', 'cursor', 'n_iter', 'status', 'n_reflect', 'n_expand', 'n_contract_out', 'n_contract_in', 'n_shrink']
NM_N_ISTATE = len(NM_ISTATE)

TQ_DERIVED = 64                                                                       # SIMPLYP_TQ_DERIVED
TQ_DERIVED_SERIES = ['Q_cumecs', 'SS_mgl', 'TDP_mgl', 'PP_mgl', 'TP_mgl', 'SRP_mgl']  # df_R names, in SIMPLYP_GOF_* order

# SIMPLYP_WB_*: the reference's df_summed columns in its order (model.py:866, :886-888, :842-845)
WB_COLUMNS = ['Q_cumecs', 'Msus_kg/day', 'TDP_kg/day', 'PP_kg/day', 'SS_mgl', 'TDP_mgl', 'PP_mgl',
              'TP_mgl', 'TP_kg/day', 'SRP_mgl', 'SRP_kg/day']
WB_MASK_ALL = (1 << len(WB_COLUMNS)) - 1

GOF_VARS = ['Q', 'SS', 'TDP', 'PP', 'TP', 'SRP']                                      # SIMPLYP_GOF_*
GOF_STATS = ['N obs', 'NSE', 'log NSE', 'r2', 'Bias (%)', 'nRMSD (%)', 'sum_log_sim', 'sum_relsq']   # SIMPLYP_GOFSTAT_*
LAG_STATS = ['n_link', 'sq_head', 'sq_tail', 'cross']                                 # SIMPLYP_LAGSTAT_* (simplyp_gof_lag)


# Solver settings used when the caller does not choose: Cash-Karp 5(4) with per-thread step
# control on the augmented (transcendental-free) form of the system, at the tolerance that meets
# the <= 1e-6 parity bar against odeint(rtol=atol=1e-12) on every member of a 100 000-member Monte-Carlo
# ensemble with a margin (1e-8 before the step controller learned about the knees
# of the gates, round 2).
DEFAULT_SOLVER = dict(integrator='cashkarp_aug', substeps=8, rtol=1e-7, atol=1e-12, max_steps=4000, project_vr=1,
                      balance=2, balance_pilot_days=0, out_slot_order=0, time_chunk_days=0, lanes_per_wave=0, lanes_per_member=0,
                      stiff_pair=0)


def make_opts(solver=None, dynamic_epc0=False, dynamic_erod=False, run_mode_cal=True, sc_qr0=0,
              out_mask=(1 << 25) - 1, step_len=1.0, n_periods=0, snow=False):
    s = dict(DEFAULT_SOLVER)
    s.update(solver or {})
    integ = s['integrator']
    if isinstance(integ, str):
        integ = INTEGRATORS[integ.lower()]
    o = Opts()
    o.integrator = int(integ)
    o.substeps = int(s['substeps'])
    o.rtol = float(s['rtol'])
    o.atol = float(s['atol'])
    o.max_steps = int(s['max_steps'])
    o.project_vr = int(s['project_vr'])
    o.balance = int(s['balance'])
    o.balance_pilot_days = int(s['balance_pilot_days'])
    o.out_slot_order = int(s['out_slot_order'])
    o.time_chunk_days = int(s['time_chunk_days'])
    o.lanes_per_wave = int(s['lanes_per_wave'])
    o.lanes_per_member = int(s['lanes_per_member'])
    o.stiff_pair = int(s['stiff_pair'])
    o.dynamic_epc0 = int(bool(dynamic_epc0))
    o.dynamic_erod = int(bool(dynamic_erod))
    o.run_mode_cal = int(bool(run_mode_cal))
    o.sc_qr0 = int(sc_qr0)
    o.out_mask = int(out_mask)
    o.step_len = float(step_len)
    o.n_periods = int(n_periods)
    o.snow = 1 if snow else 0
    return o
