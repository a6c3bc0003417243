/*
 * simplyp.h -- C ABI of the MI355X SimplyP time-stepping engine (libsimplyp_hip.so).
 *
 * The reference (JoeyYHT/SimplyP, pure Python) has no FFI.  Its seam for this path is the
 * double loop inside run_simply_p() -- `for SC in p['SC_list']` (model.py:365) x
 * `for idx in range(len(met_df))` (model.py:491) around `odeint(ode_f, ...)` (model.py:640).
 * Every entry point below replaces a piece of that loop nest; the Python host in
 * simplyp_amd/ binds them with ctypes (see INTEGRATION.md for the stub).
 *
 * Conventions
 *   - plain C, no torch / HIP types in signatures; all pointers marked "device" are
 *     device-resident (hipMalloc'd, e.g. torch CUDA tensors' data_ptr()), "host" are host.
 *   - ensemble-major SoA: the member index e is always the fastest-varying one.
 *   - every function returns 0 (SIMPLYP_OK) or a negative simplyp_status; no exceptions
 *     cross the boundary; simplyp_last_error() gives the message for the last failure.
 *   - the caller owns every buffer; the library keeps no pointer after a call returns.
 */
#ifndef SIMPLYP_H
#define SIMPLYP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 17 still with simplyp_state_bytes / simplyp_set_state and the SIMPLYP_STATE_* rows: they are purely additive -- no
 * signature and no struct layout of version 17 changed, a caller built against the earlier header runs unchanged.
 * 17 still with the packed output stream, for the same reason: simplyp_fetch_packed and simplyp_pack_roundtrip_host are new
 * entry points, and simplyp_stats keeps its size and every offset -- reserved0 (always 0 before) is now packed_records, and
 * the upper half of queue_longest_wait_polls (a 32-bit count on the device: always 0 before) is now pack_overflow_blocks.
 * 17 still with simplyp_fetch_packed_pred and simplyp_pack_roundtrip_host_pred: two more entry points, nothing else.
 * 17 still with simplyp_time_quantiles, simplyp_tq_info and SIMPLYP_TQ_DERIVED: one more entry point with its own info struct.
 * 17 still with simplyp_predictive_series, simplyp_predictive_bands and simplyp_pred_info: two more entry points, one more info
 * struct; no existing struct, enum or entry point changes.
 * 17 still with simplyp_mcmc_propose, simplyp_mcmc_log_prob, simplyp_mcmc_accept and simplyp_mcmc_info: three more entry points, one
 * more info struct, purely additive again.
 * 17 still with simplyp_nm_propose, simplyp_nm_update, simplyp_nm_info and the SIMPLYP_NM_* constants: two more entry points, one
 * more info struct, nothing existing changes.
 * 17 still with simplyp_sobol_design, simplyp_sobol_indices and simplyp_sobol_info: two more entry points, one more info struct,
 * additive once more.
 * 17 still with simplyp_pf_loglik, simplyp_pf_weights, simplyp_pf_resample, simplyp_gather_members, simplyp_pf_jitter and
 * simplyp_pf_info: five more entry points, one more info struct, nothing existing changes.
 * 17 still with simplyp_weighted_quantiles, simplyp_predictive_bands_weighted and simplyp_wq_info: two more entry points, one more
 * info struct; the unweighted entries and everything they return are untouched.
 * 17 still with simplyp_scores, simplyp_predictive_scores and simplyp_score_info: two more entry points, one more info struct; the
 * ABI is only extended, no existing struct, enum or entry point changes.
 * 17 still with simplyp_pareto and simplyp_pareto_info: one more entry point, one more info struct, three constants; nothing
 * existing changes.
 * 17 still with autocorrelated forcing errors and seasonal change factors: forcing_rho, forcing_noise_in / _out,
 * forcing_shift_group_of_day and forcing_shift_groups are appended to simplyp_opts after forcing_table (all zero = off), as the
 * forcing_* fields before them were; no entry point is added and none changes.
 * 18 still with Thornthwaite PET from each member's air temperature: forcing_reserved (always 0 before) is now forcing_pet_model,
 * and its plan stands behind the table in the forcing_table workspace; simplyp_opts keeps its size and every offset.
 * 18: simplyp_order_members, the members' lane-slot order of a balanced run from a caller-given cost table; nothing existing
 * changes.
 * 18 still with simplyp_eval_units' which = 6 (the right-hand sides) and which = 7 (the step-rule pieces): adding values of
 * `which` is purely additive -- the values before keep their rows, and what was refused as unknown (8 and above) still is. */
#define SIMPLYP_ABI_VERSION 18

typedef enum {
    SIMPLYP_OK = 0,
    SIMPLYP_ERR_ARG = -1,        /* bad dimension / option / NULL pointer            */
    SIMPLYP_ERR_TOPOLOGY = -2,   /* upstream id >= own id, out of range, ...          */
    SIMPLYP_ERR_DEVICE = -3,     /* HIP runtime error (message in simplyp_last_error) */
    SIMPLYP_ERR_NOMEM = -4
} simplyp_status;

/* ---- per-member parameters: rows of member_params[SIMPLYP_NP_M][E] --------------------
 * Raw reference parameters (sheet 'Constant' -> series p, sheet 'LU' -> frame p_LU); every
 * derived quantity (mu model.py:349, initial conditions :377-459, Kf :449-453) is computed
 * from these inside the kernel prologue, so an ensemble may perturb any of them.          */
enum {
    SIMPLYP_PM_F_QUICK = 0, SIMPLYP_PM_ALPHA, SIMPLYP_PM_FC, SIMPLYP_PM_BETA, SIMPLYP_PM_T_G,
    SIMPLYP_PM_QG_MIN, SIMPLYP_PM_A_Q, SIMPLYP_PM_B_Q, SIMPLYP_PM_QR0_INIT, SIMPLYP_PM_MSOIL_M2,
    SIMPLYP_PM_KF, SIMPLYP_PM_TDPG, SIMPLYP_PM_E_PP, SIMPLYP_PM_E_M, SIMPLYP_PM_K_M,
    SIMPLYP_PM_D_MAXE_SPR, SIMPLYP_PM_D_MAXE_AUT,
    SIMPLYP_PM_T_S_A, SIMPLYP_PM_T_S_S, SIMPLYP_PM_SOILPCONC_A, SIMPLYP_PM_SOILPCONC_S,
    SIMPLYP_PM_P_NETINPUT_A, SIMPLYP_PM_P_NETINPUT_NC, SIMPLYP_PM_EPC0_INIT_A, SIMPLYP_PM_EPC0_INIT_S,
    SIMPLYP_PM_C_COVER_A, SIMPLYP_PM_C_COVER_S, SIMPLYP_PM_C_COVER_IG,
    SIMPLYP_PM_C_MEAS_A, SIMPLYP_PM_C_MEAS_S, SIMPLYP_PM_C_MEAS_IG,
    SIMPLYP_PM_F_DDSM, SIMPLYP_PM_D_SNOW_0,   /* snow module (inputs.py:159-210); read only when opts.snow = 1 */
    SIMPLYP_NP_M
};

/* ---- per-reach parameters: rows of reach_params[SIMPLYP_NP_R][S][E] (sheet 'SC_reach') - */
enum {
    SIMPLYP_PR_A_CATCH = 0, SIMPLYP_PR_F_AR, SIMPLYP_PR_F_IG, SIMPLYP_PR_F_S,
    SIMPLYP_PR_F_NC_AR, SIMPLYP_PR_F_NC_IG, SIMPLYP_PR_F_NC_S, SIMPLYP_PR_F_SPR,
    SIMPLYP_PR_S_AR, SIMPLYP_PR_S_IG, SIMPLYP_PR_S_SN, SIMPLYP_PR_L_REACH, SIMPLYP_PR_S_REACH,
    SIMPLYP_PR_TDPEFF,
    SIMPLYP_NP_R
};

/* ---- output columns, in the reference's own order: 12 ODE results (model.py:737-739)
 * followed by 13 non-ODE results (model.py:721-723, names :743-745).                     */
enum {
    SIMPLYP_OUT_VSA = 0, SIMPLYP_OUT_VSS, SIMPLYP_OUT_VG, SIMPLYP_OUT_VR, SIMPLYP_OUT_QR_END,
    SIMPLYP_OUT_QR, SIMPLYP_OUT_MSUS_END, SIMPLYP_OUT_MSUS_FLUX, SIMPLYP_OUT_TDPR_END,
    SIMPLYP_OUT_TDP_FLUX, SIMPLYP_OUT_PPR_END, SIMPLYP_OUT_PP_FLUX,
    SIMPLYP_OUT_QQ, SIMPLYP_OUT_QSA, SIMPLYP_OUT_QSS, SIMPLYP_OUT_QG, SIMPLYP_OUT_C_COVER_A,
    SIMPLYP_OUT_EPC0_A, SIMPLYP_OUT_EPC0_NC, SIMPLYP_OUT_TDPS_A, SIMPLYP_OUT_PLAB_A,
    SIMPLYP_OUT_CONC_TDPS_A, SIMPLYP_OUT_TDPS_NC, SIMPLYP_OUT_PLAB_NC, SIMPLYP_OUT_CONC_TDPS_NC,
    SIMPLYP_N_OUT_REF,           /* = 25: the columns the reference's loop produces (model.py:644, :721-724)            */
    /* 26th column, only with opts.snow = 1: the member's snow depth at the end of the day -- met_df['D_snow_end']
     * (inputs.py:197-207), which the reference returns as df_TC['D_snow'] (model.py:775-776).  With the snow module run
     * per member inside the kernel it is a per-member series; same arithmetic and order as the host function.           */
    SIMPLYP_OUT_D_SNOW = SIMPLYP_N_OUT_REF,
    SIMPLYP_N_OUT
};
#define SIMPLYP_MASK_ALL    ((uint32_t)((1u << SIMPLYP_N_OUT_REF) - 1u))   /* the reference's 25 columns                */
#define SIMPLYP_MASK_D_SNOW ((uint32_t)(1u << SIMPLYP_OUT_D_SNOW))        /* accepted only together with opts.snow = 1 */
/* the five documented model outputs of a reach (model.py:272-277): Vr, Qr, and the three
 * daily fluxes */
#define SIMPLYP_MASK_REACH5 ((1u << SIMPLYP_OUT_VR) | (1u << SIMPLYP_OUT_QR) | (1u << SIMPLYP_OUT_MSUS_FLUX) | \
                             (1u << SIMPLYP_OUT_TDP_FLUX) | (1u << SIMPLYP_OUT_PP_FLUX))

/* ---- model state: rows of state[S][SIMPLYP_N_STATE][E] (simplyp_set_state) ----------------
 * Everything a (member, reach) carries from one day to the next, in the reference's terms: the eight carried ODE variables
 * (model.py:648-658), the soil P stores and concentrations (:696-703), the solver's trial step and the snow depth
 * (inputs.py:200, :205).  A run of D1 + D2 days and a run of D1 days followed by a run of D2 days started from the first
 * one's state give the same tables, status bits and right-hand-side counts bit for bit.  The state belongs to the model,
 * not to a kernel configuration: one written under any integrator, lane layout, member order or kernel path may be consumed
 * under any other.  Member order always, fp64, device. */
enum {
    SIMPLYP_STATE_VSA = 0,       /* VsA, soil water volume, agricultural (mm)                                          */
    SIMPLYP_STATE_VSS,           /* VsS, soil water volume, semi-natural (mm)                                          */
    SIMPLYP_STATE_VG,            /* Vg as carried: AFTER the day-end reset, Qg * T_g (:670) -- not the stored 'Vg' column */
    SIMPLYP_STATE_VR,            /* Vr, reach volume                                                                    */
    SIMPLYP_STATE_QR,            /* Qr_EndOfDay: the instantaneous flow, not the daily mean 'Qr'                        */
    SIMPLYP_STATE_MSUS,          /* Msus_EndOfDay: the reach's mass, not the daily flux (the four daily integrals start  */
    SIMPLYP_STATE_TDPR,          /* TDPr_EndOfDay   from zero every day, :618, and are no state)                         */
    SIMPLYP_STATE_PPR,           /* PPr_EndOfDay                                                                         */
    SIMPLYP_STATE_PLAB_A,        /* labile soil P, agricultural (:697)                                                  */
    SIMPLYP_STATE_TDPS_A,        /* soil-water TDP mass, agricultural (:696)                                            */
    SIMPLYP_STATE_PLAB_NC,       /* ... newly-converted land (:698-699)                                                 */
    SIMPLYP_STATE_TDPS_NC,
    SIMPLYP_STATE_CONC_TDPS_A,   /* soil-water TDP concentration used by the next day's fluxes (:702, :711)             */
    SIMPLYP_STATE_CONC_TDPS_NC,  /* (:703, :715)                                                                        */
    SIMPLYP_STATE_H_NEXT,        /* the adaptive solver's next trial step (days).  RK4: written as step_len / substeps,
                                    ignored on input                                                                    */
    SIMPLYP_STATE_D_SNOW,        /* snow depth at the end of the day; opts.snow = 0: written as 0.0, ignored on input   */
    SIMPLYP_N_STATE              /* = 16 */
};

/* per-member status bits written to member_status[E] */
#define SIMPLYP_STATUS_NONFINITE 1   /* a state became NaN/Inf                               */
#define SIMPLYP_STATUS_STEPCAP   2   /* adaptive solver hit max_steps in some day            */

typedef enum {
    SIMPLYP_INTEG_RK4 = 0,       /* classical RK4, `substeps` equal steps per day            */
    SIMPLYP_INTEG_CASHKARP = 1,  /* Cash-Karp 5(4) embedded pair, per-thread step control, on the reference's
                                    12-variable system as written (ode_f, model.py:58-187)                       */
    SIMPLYP_INTEG_CASHKARP_AUG = 2, /* same pair and step rule on the augmented form of that system: exp(-mu Vs),
                                    Qr**b_Q, Qr**k_M carried as extra states through their own exact ODEs and
                                    re-evaluated every day, Vr taken from its invariant -- no transcendental in
                                    the right-hand side.  Default.  Its step controller knows
                                    the knees of the reference's smooth-step gates (f_x, model.py:23-37: C1 only):
                                    steps are aimed at them, and the error estimate of a step that crosses one
                                    unannounced is not trusted -- parity-grade (<= 1e-6 against odeint at
                                    rtol=atol=1e-12) at rtol 1e-7.                                               */
    SIMPLYP_INTEG_CASHKARP_AUG_F32 = 3 /* scheme 2 with the stage arithmetic in fp32 (BASELINE config C5): 11 float states per
                                    member inside the day's integration; the four daily integrals, the carried state,
                                    labile soil P / soil-water TDP and the day constants stay fp64.  Meant for
                                    rtol ~ 1e-5 (rtol < 1e-6 is refused); not a parity-grade mode.                 */
} simplyp_integrator;

typedef struct {
    int32_t E;               /* ensemble members                                           */
    int32_t S;               /* sub-catchments / reaches (ids 0..S-1 = reference SC 1..S)  */
    int32_t D;               /* days                                                       */
    int32_t n_forcing_sets;  /* >= 1                                                       */
} simplyp_dims;

typedef struct {
    int32_t  integrator;     /* simplyp_integrator                                         */
    int32_t  substeps;       /* RK4: steps per day.  Cash-Karp: first trial step = step_len/substeps */
    double   rtol;           /* Cash-Karp: err_i <= atol + rtol*max(|y_i|,|y_i + h k1_i|)  (schemes 2, 3: the soil boxes
                                measured from field capacity)          */
    double   atol;
    int32_t  max_steps;      /* Cash-Karp: attempted steps per day before SIMPLYP_STATUS_STEPCAP */
    int32_t  dynamic_epc0;   /* dynamic_options['Dynamic_EPC0'] == 'y'  (model.py:600,684) */
    int32_t  dynamic_erod;   /* dynamic_options['Dynamic_erodibility'] == 'y' (model.py:555) */
    int32_t  run_mode_cal;   /* p_SU.run_mode == 'cal' -> Kf calibrated (model.py:449-453) */
    int32_t  sc_qr0;         /* zero-based reach that Qr0_init refers to (p['SC_Qr0']-1, model.py:386) */
    uint32_t out_mask;       /* bit c set -> column c (SIMPLYP_OUT_*) is written; SIMPLYP_MASK_D_SNOW needs opts.snow */
    double   step_len;       /* integration span per day, model.py:345 (default 1.0)       */
    int32_t  project_vr;     /* 1: at each day end reset Vr to the invariant of the reference's own equations,
                                L_reach*Qr^(1-b_Q)/(a_Q*86400) (drift control; 0 = integrate Vr literally) */
    int32_t  balance;        /* member load balancing: 0 off, 1 on, 2 auto (on when the ensemble needs more waves
                                than the chip holds at once, or a reach network that runs through the task queue).  Short pilot
                                runs measure each member's cost in 8 windows of the forcing; lane slots then take members in
                                blocks of decreasing total cost, ordered inside a block by cost pattern.
                                Results are unchanged bit for bit (members are independent).              */
    int32_t  balance_pilot_days;   /* total days of the pilot, split into 8 windows spread over the first ~1.6 years;
                                      0 = default (64)                                                          */
    int32_t  out_slot_order; /* 0: `out` is written in member order (when members were reordered for balance this is
                                a scatter of 8-byte words: correct, but HBM sees ~4x the output bytes as partial-sector
                                writes).  1: `out` is written in lane-slot order, fully coalesced, and the caller gets
                                the member id of every slot in `member_of_slot` (identity when no reordering happened) */
    int32_t  time_chunk_days;/* single-reach ensembles, adaptive integrators: run as (time chunk x 64-member group) tasks
                                pulled by one persistent wave per SIMD, so every SIMD stays busy whatever the members'
                                relative costs.  0 = auto (chunks of 256 days when the ensemble needs more waves than
                                the chip holds; 64 days for a single-reach run whose output is streamed to the host,
                                simplyp_stream_out), > 0 = always, with this chunk length (rounded up to a multiple of 64),
                                < 0 = never.
                                Results are unchanged bit for bit.                                              */
    int32_t  n_periods;      /* time-reduced output: 0 = one output row per day; > 0 = `out` has n_periods rows per column,
                                row p = sum over the days d with period_of_day[d] == p (e.g. calendar years) */
    int32_t  snow;           /* 0: forcing row 0 is the hydrological input P as the reference's snow_hydrol_inputs left it in
                                met_df['P'] (2 rows per set: P, PET).  1: the snow module runs inside the kernel, per member:
                                forcing has 3 rows per set -- Precipitation, PET, T_air (the met file's columns) -- and every
                                member accumulates / melts its own snow pack with its SIMPLYP_PM_F_DDSM and
                                SIMPLYP_PM_D_SNOW_0 (inputs.py:183-208), so an ensemble can perturb the snow parameters
                                without one forcing set per member.  Same arithmetic, same order: P is bit-identical
                                to the host function's.                                                          */
    int32_t  lanes_per_wave; /* member slots per 64-lane wavefront: 0 = auto (64, except that a single-reach ensemble too small
                                to fill the chip's SIMDs with full waves under an adaptive integrator is spread over more,
                                thinner waves: a wave's day costs the attempts of its slowest lane), 1..64 = as given.
                                Results are unchanged bit for bit.                                               */
    int32_t  lanes_per_member;/* lanes of a wavefront that work on one member: 1, or 4 (integrator 2 only) = a member's Cash-Karp
                                attempt spread over a DPP quad -- one lane each for the two soil boxes, the groundwater and the
                                reach; stage sums, error norm and state update three components per lane instead of eleven --
                                which makes an attempt ~1.4 x shorter.  0 = auto: 4 for an ensemble so small
                                (ceil(E / 16) x S <= SIMDs, i.e. E <= 16 384 single-reach members on MI355X) that the run is
                                bound by one member's serial chain of attempts rather than by throughput -- and for
                                single-reach ensembles up to 1.75 x that size (28 672 members), whose quads then share all
                                SIMDs through the task queue where one-lane waves would occupy a third of them --, else 1.
                                lanes_per_wave then counts member slots of 4 lanes (at most 16).  Results are unchanged bit
                                for bit for every member whose status is 0.                                      */
    int32_t  stiff_pair;     /* integrator 2: attempts whose step is bound by Cash-Karp's stability interval (a reach far down a
                                network relaxes at several hundred per day; |h x rate| <= 3.73) are taken by a second, stability-
                                optimised explicit 4(3) pair of the same 6 stages (include/simplyp_controller.h SIMPLYP_STIFF_*),
                                chosen lane by lane and attempt by attempt from the lane's own state.  0 = auto: on for reach
                                networks (S > 1), off for a single reach; > 0 on; < 0 off.  The same switch turns on the
                                damping-aware error weights (SIMPLYP_DAMP_*: the estimate of what a fast reach forgets within a
                                fraction of the day -- its flow, its three masses -- is discounted accordingly).  Same <= 1e-6
                                parity bar; 40 % fewer right-hand sides on BASELINE config C4.  Pinned to reference-made
                                tables on chains (C4's, the stiff 12-reach one, dry headwaters), a one-level confluence, a
                                two-level one of five reaches (tests/golden/net5_*.npz: static EPC0 on newly-converted land of
                                both kinds, with and without dynamic erodibility, and S-type new land paired with a last
                                sub-catchment of type A or without new land; 1.2e-7) and a branching 22-reach network
                                (tests/golden/branch_network.npz: 3.2e-7 there, 1.1 x Cash-Karp alone); other topologies and
                                regimes are not.  -1 is the conservative switch: Cash-Karp alone. */
    /* ---- forcing uncertainty (simplyp_run / simplyp_run_async only; all zero = off, and the run takes the path it took before
       these fields existed).  Appended at the end of the struct: a caller COMPILED AGAINST THE SHORTER STRUCT MUST BE REBUILT
       (the library reads these fields of whatever it is handed); one that memsets sizeof(simplyp_opts) needs no other change.
       With forcing_error = 1 every member reads a forcing set of its own, made on the device before the pilot and the main
       launches from the caller's base sets (`forcing`, `forcing_of_member`):
           z      = the counter-based normal of simplyp_predictive_bands at the counter
                    (forcing_member0 + e, forcing_group_of_day[r][d], r, SIMPLYP_FORCING_STREAM), key forcing_seed
           row 0  (P, or Precipitation with opts.snow), row 1 (PET):
                    v' = (v * scale[e]) * exp(sigma_r * z - 0.5 * sigma_r * sigma_r)      mean-one lognormal multiplier
           row 2  (T_air, opts.snow only):
                    v' = (v + offset[e]) + sigma_2 * z
       evaluated in that order without fused multiply-adds.  sigma_r = 0: no draw, the row is v * scale (v + offset); no
       forcing_shift either: the base value bit for bit.  A dry day stays exactly 0.  A draw depends on (seed, member id, group id,
       row) and on nothing else.
       Autocorrelated errors (forcing_rho[r] > 0): z of row r is an AR(1) over consecutive groups along the days.  Day d starts
       a step when its group id differs from the previous day's (for d = 0: from the last group id of forcing_noise_in, none
       without one); at a step, with eps the draw above at the day's group id,
           z = eps                                        when there is no previous z: a stationary start
           z = (forcing_rho[r] * z_prev) + (c * eps)      otherwise, c = sqrt(1 - rho * rho) in fp64
       each product and the sum rounded; the other days reuse z.  A group id that comes back after other ids is a new step that
       reuses its eps.  The noise state is a table [6][E] of doubles in member order: rows 0-2 z of P, PET, T_air, rows 3-5 that
       row's last group id as an exact double, -1.0 = none (a row without rho: 0.0 / -1.0 on output, ignored on input).  A run
       over D1 + D2 days equals a run over D1 days followed by one over D2 days handed the first one's state, bit for bit,
       wherever the cut falls.  AR orders above one, correlation between rows and a rho per member are not offered.          */
    int32_t  forcing_error;             /* 1: on                                                                             */
    uint32_t forcing_member0;           /* id of the call's member 0 in the stream (a member block of a larger ensemble)     */
    uint64_t forcing_seed;              /* key of the stream                                                                 */
    double   forcing_sigma[3];          /* per row, finite and in [0, 2]; [2] > 0 needs opts.snow                            */
    const int32_t* forcing_group_of_day[3]; /* device [D] each, ids in [0, 2^31): the days of one group share one draw per member
                                           and row (the day's ordinal: daily errors; year * 12 + month - 1: monthly; a storm id; one
                                           id: a constant multiplier per member).  Required for a row with sigma > 0        */
    const double*  forcing_shift;       /* device [forcing_shift_rows][E] in member order -- P scale, PET scale, T_air offset --
                                           or NULL: no scale, no offset                                                      */
    int32_t  forcing_shift_rows;        /* rows of forcing_shift: 0 with NULL, else 2 (the scales) or 3 (and the T_air offset:
                                           needs opts.snow)                                                                  */
    int32_t  forcing_pet_model;         /* 0: off; 1: Thornthwaite PET from the member's own T_air row (below).  This is the
                                           slot of the former forcing_reserved, which had to be 0: same offset, same size    */
    double*  forcing_table;             /* device [E][2 or 3][D] fp64, caller-owned workspace the sets are written to (required):
                                           the layout `forcing` has with n_forcing_sets = E; valid after the run.  With
                                           forcing_pet_model = 1 the workspace is SIMPLYP_FORCING_PET_PLAN_BYTES(D) longer: the
                                           caller's plan stands behind the table (below) and is only read                    */
    double   forcing_rho[3];            /* per row, finite and in [0, 0.999]: lag-one correlation between consecutive groups;
                                           > 0 needs forcing_sigma > 0 and forcing_group_of_day of that row                  */
    const double*  forcing_noise_in;    /* device [6][E] or NULL: stationary start                                           */
    double*        forcing_noise_out;   /* device [6][E] or NULL; may be the same buffer as forcing_noise_in                 */
    const int32_t* forcing_shift_group_of_day; /* device [D], ids in [0, forcing_shift_groups) (an id outside reads the nearest
                                           end), or NULL: seasonal change factors, e.g. month - 1                            */
    int32_t  forcing_shift_groups;      /* 0: forcing_shift is [rows][E] as before; G in [1, 4096]: [rows][G][E], needs the array
                                           above                                                                             */
    int32_t  forcing_reserved2;         /* 0                                                                                 */
    /* ---- Thornthwaite PET from each member's own air temperature (forcing_pet_model = 1; forcing_error = 1 and opts.snow = 1
       only).  No field is added for it: the struct keeps its size and every offset, forcing_pet_model is the former
       forcing_reserved, and the plan travels in the workspace.  The PET row of member e is
           PET[e][d] = TH[e][d] * F[e][d]
       TH: Thornthwaite's 1948 rule (below) applied to the member's FINAL T_air row of the table, (base + offset) + sigma z as
       the generator wrote it; F: exactly what the generator writes for a base PET of 1.0, (1.0 * scale) * exp(sigma z - 0.5
       sigma sigma), 1.0 bit for bit with neither.  The base PET row is not read.  The kernel runs on the run's stream after the
       generator and before the pilot and the main launches.
       The run must be whole calendar years of daily values, Y = D / 365 of them (integer division; D - 365 Y leap days, at most
       Y / 4 + 1, else the call is refused), Y <= SIMPLYP_FORCING_PET_YEARS_MAX, M = 12 Y months counted from the first January,
       year y = m / 12.  The plan is made by the caller from the calendar and the latitude and stands behind the table, at
       forcing_table + E * 3 * D doubles, in this order:
           double  daylight[M]   L, the month's mean daylight hours at the latitude (FAO-56 eq. 24, 25, 34)
           int32_t month[2][M]   the day index of the month's first day; N = its number of days (<= 31; days outside the run
                                 are left out of the sum)
           int32_t day[3][D]     j = the month whose 16th is the node at or before day d (0 before the first node; outside
                                 [0, M) reads the nearest end); k = days since that node (0 after the last node and before the
                                 first); n = days from node j to node j + 1
       and the rule, every operation rounded once, no fused multiply-add, pow(x, y) = exp(y * log(x)) for x > 0, 0.0 for
       x == 0, NaN otherwise:
           T_m   = (sum of the month's T_air, left to right in day order) / N;   T_m = T_m * (T_m >= 0 ? 1 : 0)
           I_y   = sum over the year's months in order of (T_m / 5 > 0 ? pow(T_m / 5, 1.514) : 0)
           a_y   = (((6.75e-7 * ((I * I) * I)) - (7.71e-5 * (I * I))) + (1.792e-2 * I)) + 0.49239
           V_m   = ((((1.6 * (L / 12)) * (N / 30)) * pow((10 * T_m) / I_y, a_y)) * 10) / N          mm per day, on the 16th
           TH[d] = V_j                                            when k == 0
                   V_j + ((V_j+1 - V_j) / n) * k                  otherwise
       A year whose monthly means are all <= 0 has I = 0 and V = 0 / 0 = NaN: the member's PET is NaN there and its run ends
       with the non-finite status.  The cap on the years: the monthly values live in LDS.                                     */
} simplyp_opts;

#define SIMPLYP_FORCING_PET_YEARS_MAX 64     /* years of a Thornthwaite plan: 2 x 768 monthly doubles of LDS per workgroup */
/* bytes of the plan behind forcing_table for a run of D days: daylight[M], month[2][M], day[3][D], M = 12 * (D / 365) */
#define SIMPLYP_FORCING_PET_PLAN_BYTES(D) (16LL * 12 * ((D) / 365) + 12LL * (D))

#define SIMPLYP_FORCING_STREAM 0x464F5243u   /* "FORC": the fourth word of the counter of a forcing draw */

typedef struct {
    uint64_t rhs_evals;      /* right-hand-side evaluations, all members/reaches/days      */
    uint64_t steps;          /* accepted steps                                             */
    uint64_t rejected;       /* rejected steps (Cash-Karp)                                 */
    double   kernel_ms;      /* device time of the main launches of this run (HIP events on the run's stream) */
    double   pilot_ms;       /* load balancing: pilot launches + host sort of the cost keys (0 when off)      */
    double   simt_efficiency;/* adaptive integrators: lanes that needed the attempt / lanes that executed it (1 = no
                                divergence between the members of a wavefront)                                  */
    int32_t  n_launches;     /* kernel launches issued (one per routing stage)             */
    int32_t  balanced;       /* 1 when the cost-sorted member order was used                */
    int32_t  queued;         /* 1 when the time-chunk task queue kernel ran                  */
    int32_t  lanes_per_wave; /* member slots per wavefront the run used (opts.lanes_per_wave)                     */
    int32_t  lanes_per_member;/* lanes per member the run used (opts.lanes_per_member): 1 or 4                          */
    int32_t  streamed_chunks;/* simplyp_stream_out: time chunks whose device-to-host copy started while the kernel was still
                                running (0 = the table was copied after the last launch)                           */
    double   d2h_tail_ms;    /* simplyp_stream_out: device time between the end of the last launch and the last output
                                byte reaching the host buffer (what the copy added to the run; 0 when not armed)   */
    double   wall_ms;        /* host wall clock from the entry of simplyp_run / simplyp_run_async to the end of simplyp_sync */
    double   stream_gbs;     /* simplyp_stream_out, chunked runs: table bytes / device time from the start of the main launch to
                                the last output byte in the host buffer, GB/s (0 otherwise) -- a diagnostic of the PCIe link */
    uint64_t queue_waits;    /* task-queue kernel: dependency waits (own previous chunk, upstream reach, ring reader) that
                                found their flag not yet raised and had to poll                                        */
    uint32_t queue_longest_wait_polls;  /* the longest of them, in polls (~2 us each)                                   */
    uint32_t pack_overflow_blocks;      /* packed output stream: 64-member blocks in which a coded difference needs more than
                                56 bits (records sent raw not counted)                                                */
    uint64_t queue_longest_stall_polls; /* the longest stretch of polls, inside any such wait, during which NO task of the run
                                completed: what the wait's bound counts (simplyp_sync)                                 */
    int32_t  stiff_pair;     /* 1 when the run used the stability-optimised second pair (opts.stiff_pair resolved to on)  */
    int32_t  packed_records; /* packed output stream (simplyp_stream_out with SIMPLYP_STREAM_PACK): low 16 bits = (time chunk,
                                column) records delivered packed and decoded on the host, high 16 bits = records of
                                such a run sent as raw fp64 because they had too many wide blocks.  0: the stream was not packed */
} simplyp_stats;

typedef struct simplyp_ctx simplyp_ctx;

int  simplyp_abi_version(void);
int  simplyp_device_count(void);

/* A context is bound to one HIP device and owns a stream, two events and grow-only device
 * scratch (routing series between reaches, launch schedule).  Not re-entrant; distinct
 * contexts may be driven from distinct host threads. */
int  simplyp_ctx_create(int device, simplyp_ctx** out);
void simplyp_ctx_destroy(simplyp_ctx* ctx);
const char* simplyp_last_error(const simplyp_ctx* ctx);   /* ctx may be NULL: create errors */
/* Run on the caller's stream (a hipStream_t passed as void*, e.g. torch.cuda.current_stream()
 * .cuda_stream) so the launches order with the caller's own copies; NULL = a private stream. */
int  simplyp_ctx_set_stream(simplyp_ctx* ctx, void* hip_stream);

/* Bytes of `out` that simplyp_run will write: popcount(out_mask) * (n_periods ? n_periods : D) * n_out_reaches * E * 8. */
int64_t simplyp_out_bytes(const simplyp_dims* dims, const simplyp_opts* opts, int32_t n_out_reaches);

/*
 * simplyp_run -- integrate every (member, reach) through all D days.
 * Replaces model.py:365-724 for the whole ensemble in one call.
 *
 *   forcing           device  [n_forcing_sets][2][D]   row 0 = P (met_df['P'], model.py:497),
 *                                                      row 1 = PET (model.py:498);
 *                             with opts.snow = 1: [n_forcing_sets][3][D], rows Precipitation, PET, T_air
 *   doy               device  [D]        day of year 1..366 (met_df.index[idx].dayofyear, :550)
 *   period_of_day     device  [D] int32 in [0, opts.n_periods), or NULL when opts.n_periods == 0
 *   forcing_of_member device  [E] or NULL (all members use set 0)
 *   member_params     device  [SIMPLYP_NP_M][E]
 *   reach_params      device  [SIMPLYP_NP_R][S][E]
 *   up_ptr, up_idx    host    CSR of directly-upstream reaches (p_struc 'Upstream_SCs',
 *                             model.py:480-487), zero-based, up_idx[k] < own id, shared by all
 *                             members; up_ptr has S+1 entries
 *   out_reaches       host    [n_out_reaches] reaches whose columns are written, or NULL = all S
 *   out               device  [n_cols][D or n_periods][n_out_reaches][E] fp64, n_cols = popcount(out_mask),
 *                             columns in ascending SIMPLYP_OUT_* order
 *   member_status     device  [E] int32, OR of SIMPLYP_STATUS_* bits (zeroed by the call)
 *   member_of_slot    device  [E] int32 or NULL: with opts.out_slot_order = 1, column j of `out` belongs to member
 *                             member_of_slot[j] (required in that mode)
 *   member_rhs_evals  device  [E] uint32 or NULL: right-hand-side evaluations spent on each member, summed
 *                             over its reaches and days (what LSODA's infodict['nfe'] was to the reference's
 *                             caller; also the key the host sorts members by, see simplyp_amd/engine.py)
 *   stats             host    may be NULL
 *
 * The call is synchronous: it returns after the last kernel has finished.
 */
int simplyp_run(simplyp_ctx* ctx, const simplyp_dims* dims, const simplyp_opts* opts,
                const double* forcing, const int32_t* doy, const int32_t* period_of_day,
                const int32_t* forcing_of_member,
                const double* member_params, const double* reach_params,
                const int32_t* up_ptr, const int32_t* up_idx,
                const int32_t* out_reaches, int32_t n_out_reaches,
                double* out, int32_t* member_status, int32_t* member_of_slot, uint32_t* member_rhs_evals,
                simplyp_stats* stats);

/*
 * simplyp_plan -- the routing schedule simplyp_run will use for a reach graph, without touching a
 * device (host-only; also what the CPU tests check).  Reaches are grouped into launches; inside a
 * launch each chain is walked by one thread per member, upstream to downstream.
 *   launch_of_reach, chain_of_reach, pos_in_chain, route_slot : host [S] outputs (any may be NULL);
 *   route_slot[s] = slot of the routing buffer that carries reach s's daily series downstream, -1
 *   when no reach reads it.  n_launches / n_slots: totals.
 */
int simplyp_plan(int32_t S, const int32_t* up_ptr, const int32_t* up_idx,
                 int32_t* n_launches, int32_t* n_slots,
                 int32_t* launch_of_reach, int32_t* chain_of_reach, int32_t* pos_in_chain, int32_t* route_slot);

/* Same as simplyp_run but returns once the main launch is enqueued on the context's stream (for overlap with the
 * caller's own copies); simplyp_sync() waits and fills `stats`.  With load balancing active (opts.balance) the call
 * first BLOCKS for the pilot: pilot launches, a device-to-host copy of the cost table, the member ordering on host
 * threads and the upload of the permutation (stats.pilot_ms, ~12 ms for 100 000 members) happen before it returns. */
int simplyp_run_async(simplyp_ctx* ctx, const simplyp_dims* dims, const simplyp_opts* opts,
                      const double* forcing, const int32_t* doy, const int32_t* period_of_day,
                      const int32_t* forcing_of_member,
                      const double* member_params, const double* reach_params,
                      const int32_t* up_ptr, const int32_t* up_idx,
                      const int32_t* out_reaches, int32_t n_out_reaches,
                      double* out, int32_t* member_status, int32_t* member_of_slot, uint32_t* member_rhs_evals);
/* simplyp_sync fails with SIMPLYP_ERR_DEVICE ("no task completed for ... polls") when a wave of the task-queue kernel waited
 * for a dependency while NO task of the whole run completed for `max_polls` polls (2e7 x ~2 us; environment variable
 * SIMPLYP_QUEUE_MAX_POLLS) -- a run that is merely slow (a shared GPU, a profiler) keeps completing tasks and never fails;
 * results are incomplete after such an error.  On every exit, error or not, the streamed-output machinery is quiesced: the
 * copier thread joined, the decode pool of a packed stream drained and joined, both copy streams idle, nothing of the library
 * still writes to the host buffer. */
int simplyp_sync(simplyp_ctx* ctx, simplyp_stats* stats);

/*
 * simplyp_stream_out -- deliver the NEXT run's output table to host memory as well (one-shot; NULL disarms).
 * One-shot means: the next simplyp_run / simplyp_run_async consumes the arm whatever its outcome -- also when it is refused
 * for its arguments -- so a buffer the caller has since freed is never written by a later run.
 * The reference produces its 25 values per catchment-day in host memory (model.py:644, :721-724); an ensemble's table is
 * tens of GB, so the copy is overlapped with the computation: adaptive integrators then run through the time-chunk task
 * queue (opts.time_chunk_days = 0 then means 64-day chunks for a single reach, 256 for a network), the wave that finishes the
 * last task of a time chunk raises a flag in pinned host memory, and a host thread of the library enqueues that chunk's rows (one contiguous block per column) on a
 * second HIP stream while later chunks compute.  simplyp_sync / simplyp_run return once the last byte is in `host_out`;
 * stats.d2h_tail_ms is what the copy added after the last launch.  Runs without time chunks (RK4, opts.time_chunk_days < 0,
 * time-reduced rows, runs no longer than one chunk) copy the whole table after the last launch.
 *   host_out    host  same layout and size as `out` (simplyp_out_bytes); pinned memory (simplyp_host_alloc) for the copy
 *                     engine to run at PCIe speed beside the kernel -- pageable memory works, slowly
 *   host_bytes  capacity of host_out, checked against the table size at the run
 * The device table `out` is written as always (it feeds simplyp_gof / simplyp_waterbody).
 */
int simplyp_stream_out(simplyp_ctx* ctx, double* host_out, int64_t host_bytes);

/*
 * The packed output stream.  The daily table is smooth from day to day: per (column, member), the zigzag-coded difference of
 * consecutive days' 64-bit patterns needs about 50 bits, and all 64 members of a block need few bits on the same days.  An
 * eligible streamed run -- time chunks through the task queue, daily rows (n_periods = 0), one reach, one lane per member, 64
 * member slots per wave, lane slots contiguous in the table (opts.out_slot_order = 1, or no load balancing) -- can therefore
 * send each (time chunk, column) as one packed record in which every row of a block (64 members, one day) is stored at the bit
 * width of its widest difference: the wave that computed a task packs its own rows before it releases the task, the copier
 * sends the record into a pinned staging ring, and a pool of host threads decodes it into `host_out` with non-temporal stores.
 * SIMPLYP_OUT_PP_FLUX is coded against Msus[d] * (PP[d-1] / Msus[d-1]), or against Msus[d] times that ratio extrapolated from
 * the two days before, whichever makes a span of 64 rows of a block smaller, instead of the previous day when
 * SIMPLYP_OUT_MSUS_FLUX is in the table too.  A block with a difference of more than 56 bits counts as an overflow block (it simply has wide rows); a
 * record with more of them than an eighth of its blocks plus three, or whose body outgrows 7 bytes per value, travels as raw
 * fp64.  The result is bit for bit the table of the raw stream; the device table is untouched.  simplyp_sync returns after the
 * pool has drained, on every path.
 * Environment: SIMPLYP_STREAM_PACK = 0 never, 1 whenever eligible, unset = auto (only when the raw copies
 * would outlast the kernel); SIMPLYP_DECODE_THREADS = size of the decode pool (default: the CPUs this process may run on,
 * capped by OMP_NUM_THREADS, minus two).
 *
 * simplyp_fetch_packed -- a caller's device table [n_cols][rows][row_doubles] to host memory through the same pack device
 * function, copier and decoder (blocks of 64 consecutive doubles of a row; chunk_days is rounded up to a multiple of 64; at
 * most 32 columns).
 * counts (host, may be NULL): [0] records decoded, [1] overflow blocks among them, [2] records sent raw.  Synchronous.
 *
 * simplyp_pack_roundtrip_host -- host only, no device: encodes `table` in plain C++ into records of the same layout and decodes
 * them with the decoder of the stream into `out` (raw records are copied); counts as above.
 *
 * simplyp_fetch_packed_pred, simplyp_pack_roundtrip_host_pred -- the same two with a predictor per column and the bytes:
 * pred_col (host, [n_cols], NULL = all -1): -1 = a column is coded against its previous day, k < the column's own index = against
 * X[d] * r[d-1] or X[d] * (2 r[d-1] - r[d-2]) with r = Y / X and X = column k, chosen per block and span (simplyp_pack.h).  bytes (host, may be NULL): [0] bytes of all packed records as they cross the link,
 * [1] bytes of their raw first rows.
 */
int simplyp_fetch_packed(simplyp_ctx* ctx, const double* dev_table, int32_t n_cols, int32_t rows, int32_t row_doubles,
                         int32_t chunk_days, double* host_out, int64_t host_bytes, int32_t* counts);
int simplyp_pack_roundtrip_host(const double* table, int32_t n_cols, int32_t rows, int32_t row_doubles, int32_t chunk_days,
                                double* out, int32_t* counts);
int simplyp_fetch_packed_pred(simplyp_ctx* ctx, const double* dev_table, int32_t n_cols, int32_t rows, int32_t row_doubles,
                              int32_t chunk_days, const int32_t* pred_col, double* host_out, int64_t host_bytes, int32_t* counts,
                              int64_t* bytes);
int simplyp_pack_roundtrip_host_pred(const double* table, int32_t n_cols, int32_t rows, int32_t row_doubles, int32_t chunk_days,
                                     const int32_t* pred_col, double* out, int32_t* counts, int64_t* bytes);

/*
 * simplyp_set_state -- warm start: begin the NEXT run from a saved model state and / or save the state it ends in
 * (one-shot, with exactly the contract of simplyp_stream_out: the next simplyp_run / simplyp_run_async consumes the arm
 * whatever its outcome, also when it is refused for its arguments; (NULL, NULL) disarms).
 *   state_in   device  [S][SIMPLYP_N_STATE][E] or NULL.  Every (member, reach) starts its first day from these rows
 *                      instead of the reference's cold initial conditions (model.py:377-459); parameters and everything
 *                      derived from them (mu, Kf, ...) come from member_params / reach_params as always.  The load
 *                      balancer's pilot keeps starting cold: it only ranks costs, results do not depend on the order.
 *   state_out  device  [S][SIMPLYP_N_STATE][E] or NULL.  The state after the run's last day; valid when simplyp_run returns /
 *                      after simplyp_sync.  May alias state_in: each (reach, member) cell is read before the run's first
 *                      day and written after its last, by tasks that depend on each other.
 * Both are indexed by MEMBER, whatever opts.balance, opts.out_slot_order, lanes_per_wave and lanes_per_member did.
 * The status bits of a resumed run start from zero: the status of a run made in pieces is the OR over the pieces (a member
 * that went non-finite carries the NaN in its state and is flagged again).
 * simplyp_state_bytes: S * SIMPLYP_N_STATE * E * 8 (host only; -1 for NULL or non-positive dims).
 */
int64_t simplyp_state_bytes(const simplyp_dims* dims);
int simplyp_set_state(simplyp_ctx* ctx, const double* state_in, double* state_out);

/* Host-pinned staging buffers for callers that do not use torch (hipHostMalloc/hipHostFree). */
void* simplyp_host_alloc(int64_t bytes);
void  simplyp_host_free(void* p);

/* Plain device buffers + copies for callers without a device allocator of their own. */
void* simplyp_device_alloc(simplyp_ctx* ctx, int64_t bytes);
void  simplyp_device_free(simplyp_ctx* ctx, void* p);
int   simplyp_memcpy_h2d(simplyp_ctx* ctx, void* dst, const void* src, int64_t bytes);
int   simplyp_memcpy_d2h(simplyp_ctx* ctx, void* dst, const void* src, int64_t bytes);

/* ---- what every entry below has in common (the reductions over a table, the samplers' steps, simplyp_eval_units) ----------
 * A NULL context is SIMPLYP_ERR_ARG.  While a run is pending on the context -- simplyp_run_async without its simplyp_sync --
 * every one of them returns SIMPLYP_ERR_ARG ("<entry>: a run is pending on this context; call simplyp_sync first") and launches
 * nothing: they time themselves with the events the pending run's statistics are read from.  A call refused for its arguments
 * has launched nothing either and leaves `info` as it was; a call that succeeds has written every field of `info`. */

/* ---- goodness of fit per member (the reference's goodness_of_fit_stats, visualise_results.py:387-474, for a whole
 * ensemble on the device) ------------------------------------------------------------ */
enum {  /* variables, in the order of stats_var_li (visualise_results.py:400); simulated series = df_R columns
           Q_cumecs, SS_mgl, TDP_mgl, PP_mgl, TP_mgl, SRP_mgl (:413-414; model.py:784-793, :831-847) */
    SIMPLYP_GOF_Q = 0, SIMPLYP_GOF_SS, SIMPLYP_GOF_TDP, SIMPLYP_GOF_PP, SIMPLYP_GOF_TP, SIMPLYP_GOF_SRP,
    SIMPLYP_N_GOF_VARS
};
enum {  /* rows of `gof`: the reference's table columns (:460-461) except Spearman's r (a rank statistic: host only),
           plus the two sums the reference's Gaussian likelihood with sigma = m*sim needs
           (Development/2016/MCMC.ipynb cell 6):
           loglik(m) = -n/2 ln(2 pi) - n ln m - SUM_LOG_SIM - SUM_RELSQ / (2 m^2)                               */
    SIMPLYP_GOFSTAT_N_OBS = 0,    /* non-null observations of the variable in the run period (:428)             */
    SIMPLYP_GOFSTAT_NSE,          /* 1 - sum (obs-sim)^2 / sum (obs-mean obs)^2                         (:441)  */
    SIMPLYP_GOFSTAT_LOG_NSE,      /* the same on natural logs                                            (:442)  */
    SIMPLYP_GOFSTAT_R2,           /* squared Pearson correlation                                         (:446)  */
    SIMPLYP_GOFSTAT_PBIAS,        /* 100 sum (sim-obs) / sum obs                                         (:448)  */
    SIMPLYP_GOFSTAT_NRMSD,        /* 100 mean |sim-obs| / std(obs), ddof 0                               (:449)  */
    SIMPLYP_GOFSTAT_SUM_LOG_SIM,  /* sum ln sim over the paired days                                             */
    SIMPLYP_GOFSTAT_SUM_RELSQ,    /* sum (obs/sim - 1)^2 over the paired days                                    */
    SIMPLYP_N_GOF_STATS
};

typedef struct {
    double  kernel_ms;        /* both kernels, HIP events on the context's stream                                */
    int64_t bytes_read;       /* algorithmic bytes: 8 per member and discharge day + 32 per member and chemistry day */
    int32_t n_q_days;         /* discharge-observation days summed over the output reaches                       */
    int32_t n_chem_days;      /* days with any chemistry observation, summed over the output reaches             */
    int32_t n_chunks_q;       /* slices the discharge-day lists were cut into                                    */
    int32_t n_chunks_chem;    /* slices the chemistry-day lists were cut into                                    */
} simplyp_gof_info;

/*
 * simplyp_gof -- statistics of every member's simulated series against shared observations, from the daily table a
 * previous simplyp_run left on the device.  Variables with 10 or fewer observations get NaN rows (the reference drops
 * them, :430, :453); a day is used when the observation and the simulated value are both non-NaN (:436).  A day whose
 * logarithm does not exist (a negative observation, a negative simulated value) drops out of the sums of log NSE it would
 * enter, and the mean log observation runs over the days that have one -- what the reference's NaN-skipping sums do (:442-443).
 *
 *   dims            E, S, D as in the run (n_forcing_sets ignored)
 *   out_mask, out_reaches, n_out_reaches   as passed to simplyp_run; the mask must contain Qr, Msus_kg/day,
 *                   TDP_kg/day and PP_kg/day, and the run must have written daily rows (opts.n_periods == 0)
 *   out             device  [popcount(out_mask)][D][n_out_reaches][E]
 *   member_of_slot  device  [E] or NULL (columns of `out` are in member order)
 *   f_tdp           device  [E]: p['f_TDP'] of each member (SRP = f_TDP * TDP, model.py:844); not a run parameter
 *   reach_params    device  as in the run (row SIMPLYP_PR_A_CATCH is read)
 *   obs             HOST    [n_out_reaches][SIMPLYP_N_GOF_VARS][D], NaN = no observation that day
 *   gof             device  [SIMPLYP_N_GOF_STATS][SIMPLYP_N_GOF_VARS][n_out_reaches][E], member order
 *   info            host    may be NULL
 * Synchronous.
 */
int simplyp_gof(simplyp_ctx* ctx, const simplyp_dims* dims, uint32_t out_mask,
                const int32_t* out_reaches, int32_t n_out_reaches,
                const double* out, const int32_t* member_of_slot,
                const double* f_tdp, const double* reach_params,
                const double* obs, double* gof, simplyp_gof_info* info);

/*
 * simplyp_gof_spearman -- Spearman's r (visualise_results.py:444-445: DataFrame.corr(method='spearman'), the Pearson
 * correlation of the average ranks of the paired observed and simulated values) of every member, the one column of the
 * reference's table that simplyp_gof does not produce.  A rank statistic: each member's simulated values on the
 * observation days are ranked among themselves by counting (n^2 compares per member and variable, n <= a few thousand),
 * so this pass costs ~0.1-0.2 s for a 100 000-member table where simplyp_gof costs milliseconds -- call it when wanted.
 * Arguments as for simplyp_gof;
 *   rho   device  [SIMPLYP_N_GOF_VARS][n_out_reaches][E], member order; NaN for variables with 10 or fewer observations and
 *                 for members with a NaN simulated value on an observation day (the reference would rank the remaining
 *                 pairs; such members carry SIMPLYP_STATUS_NONFINITE anyway)
 *   info  kernel_ms = all passes; bytes_read = rows of the compact value table streamed in the counting pass
 */
int simplyp_gof_spearman(simplyp_ctx* ctx, const simplyp_dims* dims, uint32_t out_mask,
                         const int32_t* out_reaches, int32_t n_out_reaches,
                         const double* out, const int32_t* member_of_slot,
                         const double* f_tdp, const double* reach_params,
                         const double* obs, double* rho, simplyp_gof_info* info);

/* ---- receiving waterbody: the reference's sum_to_waterbody (model.py:851-900) for a whole ensemble -------------------- */
enum {  /* columns of the reference's df_summed, in its order: the four summed series (vars_to_sum, :866), the three
           volume-weighted concentrations (:886-888), derived_P_species (:842-845) */
    SIMPLYP_WB_Q_CUMECS = 0, SIMPLYP_WB_MSUS_FLUX, SIMPLYP_WB_TDP_FLUX, SIMPLYP_WB_PP_FLUX,
    SIMPLYP_WB_SS_MGL, SIMPLYP_WB_TDP_MGL, SIMPLYP_WB_PP_MGL,
    SIMPLYP_WB_TP_MGL, SIMPLYP_WB_TP_FLUX, SIMPLYP_WB_SRP_MGL, SIMPLYP_WB_SRP_FLUX,
    SIMPLYP_N_WB
};
#define SIMPLYP_WB_MASK_ALL ((uint32_t)((1u << SIMPLYP_N_WB) - 1u))

typedef struct {
    double  kernel_ms;        /* HIP events on the context's stream                                              */
    int64_t bytes_moved;      /* algorithmic bytes: 32 read per member, day and summed reach + 8 written per member, day
                                 and requested column                                                            */
} simplyp_wb_info;

/*
 * simplyp_waterbody -- sum the daily series of the reaches that flow into the receiving waterbody
 * (p_struc['In_final_flux?'] == 1, model.py:867) into one series per member, from the table a previous simplyp_run left
 * on the device: Q_cumecs (= Qr * A_catch * 1000 / 86400 per reach, :784) and the three daily fluxes added in ascending
 * reach order (DataFrame.sum: NaN counts as 0), concentrations = (flux / Q_cumecs) * 1000/86400, TP and SRP as
 * derived_P_species.  Same operations in the same order as the reference: bit-identical to its restatement in
 * oracle/waterbody.py.  The reference returns nothing for fewer than two flagged reaches (:872, :895); the host wrapper
 * keeps that rule, this entry sums whatever it is given (n_sum >= 1).
 *
 *   dims, out_mask, out_reaches, n_out_reaches, out, member_of_slot   as for simplyp_gof (daily rows; the mask must
 *                   contain Qr and the three fluxes)
 *   f_tdp           device  [E], member order (p['f_TDP'])
 *   reach_params    device  as in the run (row SIMPLYP_PR_A_CATCH is read)
 *   sum_reaches     host    [n_sum] zero-based reach ids, ascending, each one of the table's output reaches; n_sum <= 16
 *   wb_mask         bit c set -> column c (SIMPLYP_WB_*) is written
 *   wb              device  [popcount(wb_mask)][D][E]; member axis in the order of `out`'s (slots when the run wrote
 *                           slot order)
 *   info            host    may be NULL
 * Synchronous.
 */
int simplyp_waterbody(simplyp_ctx* ctx, const simplyp_dims* dims, uint32_t out_mask,
                      const int32_t* out_reaches, int32_t n_out_reaches,
                      const double* out, const int32_t* member_of_slot,
                      const double* f_tdp, const double* reach_params,
                      const int32_t* sum_reaches, int32_t n_sum,
                      uint32_t wb_mask, double* wb, simplyp_wb_info* info);

/*
 * simplyp_gof_waterbody -- simplyp_gof for the summed series: statistics of every member's waterbody series (table
 * written by simplyp_waterbody) against observations taken at the waterbody's inflow.
 *   dims            E, D (S, n_forcing_sets ignored)
 *   wb_mask, wb     as written by simplyp_waterbody; the mask must contain Q_cumecs and the three summed fluxes
 *   obs             HOST  [SIMPLYP_N_GOF_VARS][D], NaN = no observation
 *   gof             device [SIMPLYP_N_GOF_STATS][SIMPLYP_N_GOF_VARS][1][E], member order
 */
int simplyp_gof_waterbody(simplyp_ctx* ctx, const simplyp_dims* dims, uint32_t wb_mask, const double* wb,
                          const int32_t* member_of_slot, const double* f_tdp,
                          const double* obs, double* gof, simplyp_gof_info* info);

/* ---- percentile bands across the members: what the reference's only ensemble caller makes of its runs -- for every day the
 * 2.5 / 50 / 97.5 percentiles over the sampled parameter sets (Development/2016/MCMC.ipynb, get_uncertainty_intervals:
 * param_only.T.describe(percentiles=[0.025, 0.5, 0.975])) ---------------------------------------------------------------- */
typedef struct {
    double  kernel_ms;     /* all launches of the call, HIP events on the context's stream        */
    int64_t bytes_table;   /* n_rows * E * 8: the algorithmic read                                  */
    int32_t n_used;        /* members that took part (popcount of include, or E)                    */
    int32_t n_passes;      /* sweeps over a row the selection made (diagnostic)                     */
} simplyp_quantile_info;

/*
 * simplyp_quantiles -- exact order statistics across the member axis of any table of the library whose fastest axis is the
 * member axis: the run's `out` (daily or period-reduced), simplyp_waterbody's `wb`, a goodness-of-fit table; the leading
 * axes flattened to n_rows.  For every row and each probability q[k], with n = members that take part and h = q[k] * (n - 1)
 * in fp64: k_lo = floor(h), k_hi = min(k_lo + 1, n - 1), and the outputs are the row's k_lo-th and k_hi-th smallest
 * included values -- numpy's method='linear' indices (DataFrame.describe's too); the caller interpolates with
 * gamma = h - floor(h).  Exact selection (no sampling): every output is an element of its row, the one np.sort puts at that
 * index.  NaN sorts after +inf as in np.sort; -0.0 and +0.0 compare equal, either may be returned.  The table is only
 * read; device workspace is E + 16 bytes, whatever the table's size.  Results are deterministic bit for bit.
 *
 *   E, n_rows       row length (members), rows; n_rows == 0 succeeds and launches nothing
 *   table           device  [n_rows][E] fp64
 *   member_of_slot  device  [E] or NULL: as for simplyp_gof -- column j of the table belongs to member member_of_slot[j]
 *                           (tables a run wrote with opts.out_slot_order = 1); `include` is looked up through it
 *   include         device  [E] uint8 in MEMBER order, or NULL = all members: a member with 0 takes part in no row
 *                           (members flagged SIMPLYP_STATUS_NONFINITE; GLUE-style "behavioural" subsets).  When no member
 *                           is left (n == 0) every output is NaN and the call succeeds.
 *   q, K            HOST    [K] probabilities in [0, 1], 1 <= K <= 16
 *   order_stats     device  [2][K][n_rows]: plane 0 = x_(k_lo), plane 1 = x_(k_hi)
 *   info            host    may be NULL
 * Synchronous, on the context's stream.  SIMPLYP_ERR_ARG (nothing launched) for K outside 1..16, a q outside [0, 1] or
 * NaN, E < 1, n_rows < 0, NULL table / q / order_stats.
 */
int simplyp_quantiles(simplyp_ctx* ctx, int32_t E, int64_t n_rows, const double* table,
                      const int32_t* member_of_slot, const uint8_t* include,
                      const double* q /* host [K] */, int32_t K,
                      double* order_stats /* device [2][K][n_rows]: lower, upper */,
                      simplyp_quantile_info* info);

/* ---- order statistics per member over time: what a user of the reference gets from one DataFrame.quantile() call on the
 * frames run_simply_p returns -- the flow-duration curve (Q95, Q50, Q10), annual maxima (q = 1), the annual 90th percentile
 * of a concentration, the same for a season only -- for every member of an ensemble, from the table on the device ---------- */
#define SIMPLYP_TQ_DERIVED 64   /* series id = SIMPLYP_OUT_* (a column in out_mask) or SIMPLYP_TQ_DERIVED + SIMPLYP_GOF_* */

typedef struct {
    double  kernel_ms;     /* the selection kernel, HIP events on the context's stream                                  */
    int64_t bytes_read;    /* bytes of the table all sweeps loaded (512 per wave and day row, idle lanes included)       */
    int32_t n_sweeps;      /* the most sweeps over its period's days any (64 members, period, series, reach) needed      */
    int32_t n_periods;     /* max(n_periods, 1)                                                                          */
} simplyp_tq_info;

/*
 * simplyp_time_quantiles -- exact order statistics along the DAY axis of the daily table a previous simplyp_run left on the
 * device, for every (series, period, output reach, member).  With n = the period's participating days (the same for all
 * members) and h = q[k] * (n - 1) in fp64: k_lo = floor(h), k_hi = min(k_lo + 1, n - 1), and the outputs are the k_lo-th and
 * k_hi-th smallest values of the member's series over those days -- numpy's method='linear' indices; the caller interpolates
 * with gamma = h - floor(h).  Exact selection: every output is an element of the series, the one np.sort puts at that index.
 * NaN sorts after +inf as in np.sort; -0.0 and +0.0 compare equal, either may come back.  A period without days gives NaN.
 * The table is only read; device workspace is a few bytes per day and probability, whatever E and the table's size.
 * Results are deterministic bit for bit.
 *
 *   dims, out_mask, out_reaches, n_out_reaches, out, member_of_slot   as for simplyp_gof (daily rows); D == 0 succeeds
 *                   (every output NaN)
 *   f_tdp           device  [E] member order, and
 *   reach_params    device  as in the run (row SIMPLYP_PR_A_CATCH): read only when a derived series is asked for, else NULL
 *   series          HOST    [n_series], 1 <= n_series <= 32: SIMPLYP_OUT_c = column c of the table as it stands (must be
 *                           in out_mask), or SIMPLYP_TQ_DERIVED + SIMPLYP_GOF_v = the df_R series Q_cumecs, SS_mgl, TDP_mgl,
 *                           PP_mgl, TP_mgl, SRP_mgl of the reach (model.py:784-793, :842-845), computed on the fly with the
 *                           reference's operations one for one: Qr*A*1000/86400, (flux/Qr)/A, TDP+PP, TDP*f_TDP (out_mask
 *                           must contain Qr and the three fluxes)
 *   period_of_day   HOST    [D] in [-1, n_periods): -1 = the day takes part in no period (seasons); the non-negative
 *                           entries must not decrease.  NULL (n_periods 0) = one period holding every day
 *   q, K            HOST    [K] probabilities in [0, 1], 1 <= K <= 16
 *   order_stats     device  [2][K][n_series][max(n_periods, 1)][n_out_reaches][E]: plane 0 = x_(k_lo), plane 1 = x_(k_hi);
 *                           member axis in the order of `out`'s (slots when the run wrote slot order), as simplyp_waterbody
 *   n_days          HOST    [max(n_periods, 1)] the periods' participating days, or NULL
 *   info            host    may be NULL
 * Synchronous, on the context's stream.  SIMPLYP_ERR_ARG (nothing launched) for K outside 1..16, a q outside [0, 1] or NaN,
 * a series that is not in the mask, a derived series whose mask lacks Qr or a flux or with NULL f_tdp / reach_params, a
 * period_of_day that decreases or leaves [-1, n_periods), n_series outside 1..32, NULL out / q / order_stats / series.
 */
int simplyp_time_quantiles(simplyp_ctx* ctx, const simplyp_dims* dims, uint32_t out_mask,
                           const int32_t* out_reaches, int32_t n_out_reaches,
                           const double* out, const int32_t* member_of_slot,
                           const double* f_tdp, const double* reach_params,
                           const int32_t* series /* host [n_series] */, int32_t n_series,
                           const int32_t* period_of_day /* host [D] or NULL */, int32_t n_periods,
                           const double* q /* host [K] */, int32_t K,
                           double* order_stats, int32_t* n_days /* host or NULL */,
                           simplyp_tq_info* info);

/* ---- predictive bands: the second frame of the reference's get_uncertainty_intervals (Development/2016/MCMC.ipynb, cell 11) --
 * the percentiles across the members after sim + norm.rvs(loc=0, scale=m*sim) has been added to every member's series -- and
 * the bands of the six df_R series (and of plain columns) without it, selected on the device from series generated there.
 *
 * The draw is counter-based, a pure function of what it belongs to: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl
 * constants 0x9E3779B9, 0xBB67AE85) with key (seed & 0xffffffff, seed >> 32) and counter (member id, day0 + d,
 * out_reaches[r] = the zero-based model reach, series id as passed).  From its outputs x0..x3: h1 = ((x0 << 32) | x1) >> 12,
 * u1 = (h1 + 0.5) 2^-52, h2 / u2 alike from x2, x3 (exact in fp64, u in (0, 1)); z = sqrt(-2 ln u1) cospi(2 u2), |z| <= 8.58;
 * v' = v + (m v) z, two multiplies and an add.  Neither the launch shape, the slot a member sits in, the chunking, the window
 * nor the time enters; simplyp_amd/predictive.py restates the stream in NumPy. --------------------------------------------- */
typedef struct {
    double  kernel_ms;        /* all launches of the call, HIP events on the context's stream                              */
    double  gen_ms;           /* of these, the generation kernel's                                                         */
    int64_t bytes_read;       /* bytes of the run's table the generation read                                              */
    int64_t bytes_workspace;  /* the chunk of generated series in the context's workspace                                  */
    int32_t n_used;           /* members that took part                                                                    */
    int32_t n_passes;         /* sweeps over a row the selection made (diagnostic)                                         */
    int32_t n_chunks;         /* blocks of whole days generated and selected one after the other                           */
    int32_t reserved;
} simplyp_pred_info;

/*
 * simplyp_predictive_series -- the series themselves: individual noisy realisations (or the normals behind them) of every
 * member, into a caller-owned device table.
 *   dims, out_mask, out_reaches, n_out_reaches, out, member_of_slot, f_tdp, reach_params, series, n_series
 *                   as for simplyp_time_quantiles: `out` holds daily rows (dims->D of them; D == 0 succeeds, D < 0 is an error)
 *   err_m           device  [n_series][E] in MEMBER order: the error model's m per series and member, or NULL
 *   seed, day0      the stream's key; the absolute index of the table's first day (>= 0): windows of one run pass their offset
 *   which           0: the values -- v' = v + (m v) z with err_m, the series v itself without;  1: the normals z (needs err_m)
 *   table           device  [n_series][D][n_out_reaches][E], member axis in the order of `out`'s
 * Synchronous.  SIMPLYP_ERR_ARG (nothing launched) as for simplyp_predictive_bands, and for `which` outside {0, 1}, which = 1
 * with NULL err_m, NULL table.
 */
int simplyp_predictive_series(simplyp_ctx* ctx, const simplyp_dims* dims, uint32_t out_mask,
                              const int32_t* out_reaches, int32_t n_out_reaches,
                              const double* out, const int32_t* member_of_slot,
                              const double* f_tdp, const double* reach_params,
                              const int32_t* series /* host [n_series] */, int32_t n_series,
                              const double* err_m, uint64_t seed, int32_t day0, int32_t which, double* table);

/*
 * simplyp_predictive_bands -- the order statistics across the members, for every (series, day, output reach), of the series
 * simplyp_predictive_series(which = 0) would write: rank rule, NaN ordering and `include` exactly as simplyp_quantiles.  The
 * series are generated into a bounded workspace of the context by whole days (256 MiB at most, a day at least; the
 * environment variable SIMPLYP_PRED_CHUNK_DAYS sets the days per chunk) and each chunk is selected with simplyp_quantiles'
 * kernels; the include mask and the ranks are formed once per call.  The result does not depend on the chunk length, bit
 * for bit.  The run's table is only read.
 *   include         device  [E] uint8 in MEMBER order or NULL, as for simplyp_quantiles; no member left: every output NaN
 *   err_m           NULL = the parameter-only band of the series: no draws are made
 *   q, K            HOST    [K] probabilities in [0, 1], 1 <= K <= 16
 *   order_stats     device  [2][K][n_series][D][n_out_reaches]: plane 0 = x_(k_lo), plane 1 = x_(k_hi)
 *   info            host    may be NULL
 * Synchronous, on the context's stream.  SIMPLYP_ERR_ARG (nothing launched) for K outside 1..16, a q outside [0, 1] or NaN,
 * n_series outside 1..32, a series that is not in the mask, a derived series whose mask lacks Qr or a flux or with NULL
 * f_tdp / reach_params, day0 < 0, D < 0, NULL out / series / q / order_stats.
 */
int simplyp_predictive_bands(simplyp_ctx* ctx, const simplyp_dims* dims, uint32_t out_mask,
                             const int32_t* out_reaches, int32_t n_out_reaches,
                             const double* out, const int32_t* member_of_slot, const uint8_t* include,
                             const double* f_tdp, const double* reach_params,
                             const int32_t* series /* host [n_series] */, int32_t n_series,
                             const double* err_m, uint64_t seed, int32_t day0,
                             const double* q /* host [K] */, int32_t K,
                             double* order_stats, simplyp_pred_info* info);

/* ---- weighted bands: exact quantiles across the members under the particle filter's integer weights -- the forecast band of a
 * filter that does not resample every window, and the likelihood-weighted (GLUE) band of a Monte-Carlo ensemble.
 *
 * The rule, for one row over its member axis (simplyp_amd/csrc/simplyp_weighted.h and simplyp_amd/weighted.py state it too):
 * weights are the integers simplyp_pf_weights writes, q_i = floor(w_i 2^40), 0 <= q_i <= 2^40.  A member takes part iff its
 * include flag is set and q_i > 0; T is the sum of the participating weights (<= 2^62 with E <= 2^22).  The members are ordered
 * as simplyp_quantiles orders them (NaN after +inf; -0.0 and +0.0 equal), C_i is the inclusive running sum of the weights in
 * that order, and for a probability p the threshold is t = max(1, ceil(p T)), formed exactly (p = m 2^e, m < 2^53: m T fits
 * 128 bits).  The result is the value of the first member with C_i >= t: the order statistic of rank t - 1 (zero-based) of the
 * multiset in which member i occurs q_i times -- numpy's method='inverted_cdf' with weights=, NOT the 'linear' rule of the
 * unweighted entries: one value per probability, nothing to interpolate.  Everything is integer arithmetic, so every output is
 * an element of its row and every correct implementation returns the same one, bit for bit (which of -0.0 / +0.0 is free).
 * T == 0 (nobody takes part): every output is NaN and the call succeeds. ---------------------------------------------------- */
typedef struct {
    double   kernel_ms;    /* all launches of the call, HIP events on the context's stream                      */
    int64_t  bytes_table;  /* bytes of the rows selected from: n_rows * E * 8                                   */
    uint64_t T;            /* the sum of the participating weights                                              */
    int32_t  n_used;       /* members that took part: include set and weight > 0                                */
    int32_t  n_passes;     /* sweeps over a row the selection made (diagnostic)                                 */
} simplyp_wq_info;

/*
 * simplyp_weighted_quantiles -- the weighted twin of simplyp_quantiles: same tables, same member_of_slot / include.
 *   E, n_rows       1 <= E <= 2^22; n_rows == 0 succeeds and launches nothing
 *   weights         device  [E] uint64 in MEMBER order (looked up through member_of_slot like include), each <= 2^40
 *   q, K            HOST    [K] probabilities in [0, 1], 1 <= K <= 16
 *   order_stats     device  [K][n_rows]
 *   info            host    may be NULL
 * One launch forms the weights in column order, T, n_used and the count of weights above 2^40, read back once; then rows of
 * <= 2048 members are sorted in LDS as (key, weight) pairs and longer rows go through a radix select on weights.  Device
 * workspace is 8 E + 24 bytes.  Synchronous, on the context's stream.  SIMPLYP_ERR_ARG with nothing launched for E outside
 * 1..2^22, n_rows < 0, NULL table / weights / q / order_stats, K outside 1..16, a q outside [0, 1] or NaN; SIMPLYP_ERR_ARG with
 * order_stats unwritten for a weight above 2^40.
 */
int simplyp_weighted_quantiles(simplyp_ctx* ctx, int32_t E, int64_t n_rows, const double* table,
                               const int32_t* member_of_slot, const uint8_t* include,
                               const uint64_t* weights /* device [E], member order */,
                               const double* q /* host [K] */, int32_t K,
                               double* order_stats /* device [K][n_rows] */,
                               simplyp_wq_info* info);

/*
 * simplyp_predictive_bands_weighted -- simplyp_predictive_bands under weights: the same arguments, checks, generation kernel
 * and chunks (SIMPLYP_PRED_CHUNK_DAYS included); each chunk is selected with simplyp_weighted_quantiles' kernels, the weights
 * are prepared once per call, and the result does not depend on the chunk length, bit for bit.
 *   weights         device  [E] uint64 in MEMBER order, each <= 2^40
 *   order_stats     device  [K][n_series][D][n_out_reaches]
 * SIMPLYP_ERR_ARG as for simplyp_predictive_bands and simplyp_weighted_quantiles.
 */
int simplyp_predictive_bands_weighted(simplyp_ctx* ctx, const simplyp_dims* dims, uint32_t out_mask,
                                      const int32_t* out_reaches, int32_t n_out_reaches,
                                      const double* out, const int32_t* member_of_slot, const uint8_t* include,
                                      const double* f_tdp, const double* reach_params,
                                      const int32_t* series /* host [n_series] */, int32_t n_series,
                                      const double* err_m, uint64_t seed, int32_t day0,
                                      const double* q /* host [K] */, int32_t K,
                                      const uint64_t* weights /* device [E], member order */,
                                      double* order_stats, simplyp_wq_info* info);

/* ---- scores: an ensemble forecast judged against observations across the member axis -- the continuous ranked probability
 * score (CRPS) in its two terms, and the two counts the probability integral transform (PIT) is made of.
 *
 * The rule, for one row over its member axis (values x_j) and one observation y (simplyp_amd/csrc/simplyp_score.h and
 * simplyp_amd/score.py state it too).  Participation and order are simplyp_weighted_quantiles': member j takes part iff its
 * include flag is set and its integer weight q_j > 0; weights == NULL gives every included member q_j = 1 (the special case, not
 * a second code path); T is the sum of the participating weights; the key order has NaN after +inf, -0.0 and +0.0 equal.
 *   below       = sum q_j [x_j < y]   and   at_or_below = sum q_j [x_j <= y]: exact integers; a NaN member is above every y.
 *                 They are T F(y-) and T F(y) of the weighted empirical CDF whose inverse simplyp_weighted_quantiles returns.
 *   abs_err  A  = (1/T) sum q_j |x_j - y|
 *   spread   B  = (1/T^2) sum_k (x_(k+1) - x_(k)) C_k (T - C_k), x_(k) the participating values in key order, C_k the inclusive
 *                 running weight: half the expected distance of two draws, over the gaps, every term >= 0
 *   CRPS        = A - B = the integral of (F - 1{x >= y})^2: one subtraction, left to the caller
 * A row whose y is NaN is not scored: sums NaN, counts 0.  y = +-inf is an argument error.  A participating non-finite value
 * makes A and B of its row NaN; the counts stay exact.  T == 0: NaN and 0, and the call succeeds.
 * The counts are the same bits in every correct implementation.  A and B are sums of non-negative terms of at most 8 roundings
 * each, added as 1024 per-lane partials (at most 4096 terms each) and a fixed tree: within 1e-12 of their exact values, relative
 * to themselves (CRPS therefore within 1e-12 (A + B); it cancels, so never judge it relative to itself).  No floating-point
 * atomics: the same call twice gives the same bits, and a row's outputs depend neither on its place in the table nor on the
 * chunks. -------------------------------------------------------------------------------------------------------------------- */
typedef struct {
    double   kernel_ms;       /* all launches of the call, HIP events on the context's stream                     */
    double   gen_ms;          /* of which: generating the scored rows (simplyp_predictive_scores; else 0)         */
    double   sort_ms;         /* of which: sorting the rows for the spread term                                   */
    int64_t  bytes_read;      /* table bytes behind one pass over the scored rows                                 */
    int64_t  bytes_workspace; /* bytes of a chunk of rows in the context's workspace (<= 256 MiB, or one row)     */
    uint64_t T;               /* the sum of the participating weights                                             */
    int32_t  n_used;          /* members that took part: include set and weight > 0                               */
    int32_t  n_rows_scored;   /* rows with an observation                                                         */
    int32_t  n_chunks;        /* chunks of rows the workspace was filled with                                     */
    int32_t  reserved;        /* 0                                                                                */
} simplyp_score_info;

/*
 * simplyp_scores -- the scores of every row of a device table [n_rows][E] (any table whose last axis is the member axis).
 *   E, n_rows       1 <= E <= 2^22; n_rows == 0 succeeds and launches nothing
 *   member_of_slot, include, weights   as for simplyp_weighted_quantiles; weights may be NULL (all 1)
 *   y               HOST    [n_rows] observations, NaN = the row is not scored
 *   sums            device  [2][n_rows]: abs_err, spread
 *   counts          device  [2][n_rows] uint64: below, at_or_below
 *   info            host    may be NULL
 * Only rows with an observation are read.  Counts and A are one streaming pass per row; for B the row is sorted with its weights
 * -- tiles of 4096 (key, weight) pairs in LDS, then stable merge passes through the context's workspace -- and one pass forms
 * the running weight and the sum over the gaps.  Rows go through the workspace in chunks of at most 256 MiB (32 E bytes per row;
 * SIMPLYP_SCORE_CHUNK_ROWS in the environment asks for fewer rows per chunk, never more).  Synchronous, on the context's stream.  SIMPLYP_ERR_ARG
 * with nothing launched for E outside 1..2^22, n_rows < 0, NULL table / y / sums / counts, an infinite observation;
 * SIMPLYP_ERR_ARG with sums and counts unwritten for a weight above 2^40.  Without any observation no row kernel runs and no
 * row is read, but the call is not empty: the weights are still prepared and checked (a weight above 2^40 is refused whatever y
 * holds, and T and n_used are reported), and every output is filled as "not scored" -- NaN and 0 -- because the caller's sums
 * and counts must be defined when the call returns.
 */
int simplyp_scores(simplyp_ctx* ctx, int32_t E, int64_t n_rows, const double* table /* device [n_rows][E] */,
                   const int32_t* member_of_slot, const uint8_t* include,
                   const uint64_t* weights /* device [E], member order, or NULL */,
                   const double* y /* HOST [n_rows], NaN = not scored */,
                   double* sums /* device [2][n_rows]: abs_err, spread */,
                   uint64_t* counts /* device [2][n_rows]: below, at_or_below */,
                   simplyp_score_info* info);

/*
 * simplyp_predictive_scores -- the scores of the series simplyp_predictive_series (which = 0) would write, against observations
 * of every (series, day, reach): only the observed rows are generated -- by the same series resolver and the same Philox
 * counter (seed, member, day0 + d, reach, series) -- and scored by simplyp_scores' row kernels, chunk by chunk.  The result
 * equals simplyp_predictive_series followed by simplyp_scores on the observed rows, bit for bit, sums included.
 *   err_m           device  [n_series][E] member order, or NULL: the parameter-only forecast
 *   weights         device  [E] uint64 in MEMBER order, each <= 2^40, or NULL (all 1)
 *   obs             HOST    [n_series][D][n_out_reaches], NaN = no observation
 *   sums, counts    device  [2][n_series][D][n_out_reaches]
 * SIMPLYP_ERR_ARG as for simplyp_predictive_bands (series, mask, day0) and simplyp_scores.  D == 0 succeeds and launches nothing.
 */
int simplyp_predictive_scores(simplyp_ctx* ctx, const simplyp_dims* dims, uint32_t out_mask,
                              const int32_t* out_reaches, int32_t n_out_reaches,
                              const double* out, const int32_t* member_of_slot, const uint8_t* include,
                              const double* f_tdp, const double* reach_params,
                              const int32_t* series /* host [n_series] */, int32_t n_series,
                              const double* err_m, uint64_t seed, int32_t day0,
                              const uint64_t* weights /* device [E], member order, or NULL */,
                              const double* obs /* HOST [n_series][D][n_out_reaches] */,
                              double* sums, uint64_t* counts, simplyp_score_info* info);

/* ---- Pareto counts and non-dominated ranks: the members of an ensemble compared on several objectives at once.
 *
 * The rule (simplyp_amd/csrc/simplyp_pareto.h and simplyp_amd/pareto.py state it too).  obj[M][E] holds M objectives of the E
 * members, the member axis fastest and in the column order of the table it came from (member_of_slot and include as for
 * simplyp_quantiles); sense[m] = +1: larger is better, -1: smaller is better.
 *   A member takes part iff its include flag is set (include == NULL: every flag) and none of its M objectives is NaN.  +-inf
 *   are ordinary values; -0.0 and +0.0 are equal.  n = the members that take part.
 *   With y = sense x, a dominates b iff y_a[m] >= y_b[m] for every m and y_a[m] > y_b[m] for some m.  Members with identical
 *   objectives do not dominate each other.
 *   dominated_by[i] = the participants that dominate i;   dominates[i] = the participants i dominates
 *   rank[i]         = 0 when nobody dominates i, else 1 + the largest rank among its dominators: the length of the longest
 *                     chain of dominators above i = the index of the front i leaves with when the non-dominated members are
 *                     peeled off again and again (NSGA-II's non-dominated rank).  The Pareto front is rank == 0.
 *   A member that does not take part gets SIMPLYP_PARETO_EXCLUDED in all three outputs.  With max_fronts = F > 0 only the ranks
 *   0 .. F-1 are resolved: a deeper participant gets SIMPLYP_PARETO_UNRANKED as its rank, its two counts are still exact.
 * Only comparisons and integer counters: every correct implementation returns the same integers, in every run. ---------------- */
#define SIMPLYP_PARETO_MAX_OBJ   8
#define SIMPLYP_PARETO_EXCLUDED (-1)
#define SIMPLYP_PARETO_UNRANKED (-2)
typedef struct {
    double  kernel_ms;        /* all launches of the call, HIP events on the context's stream (the host's reads between them too) */
    int64_t pair_tests;       /* n^2 of the counts + (front x members left) of every front peeled                                  */
    int32_t n_used;           /* n: the members that took part                                                                    */
    int32_t n_fronts;         /* fronts resolved (<= max_fronts when that is set; 0 when rank == NULL)                            */
    int32_t n_front0;         /* members of rank 0 (0 when rank == NULL)                                                          */
    int32_t n_unranked;       /* participants left at SIMPLYP_PARETO_UNRANKED                                                     */
} simplyp_pareto_info;

/*
 * simplyp_pareto -- the three outputs above for a device table of objectives.
 *   E, M            1 <= E <= 2^24, 1 <= M <= SIMPLYP_PARETO_MAX_OBJ
 *   obj             device  [M][E] fp64, only read
 *   sense           HOST    [M], each +1 or -1
 *   member_of_slot  device  [E] or NULL: column j of obj holds member member_of_slot[j]
 *   include         device  [E] uint8 in member order, or NULL
 *   max_fronts      0 = every rank; F > 0 = the ranks 0 .. F-1
 *   dominated_by, dominates, rank   device [E] int32 in member order; any may be NULL, not all three.  rank == NULL: no peeling.
 *   info            host    may be NULL
 * Three small launches find the participants and write their keys (the order-preserving 64-bit key of simplyp_quantiles with the
 * sense folded in and the zeros made one), compacted in column order; n is read back once.  One all-pairs launch gives both
 * counts: a lane owns a member with its keys in registers, the other side of the pair comes through LDS tiles, and the grid's
 * splits of that side are combined with integer atomic adds.  The ranks are peeled front by front: one launch marks the members
 * nobody left dominates, a second takes the front's members off the counters of those that remain (front x remaining pair
 * tests, at most about n^2 / 2 over all fronts), and the host reads two integers per front to know when to stop -- a totally
 * ordered ensemble (M = 1 without ties) has n fronts and costs n such round trips; max_fronts bounds them.  The workspace is
 * grow-only context scratch of (8 M + 33) E bytes; no E x E array exists.  Synchronous, on the context's stream.
 * (SIMPLYP_PARETO_JLOAD=scalar in the environment makes the all-pairs launch read the other side from memory at wave-uniform
 * addresses instead of LDS tiles: a measurement switch of tools/time_pareto.py, 2.4 to 2.6 times slower, the same integers.)
 * SIMPLYP_ERR_ARG with nothing launched and nothing written for E or M out of range, a sense other than +-1, max_fronts < 0,
 * NULL obj or sense, or all three outputs NULL.  n == 0 succeeds: every output SIMPLYP_PARETO_EXCLUDED, n_fronts 0.
 */
int simplyp_pareto(simplyp_ctx* ctx, int32_t E, int32_t M, const double* obj /* device [M][E] */,
                   const int32_t* sense /* host [M] */, const int32_t* member_of_slot, const uint8_t* include,
                   int32_t max_fronts, int32_t* dominated_by, int32_t* dominates, int32_t* rank /* device [E], any may be NULL */,
                   simplyp_pareto_info* info);

/* ---- sampling the posterior: the affine-invariant ensemble sampler of the reference's calibration notebook
 * (Development/2016/MCMC.ipynb, cell 10: emcee.EnsembleSampler(n_walk, n_dim, log_posterior).run_mcmc(start, n_steps)), the stretch
 * move of Goodman & Weare (2010), with the walkers' positions, the model runs and the decisions all on the device.
 *
 * W walkers (W even, W >= 2 n_dim, 1 <= n_dim <= 16) in two halves of h = W / 2; positions theta [n_dim][W] and log posterior
 * lp [W] on the device.  Step t (absolute, counted from the start of the chain) moves half 0, then half 1; the active walkers of
 * half k are i in [k h, (k + 1) h), their partners come from the other half, offset c = (1 - k) h, at the positions it holds then.
 * One half-step is
 *     propose -> simplyp_run + simplyp_gof on the h run points (or the caller's own target) -> log_prob -> accept
 * The random stream is counter-based like the predictive stream's: Philox4x32-10 with key (seed & 0xffffffff, seed >> 32);
 *     draw A  counter (i, t, 0, 0x4D434D43):  u_z = uniform(x0, x1), partner j = c + (((uint64)x2 * h) >> 32)
 *     draw B  counter (i, t, 1, 0x4D434D43):  u_a = uniform(x0, x1)
 * with uniform(hi, lo) = ((((uint64)hi << 32) | lo) >> 12) + 0.5) 2^-52 in (0, 1).  Then
 *     s = (a - 1) u_z + 1,  z = (s s) / a                    emcee's g(z) on [1/a, a]
 *     y[d] = x_j[d] + z (x_i[d] - x_j[d])
 *     inside  = lo[d] <= y[d] < hi[d] for every d              the reference's log_prior; a NaN is outside
 *     run point = y where inside, else x_i                   the model never sees a point outside the box
 *     margin = (n_dim - 1) ln z + lp_y - lp[i] - ln u_a       accept iff inside, lp_y is not NaN and margin > 0
 * Everything but the two logarithms is integer arithmetic or + * / in fp64 without contraction: partner, z, y and inside are
 * the same bits on any implementation; simplyp_amd/mcmc.py restates the move in NumPy.  Neither the launch shape nor the time
 * enters.  All three entries are synchronous on the context's stream and return SIMPLYP_ERR_ARG with nothing launched for an odd
 * W or W < 2 n_dim, n_dim outside 1..16, half outside {0, 1}, a <= 1 or NaN, lo[d] >= hi[d] or a NaN bound, a target outside
 * [-2, SIMPLYP_NP_M), a NULL required pointer. ------------------------------------------------------------------------------ */
typedef struct {
    double  kernel_ms;     /* the entry's kernel, HIP events on the context's stream                                        */
    int32_t n_inside;      /* active walkers whose proposal lies inside the box (log_prob without `inside`: h)              */
    int32_t n_accepted;    /* accept: proposals taken; 0 from the other two entries                                         */
    int32_t n_nan;         /* log_prob, accept: proposals whose lp was NaN (log_prob turns them into -inf); 0 from propose  */
    int32_t reserved;
} simplyp_mcmc_info;

/*
 * simplyp_mcmc_propose -- the proposals of half `half` at step t, and the run points scattered into the arrays of the run.
 *   lo, hi          HOST    [n_dim] the prior box
 *   target          HOST    [n_dim] where dimension d's run point goes: 0 .. SIMPLYP_NP_M - 1 = that row of member_params,
 *                           -1 = f_tdp, -2 = nowhere (an error-model m, which no model input holds); a row or f_tdp at most once
 *   theta           device  [n_dim][W], only read
 *   prop            device  [n_dim][h]  y
 *   inside          device  [h] int32, 1 or 0
 *   member_params   device  [SIMPLYP_NP_M][h] of an ensemble of h members, or NULL when no target is >= 0; rows that no dimension
 *                           names are not touched
 *   f_tdp           device  [h], or NULL when no target is -1
 *   info            host    may be NULL
 */
int simplyp_mcmc_propose(simplyp_ctx* ctx, int32_t W, int32_t n_dim, int32_t half, double a, uint64_t seed, uint32_t t,
                         const double* lo /* host */, const double* hi /* host */, const int32_t* target /* host */,
                         const double* theta, double* prop, int32_t* inside, double* member_params, double* f_tdp,
                         simplyp_mcmc_info* info);

/*
 * simplyp_mcmc_log_prob -- the log posterior of the h run points from the table simplyp_gof left on the device: the sum over the
 * given (variable, output reach) pairs of the reference's Gaussian likelihood with sigma = m_v sim,
 *     -0.5 n ln(2 pi) - n ln(m_v) - SUM_LOG_SIM - SUM_RELSQ / (2 m_v m_v)
 * in that order of operations; the flat prior adds nothing inside the box.  -inf where `inside` is 0, where the member's status
 * carries SIMPLYP_STATUS_NONFINITE, where an m_v <= 0 and where the sum is NaN (a variable with 10 or fewer observations).
 *   gof             device  [SIMPLYP_N_GOF_STATS][SIMPLYP_N_GOF_VARS][n_out_reaches][h]
 *   status          device  [h] as written by simplyp_run, or NULL
 *   inside          device  [h] as written by the proposal, or NULL = all inside
 *   pair_var, pair_reach   HOST  [n_pairs], 1 <= n_pairs <= 32: SIMPLYP_GOF_v and the position among the output reaches
 *   m_dim           HOST    [SIMPLYP_N_GOF_VARS] the row of prop that holds the variable's m, or -1: m_const[v]
 *   m_const         HOST    [SIMPLYP_N_GOF_VARS]
 *   prop            device  [n_dim][h]
 *   lp_prop         device  [h]
 */
int simplyp_mcmc_log_prob(simplyp_ctx* ctx, int32_t W, int32_t n_dim, int32_t n_out_reaches, const double* gof,
                          const int32_t* status, const int32_t* inside,
                          const int32_t* pair_var /* host */, const int32_t* pair_reach /* host */, int32_t n_pairs,
                          const int32_t* m_dim /* host */, const double* m_const /* host */,
                          const double* prop, double* lp_prop, simplyp_mcmc_info* info);

/*
 * simplyp_mcmc_accept -- the decisions of half `half` at step t, in place.  z is recomputed from the counter; lp_prop is a plain
 * device array, so a caller may sample any target: propose, evaluate ln p at prop by its own means, accept.
 *   prop, inside    device  as written by the proposal of the same (half, t)
 *   lp_prop         device  [h] ln p of the proposals; -inf and NaN are refused
 *   theta, lp       device  [n_dim][W], [W]: the active half's accepted lanes are overwritten
 *   n_accept        device  [W] int32: + 1 where accepted
 *   chain_row       device  [n_dim + 1][W] or NULL: the active half's positions and lp after the decision; after half 1 of a
 *                           step every lane of the row has been written
 */
int simplyp_mcmc_accept(simplyp_ctx* ctx, int32_t W, int32_t n_dim, int32_t half, double a, uint64_t seed, uint32_t t,
                        const double* prop, const int32_t* inside, const double* lp_prop,
                        double* theta, double* lp, int32_t* n_accept, double* chain_row, simplyp_mcmc_info* info);

/* ---- finding the posterior mode: multi-start Nelder-Mead, the reference's find_map (Development/2016/MAP.ipynb:
 * scipy.optimize.fmin on the negative log posterior) for S simplexes at once, with the simplexes, the model runs and the decisions
 * on the device.
 *
 * S simplexes in n_dim dimensions (1 <= n_dim <= 16, N = n_dim): vertices sim [N + 1][n_dim][S] and their values fsim [N + 1][S],
 * f = -ln p, kept sorted by value; the box lo <= x < hi.  Every simplex owns four members of a run -- member index slot S + s --
 * and integer state istate [SIMPLYP_NM_N_ISTATE][S].  One run of all simplexes is
 *     propose -> simplyp_run + simplyp_gof + simplyp_mcmc_log_prob on the 4 S run points (or the caller's own target) -> update
 * In phase STEP the slots hold scipy's four candidates, with xbar = (sim[0] + ... + sim[N - 1]) / N summed in that order and w = sim[N]:
 *     xr = 2 xbar - w,  xe = 3 xbar - 2 w,  xc = 1.5 xbar - 0.5 w,  xcc = 0.5 xbar + 0.5 w        rho 1, chi 2, psi 0.5
 * and update walks scipy's decision tree (_minimize_neldermead, its < and <= as they are) on their four values: the lazy algorithm's
 * path.  The new vertex is inserted behind every vertex that is not worse.  A shrink, sim[j] = sim[0] + 0.5 (sim[j] - sim[0]) for
 * j >= 1, puts the simplex into phase EVAL: the slots hold up to four vertices without a value, from istate's cursor on, for as many
 * runs as that takes; then the vertices are sorted stably.  A fresh simplex starts in EVAL with cursor 0 and n_iter 0.
 * When an iteration is complete n_iter grows by one (the initial evaluation makes it 1, like scipy's nit) and the simplex ends if
 *     a vertex of the initial simplex has a value that is not finite                          status SIMPLYP_NM_NONFINITE_START
 *     n_iter >= max_iter                                                                      status SIMPLYP_NM_MAXITER (scipy's 2)
 *     max |sim[j] - sim[0]| <= xatol and max |fsim[0] - fsim[j]| <= fatol over j >= 1           status SIMPLYP_NM_CONVERGED (scipy's 0)
 * tested in that order.  A slot that is idle holds sim[0]; the run point of a slot that is idle or outside the box is sim[0]: the
 * model never sees a point outside the box.  Everything is + - * / and comparisons in fp64 without contraction, so any
 * implementation gives the same bits; simplyp_amd/neldermead.py restates it in NumPy.  Both entries are synchronous on the context's
 * stream and return SIMPLYP_ERR_ARG with nothing launched for S < 1 or S > 2^28, n_dim outside 1..16, lo[d] >= hi[d] or a NaN
 * bound, a target outside [-2, SIMPLYP_NP_M), max_iter < 1, a negative or NaN tolerance, history_rows < 0, a NULL required pointer. */
enum { SIMPLYP_NM_STEP = 0, SIMPLYP_NM_EVAL = 1, SIMPLYP_NM_DONE = 2 };                               /* istate row PHASE  */
enum { SIMPLYP_NM_RUNNING = -1, SIMPLYP_NM_CONVERGED = 0, SIMPLYP_NM_MAXITER = 2, SIMPLYP_NM_NONFINITE_START = 3 };  /* STATUS */
enum {
    SIMPLYP_NM_PHASE = 0,        /* rows of istate                                                                    */
    SIMPLYP_NM_CURSOR,           /* EVAL: the first vertex that has no value yet                                      */
    SIMPLYP_NM_N_ITER,
    SIMPLYP_NM_STATUS,
    SIMPLYP_NM_N_REFLECT,        /* how many iterations ended in each kind of move                                    */
    SIMPLYP_NM_N_EXPAND,
    SIMPLYP_NM_N_CONTRACT_OUT,
    SIMPLYP_NM_N_CONTRACT_IN,
    SIMPLYP_NM_N_SHRINK,
    SIMPLYP_NM_N_ISTATE
};

typedef struct {
    double  kernel_ms;           /* the entry's kernel, HIP events on the context's stream                              */
    int32_t n_active;            /* simplexes that are not DONE, in the state the entry leaves                          */
    int32_t n_converged;         /* ... DONE with status CONVERGED                                                      */
    int32_t n_shrinking;         /* ... in EVAL after a shrink                                                          */
    int32_t n_nonfinite_start;   /* ... DONE with status NONFINITE_START                                                */
    int32_t n_inside;            /* propose: slots that want a value and lie inside the box; 0 from update              */
    int32_t reserved;
} simplyp_nm_info;

/*
 * simplyp_nm_propose -- the points of the four slots of every simplex, and the run points scattered into the arrays of the run.
 *   lo, hi          HOST    [n_dim] the box
 *   target          HOST    [n_dim] as for simplyp_mcmc_propose: a row of member_params, -1 = f_tdp, -2 = nowhere
 *   sim, istate     device  only read
 *   prop            device  [n_dim][4 S] the slots' points
 *   inside          device  [4 S] int32: 1 where the slot wants a value and its point lies inside the box, else 0
 *   member_params   device  [SIMPLYP_NP_M][4 S] of an ensemble of 4 S members, or NULL when no target is >= 0; rows that no
 *                           dimension names are not touched
 *   f_tdp           device  [4 S], or NULL when no target is -1
 */
int simplyp_nm_propose(simplyp_ctx* ctx, int32_t S, int32_t n_dim,
                       const double* lo /* host */, const double* hi /* host */, const int32_t* target /* host */,
                       const double* sim, const int32_t* istate, double* prop, int32_t* inside,
                       double* member_params, double* f_tdp, simplyp_nm_info* info);

/*
 * simplyp_nm_update -- one run's values applied, in place.  lp_prop is a plain device array, so a caller may minimise any
 * function: propose, evaluate ln p = -f at the run points by its own means, update.
 *   prop, inside    device  as written by the proposal
 *   lp_prop         device  [4 S] ln p of the run points; f = -ln p, +inf where inside is 0 or ln p is NaN
 *   sim, fsim, istate       device  the state
 *   history         device  [history_rows][S] or NULL: row n_iter - 1 receives fsim[0] when an iteration is complete; rows past the
 *                           end are dropped
 */
int simplyp_nm_update(simplyp_ctx* ctx, int32_t S, int32_t n_dim, int32_t max_iter, double xatol, double fatol,
                      const double* prop, const int32_t* inside, const double* lp_prop,
                      double* sim, double* fsim, int32_t* istate, double* history, int32_t history_rows,
                      simplyp_nm_info* info);

/*
 * Sobol' sensitivity indices of an ensemble, bootstrapped on the device: which parameters matter for which output.  Saltelli's
 * design, the first- and total-order estimators of Saltelli et al. 2010 with the Sobol'-Levitan centring (what
 * scipy.stats.sobol_indices computes), and the bootstrap of both as resampling counts times per-sample terms.
 *
 * N base samples (2 <= N <= 32768), n_dim dimensions (1 <= n_dim <= 16) with a box lo < hi, E = N (n_dim + 2) members in
 * blocks of N: member j N + n is A_n for j = 0, B_n for j = 1, and A_n with dimension i taken from B_n for j = 2 + i.  The unit
 * points u[m][k][n], m = 0: A, 1: B, are the caller's or uniform(x0, x1) of Philox4x32-10 under key (seed & 0xffffffff,
 * seed >> 32) at counter (n, k, m, 0x53454E53); x = lo + (hi - lo) u.
 *
 * For a row f[E] of any table whose fastest axis is the member axis, sample n is valid iff none of its n_dim + 2 members carries
 * SIMPLYP_STATUS_NONFINITE.  With a, b, ab_i the row at A, B, AB_i minus mu = sum_valid (a + b) / (2 n_valid):
 *     p = a + b,  s = a a + b b,  g_i = b (ab_i - a),  t_i = (a - ab_i) (a - ab_i)
 * and for a weight vector c[N] (an invalid sample's terms and count are selected to 0, never multiplied by it)
 *     n_c = sum c v,  P = sum c p,  S = sum c s,  G_i = sum c g_i,  T_i = sum c t_i
 *     m1 = P / (2 n_c),  m2 = S / (2 n_c),  var = m2 - m1 m1,  S1_i = (G_i / n_c) / var,  ST_i = (0.5 (T_i / n_c)) / var
 * each + * / in fp64 in this order without contraction.  var = 0 (a constant row) gives what IEEE gives, NaN (scipy maps it to 0).
 * Resample 0 is c = 1, the point estimate; resample b >= 1 has c[n] = the number of j < N with idx(b, j) == n,
 * idx(b, j) = (x_{j & 3} N) >> 32 of Philox counter (b, j >> 2, 0, 0x424F4F54).  The sums are an fp64 matrix product of the
 * counts with the terms (v_mfma_f64_16x16x4_f64) added in one fixed order: the same call twice gives the same bits; the ratios
 * are bit for bit the formulas above applied to the sums.  simplyp_amd/sobol.py states all of it in NumPy.
 *
 * Both entries are synchronous on the context's stream and return SIMPLYP_ERR_ARG with nothing launched for N outside 2..32768,
 * n_dim outside 1..16, n_rows < 0, n_boot < 0 or > 2^20, lo[d] >= hi[d] or a NaN bound, a target outside [-2, SIMPLYP_NP_M), a
 * row named twice, a NULL required pointer.
 */
typedef struct {
    double  kernel_ms;           /* all of the entry's kernels, HIP events on the context's stream                      */
    double  counts_ms;           /* indices: validity, row means and the resampling counts                              */
    double  contract_ms;         /* indices: the contraction                                                            */
    int64_t flops;               /* indices: 2 (1 + n_boot) n_rows N (2 n_dim + 2), the contraction's useful fp64 operations */
    int64_t bytes_workspace;     /* indices: the context's workspace the call used                                      */
    int32_t n_valid;             /* indices: valid samples                                                              */
    int32_t n_resamples;         /* indices: 1 + n_boot                                                                 */
} simplyp_sobol_info;

/*
 * simplyp_sobol_design -- the design of N (n_dim + 2) members, one lane per member.
 *   lo, hi          HOST    [n_dim] the box
 *   target          HOST    [n_dim] as for simplyp_mcmc_propose: a row of member_params, -1 = f_tdp, -2 = nowhere
 *   unit            device  [2][n_dim][N] unit points in [0, 1) (a scrambled Sobol' sequence, say), or NULL: the Philox stream
 *   x               device  [n_dim][E] the design
 *   member_params   device  [SIMPLYP_NP_M][E], or NULL when no target is >= 0; rows that no dimension names are not touched
 *   f_tdp           device  [E], or NULL when no target is -1
 */
int simplyp_sobol_design(simplyp_ctx* ctx, int32_t N, int32_t n_dim, uint64_t seed,
                         const double* lo /* host */, const double* hi /* host */, const int32_t* target /* host */,
                         const double* unit, double* x, double* member_params, double* f_tdp, simplyp_sobol_info* info);

/*
 * simplyp_sobol_indices -- the indices of every row of a table, with n_boot bootstrap resamples.
 *   table           device  [n_rows][E], only read: period sums, a goodness-of-fit table, any table whose fastest axis is the
 *                           member axis.  n_rows = 0 succeeds and launches nothing.
 *   status          device  [E] int32 as simplyp_run writes it, or NULL: every sample is valid
 *   sums            device  [1 + n_boot][n_rows][2 n_dim + 2] in the order P, S, G_0.., T_0.., or NULL
 *   n_used          device  [1 + n_boot] int32 n_c, or NULL
 *   indices         device  [2][n_dim][n_rows][1 + n_boot]: plane 0 S1, plane 1 ST, the resample axis fastest -- the slice
 *                           [..., 1:] (made contiguous) is a table simplyp_quantiles takes for the percentile interval
 * The counts live in the context's grow-only workspace.
 */
int simplyp_sobol_indices(simplyp_ctx* ctx, int32_t N, int32_t n_dim, int32_t n_rows, const double* table, const int32_t* status,
                          int32_t n_boot, uint64_t seed, double* sums, int32_t* n_used, double* indices, simplyp_sobol_info* info);

/* ---- assimilating observations as they arrive: sequential importance resampling (a particle filter) over the joint (state,
 * parameter) space, on the device.  E particles, 1 <= E <= 2^22, each a member of the ensemble with its model state
 * (simplyp_set_state), its rows of member_params / reach_params / f_tdp, its position theta[n_dim] and its error-model m.  One
 * assimilation window is
 *     simplyp_run from the particles' states (state in, state out) -> pf_loglik -> pf_weights
 *     -> when the effective sample size sum_w^2 / sum_w2 is too small: pf_resample -> gather_members for every array a particle
 *        owns -> pf_jitter, the rejuvenation move (the model is deterministic: duplicates would stay identical for ever)
 * with nothing but the info structs crossing to the host.  simplyp_amd/particle.py states every rule below in NumPy and Python
 * integers.
 *
 * Likelihood.  For a pair (variable v, output reach r) take the days of the window with an observation, ascending; with sim the
 * df_R series as simplyp_time_quantiles computes it,
 *     n = their count,  SL = sum ln sim,  SR = sum (obs / sim - 1)^2
 *     term = -0.5 n ln(2 pi) - n ln(m) - SL - SR / (2 m m)                     in this order of operations
 * -- the reference's Gaussian likelihood with sigma = m sim as simplyp_mcmc_log_prob states it, without the more-than-10-
 * observations rule of simplyp_gof, so a window with two chemistry samples has a likelihood.  The increment is the sum of the
 * terms over the pairs in the given order, started from +0.0; a pair without an observation in the window adds nothing, so a
 * window without observations gives exactly +0.0.  The increment is -inf where the status carries SIMPLYP_STATUS_NONFINITE, where
 * an m <= 0 and where the sum is NaN (counted in n_nan) -- a NaN simulated value on an observation day among them: a particle may
 * not skip an observation.
 *
 * Weights.  lw_max is the largest finite entry of lw;  w = exp(lw - lw_max), selected to exactly 1 where lw == lw_max and to 0
 * where lw is -inf, +inf or NaN (the last two counted in n_nan);  q = (uint64) floor(w 2^40).  A particle more than 40 ln 2 = 27.7
 * below the maximum therefore has weight 0: the filter resolves weights to 2^-40.  T = sum q is a 64-bit integer, exact in any
 * order; sum_w and sum_w2 are added in one fixed order.  The caller forms ESS = sum_w^2 / sum_w2 and the log of the mean weight,
 * lw_max + ln(sum_w / E).  No finite entry: w = q = 0, T = 0, lw_max = -inf.
 *
 * Resampling is systematic and in integers only, so any implementation gives the same ancestors (the rules are the plain C++ of
 * simplyp_amd/csrc/simplyp_resample.h, which the kernel and a host program share):
 *     C_i = q_0 + ... + q_i (inclusive),  T = C_{E-1}
 *     x = (x0 << 32) | x1 of Philox4x32-10 under key (seed & 0xffffffff, seed >> 32) at counter (t, 0, 0, 0x50465253 "PFRS")
 *     r = the high 64 bits of x T, so 0 <= r < T
 *     the ancestor of particle k is the smallest i with E C_i > k T + r           both sides exact, below 2^85
 * The ancestors do not decrease with k, and particle i is taken floor(E q_i / T) or ceil(E q_i / T) times.  T = 0: the ancestors
 * are the identity, the offspring 0, n_unique = 0, and the call succeeds -- every particle is dead, which is the caller's to report.
 *
 * Rejuvenation.  y[d] = centre[d] + a (theta[d][k] - centre[d]) + scale[d] z, each + * in fp64 in this order without contraction,
 * z the standard normal of the predictive stream (simplyp_predictive_series) at counter (k, t, d, 0x50464A54 "PFJT").  The whole
 * particle keeps its position when any y[d] falls outside lo[d] <= y < hi[d] (counted in n_outside).  a = (3 delta - 1) /
 * (2 delta), centre = the mean and scale = sqrt(1 - a a) times the standard deviation of the resampled positions is the
 * kernel-shrinkage move of Liu & West (2001); a = 1 is plain jitter.
 *
 * All five entries are synchronous on the context's stream, keep their workspace in the context's grow-only scratch, and return
 * SIMPLYP_ERR_ARG with nothing launched for E outside 1..2^22, a NULL required pointer, n_pairs outside 1..32, a pair out of range,
 * n_dim outside 1..16, n_rows < 0, overlapping src and dst, lo[d] >= hi[d] or a NaN bound, a target outside [-2, SIMPLYP_NP_M) or
 * named twice, a non-finite a or centre, a scale that is negative or not finite.
 */
typedef struct {
    double   kernel_ms;    /* all of the entry's kernels, HIP events on the context's stream                                 */
    double   lw_max;       /* pf_weights: the largest finite log weight, -inf when there is none                             */
    double   sum_w;        /* pf_weights: sum of w                                                                            */
    double   sum_w2;       /* pf_weights: sum of w w                                                                          */
    uint64_t T;            /* pf_weights, pf_resample: sum of q                                                               */
    int32_t  n_alive;      /* pf_weights: particles with q > 0                                                                */
    int32_t  n_nan;        /* pf_loglik: increments that were NaN; pf_weights: log weights that were +inf or NaN              */
    int32_t  n_unique;     /* pf_resample: distinct ancestors                                                                 */
    int32_t  n_bad;        /* gather_members: ancestors outside [0, E)                                                        */
    int32_t  n_outside;    /* pf_jitter: particles that kept their position                                                   */
    int32_t  reserved;     /* fields an entry does not name are 0                                                             */
} simplyp_pf_info;

/*
 * simplyp_pf_loglik -- every particle's log-likelihood of a window's observations, from the daily table the window's simplyp_run
 * left on the device; one lane per particle.
 *   dims .. reach_params    as for simplyp_gof (out_mask must contain Qr and the three daily fluxes)
 *   obs             HOST    [n_out_reaches][SIMPLYP_N_GOF_VARS][D], NaN = no observation
 *   pair_var, pair_reach   HOST  [n_pairs], 1 <= n_pairs <= 32: SIMPLYP_GOF_v and the position among the output reaches
 *   err_m           device  [n_pairs][E] member order: the pair's m for every particle
 *   status          device  [E] as written by simplyp_run, or NULL
 *   lw              device  [E] member order: lw = accumulate ? lw + inc : inc
 *   inc             device  [E] member order, or NULL: the increment
 */
int simplyp_pf_loglik(simplyp_ctx* ctx, const simplyp_dims* dims, uint32_t out_mask,
                      const int32_t* out_reaches, int32_t n_out_reaches,
                      const double* out, const int32_t* member_of_slot,
                      const double* f_tdp, const double* reach_params, const double* obs /* host */,
                      const int32_t* pair_var /* host */, const int32_t* pair_reach /* host */, int32_t n_pairs,
                      const double* err_m, const int32_t* status, double* lw, double* inc, int32_t accumulate,
                      simplyp_pf_info* info);

/*
 * simplyp_pf_weights -- the normalised weights of lw [E]: w [E] fp64 and q [E] uint64, all three on the device; info carries
 * lw_max, sum_w, sum_w2, T, n_alive and n_nan.
 */
int simplyp_pf_weights(simplyp_ctx* ctx, int32_t E, const double* lw, double* w, uint64_t* q, simplyp_pf_info* info);

/*
 * simplyp_pf_resample -- the ancestors of assimilation step t (absolute: counted from the start of the filter) from q [E].
 *   ancestors       device  [E] int32, non-decreasing
 *   offspring       device  [E] int32, or NULL: how often each particle was taken
 * info carries T and n_unique.  The prefix sum is a device scan (wave64 cross-lane, block, block sums), the search a bisection per
 * particle on the 128-bit products.
 */
int simplyp_pf_resample(simplyp_ctx* ctx, int32_t E, const uint64_t* q, uint64_t seed, uint32_t t,
                        int32_t* ancestors, int32_t* offspring, simplyp_pf_info* info);

/*
 * simplyp_gather_members -- dst[row][k] = src[row][ancestors[k]] for a table [n_rows][E] of 8-byte words (moved as words: NaN
 * payloads survive): the model state (S * SIMPLYP_N_STATE rows), member_params, reach_params, f_tdp, the positions, err_m.
 * Out of place: overlapping src and dst are refused.  An ancestor outside [0, E) is never dereferenced; its destination words
 * become NaN and the case is counted in n_bad.  n_rows = 0 succeeds and launches nothing.
 */
int simplyp_gather_members(simplyp_ctx* ctx, int32_t E, int64_t n_rows, const int32_t* ancestors, const void* src, void* dst,
                           simplyp_pf_info* info);

/*
 * simplyp_pf_jitter -- the rejuvenation move of step t, in place on theta [n_dim][E], scattered into the run's arrays.
 *   centre, scale, lo, hi   HOST  [n_dim]
 *   target          HOST    [n_dim] as for simplyp_mcmc_propose: a row of member_params, -1 = f_tdp, -2 = nowhere
 *   member_params   device  [SIMPLYP_NP_M][E], or NULL when no target is >= 0; rows that no dimension names are not touched
 *   f_tdp           device  [E], or NULL when no target is -1
 */
int simplyp_pf_jitter(simplyp_ctx* ctx, int32_t E, int32_t n_dim, uint64_t seed, uint32_t t, double a,
                      const double* centre /* host */, const double* scale /* host */,
                      const double* lo /* host */, const double* hi /* host */, const int32_t* target /* host */,
                      double* theta, double* member_params, double* f_tdp, simplyp_pf_info* info);

/*
 * simplyp_eval_units -- the path's scalar device functions on caller-given arguments, one thread per row: how the tests pin the
 * DEVICE restatements of f_x (model.py:23-37) and discretized_soilP (model.py:39-56 followed by the >= 0 clamps of :696-699 and
 * conc_TDPs = TDPs / Vs of :702-703) to vectors the unmodified reference functions produced (tests/golden/unit_vectors.npz).
 *   which = 0   in  device [n][2]  = x, threshold (reld = 0.01)
 *               out device [n][2]  = f_x as the end-of-day flows evaluate it, f_x as the right-hand side's fused form does
 *   which = 1   in  device [n][10] = P_netInput, A_catch, Kf, Msoil, EPC0, Qs, Qq, Vs, TDPs, Plab
 *               out device [n][3]  = TDPs, Plab (clamped at 0 like :696-697), conc_TDPs
 * and the fp64 elementary functions every kernel of the library calls (the same inline functions, not copies), whose contract
 * is < 1 ulp for finite arguments in range (exp: |x| <= 700; log, reciprocal: normal x > 0 resp. x != 0):
 *   which = 2   in  device [n][1]  = x
 *               out device [n][4]  = exp(x) evaluated alone; in slot 1 of a group of two; in slot 0 and in slot 6 of a group of
 *                                    seven, the other slots holding other rows' arguments: four columns that are bit-identical
 *   which = 3   in  device [n][1]  = x            out device [n][1] = log(x)
 *   which = 4   in  device [n][1]  = x            out device [n][3] = the raw hardware reciprocal, one Newton step, two steps
 *   which = 5   in  device [n][2]  = q, b         out device [n][1] = q**b as the right-hand side forms it, exp(b log(q))
 * and the device's four statements of the model's right-hand side and the pieces of the step rule (again the inline functions the
 * time-stepping kernels call), so that each can be held to a plain statement of the equations point by point:
 *   which = 6   in  device [n][51] = the carried states VsA VsS Vg Vr Qr Msus TDPr PPr, then the 43 parameters of the reference's
 *                                    ode_f in the order of tests/golden/unit_vectors.npz 'ode_p_names' (NC_type as 0 / 1 / 2)
 *               out device [n][77] = the literal form: dy[8], q[4] (the daily integrands Qr, Msus Qr/Vr, TDPr Qr/Vr, PPr Qr/Vr);
 *                                    the augmented form: dz[11] (VsA VsS Vg Qr Msus TDPr PPr, exp(-mu VsA), exp(-mu VsS),
 *                                    cQ Qr**b_Q, Qr**k_M), q[4] and the four auxiliary states it was given, formed as a run forms
 *                                    them before a day; the four-lane form: each lane's d[3] and integrand (16 values), then
 *                                    the augmented form on the auxiliary states those lanes formed: dz[11], q[4]; the fp32 form on
 *                                    constants and states rounded to float: dz[11], q[4], widened.  The day constants are
 *                                    assembled by the functions a run assembles them with.  Four lanes per row.
 *   which = 7   in  device [n][19] = the opening step's h_carry, T, rate; the proposal's h, rem, 1.1; the pair choice's hh, rate,
 *                                    kneeish, last_chance, alive; the damping weight's b_Q, Qr, dQr/dt, rate, T, what is left of
 *                                    the day; the step factor's err, stiff -- flags as 0 / 1
 *               out device [n][11] = the opening step of integrator 2, of integrator 2 with the second pair, of integrator 1, of
 *                                    integrator 3 (fp32); the proposed step; hh after the pair choice, the tableau's row offset,
 *                                    the returned flag; the damping factor F; the step-size factor without and with the second
 *                                    pair (fp32, widened)
 * Any other value of `which` is SIMPLYP_ERR_ARG.
 * Synchronous.  Not on the hot path.
 */
int simplyp_eval_units(simplyp_ctx* ctx, int32_t which, int32_t n, const double* in, double* out);

/*
 * simplyp_order_members -- the members' lane-slot order of a balanced run (opts.balance) from a caller-given cost table, without
 * the run around it: how the tests pin the device's ordering kernels and the host rule they restate to one statement of what a
 * correct order is.  Blocks of the total-cost order (cost summed over the windows mod 2^32, descending, the member id breaking
 * ties), nb1 = clamp(E / 256, 1, 24) of them with borders at E b / nb1; inside a block nb2 = clamp(E / (256 nb1), 1, 6)
 * sub-blocks by the 2nd principal component of the standardised log2(cost + 1) table, the 3rd inside a sub-block, the directions
 * alternating.
 *   E               members, >= 1; where = 0 takes at most 196608 (24 blocks of one 8192-key LDS sort)
 *   cost            device  [8][E] uint32: what a pilot would have counted in each of its 8 windows
 *   where           0 = the kernels a balanced run launches (the same launch sequence, on a workspace of this entry's own that
 *                   only grows), 1 = the host rule on a copy of `cost` (what SIMPLYP_ORDER_HOST=1 and larger ensembles use)
 *   perm            device  [E] int32: the member of each lane slot
 *   diag            device  [68] doubles, or NULL: mean[8] and 1 / deviation[8] of the log costs per window, the 36 covariances
 *                   of the standardised windows (i <= j, row by row), the eigenvectors v2[8], v3[8] of the 2nd and 3rd largest
 *                   eigenvalue as the projection uses them (fp32, widened)
 *   keys            device  [E] uint64, or NULL; where = 0 only: the sorted total-cost keys
 *                   (0xFFFFFFFF - total) << 32 | member, without the all-ones pads that sort behind them
 * Any other `where`, where = 0 above the limit, keys with where = 1, E < 1 and a NULL cost or perm are SIMPLYP_ERR_ARG.
 * Synchronous.  Not on the hot path.
 */
int simplyp_order_members(simplyp_ctx* ctx, int32_t E, const uint32_t* cost, int32_t where, int32_t* perm, double* diag,
                          uint64_t* keys);

#ifdef __cplusplus
}
#endif
#endif /* SIMPLYP_H */
