/*
 * simplyp_oracle.c -- TEST INFRASTRUCTURE ONLY.  Not part of the product.
 *
 * A scalar fp64 CPU restatement of the reference's time-stepping path
 * (/root/reference/Current_Release/v0-2A/simplyP/model.py), written formula by formula in
 * the reference's own order, so that the HIP kernel can be checked against it on a machine
 * where the Python reference does not exist.  Only tests/, __graft_entry__.smoke() and
 * bench.py's cpu_baseline leg may load this; the product path never does.
 *
 * Pinning (tests/test_oracle_*.py, fixtures in tests/golden/ made by make_golden.py from the
 * unmodified reference):
 *   - oracle_fx / oracle_soilp / oracle_ode_f  ==  reference f_x / discretized_soilP / ode_f
 *     on the committed in/out vectors (1e-13 rel);
 *   - the full driver with a converged integrator == reference run_simply_p with
 *     odeint(rtol=atol=1e-12) on 4 scenarios (tolerance stated in the tests).
 * The integrator itself is NOT the reference's: the reference calls SciPy odeint = ODEPACK
 * LSODA (scipy is un-vendored; reference pins scipy 1.2.0 in README.md:39, 1.15.3 here) at
 * rtol=0.01 (model.py:640).  LSODA's step/order heuristics are not restated; the oracle
 * integrates the same right-hand side with the schemes the device kernel implements: classical RK4,
 * Cash-Karp 5(4) on the literal system, Cash-Karp on the augmented transcendental-free form described
 * at ode_aug (with the second pair of opts.stiff_pair), and that scheme's fp32-stage mirror (config C5).
 * For the LSODA-at-rtol=0.01 trajectory itself: parity unpinned (the reference's own shipped CSVs pin it
 * only to ~3e-3).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#include "../include/simplyp.h"
#include "../include/simplyp_controller.h"    /* the step controller's constants, shared with the device kernels */

/* ------------------------------------------------------------------------------------- */
/* f_x, model.py:23-37.  threshold == 0 gives d == 0: the reference then divides 0/0 on the
 * single point x == 0; defined here (and in the kernel) as a plain step.                  */
static double f_x(double x, double threshold, double reld)
{
    double d = threshold * reld;
    if (x < threshold) return 0.0;
    if (x > threshold + d) return 1.0;
    if (d == 0.0) return 0.0;            /* x == threshold == 0 */
    double s = (x - threshold) / d;
    return -2.0 * s * s * s + 3.0 * s * s;                      /* :33 */
}

/* discretized_soilP, model.py:39-56 */
static void discretized_soilP(double P_netInput, double A_catch, double Kf, double Msoil, double EPC0,
                              double Qs, double Qq, double Vs, double TDPs, double Plab,
                              double* TDPs_out, double* Plab_out)
{
    double a = P_netInput * A_catch * 100.0 / 365. + Kf * Msoil * EPC0;          /* :42 */
    double b = (Kf * Msoil + Qs + Qq) / Vs;                                      /* :43 */
    TDPs = a / b + (TDPs - a / b) * exp(-b);                                     /* :44 */
    double b0 = b * Vs;                                                          /* :47 */
    double sorp;
    if (Vs > 0)                                                                  /* :50 */
        sorp = Kf * Msoil * (a / b0 - EPC0 + (1 / b) * (TDPs / Vs - a / b0) * (1 - exp(-b)));   /* :51 */
    else
        sorp = 0.;
    *TDPs_out = TDPs;
    *Plab_out = Plab + sorp;                                                     /* :54 */
}

/* Everything ode_f unpacks from its 41-tuple (model.py:74-78) that it actually uses. */
typedef struct {
    double P, E, mu, Qq_i, Qr_US_i, Esus_A, Esus_S, Esus_IG, Msus_US_i, TDPr_US_i, PPr_US_i;
    double f_A, f_Ar, f_IG, f_S, f_NC_A, f_NC_Ar, f_NC_IG, f_NC_S;
    int    NC_type;          /* 0 'None', 1 'A', 2 'S' */
    double f_quick, alpha, beta, T_s_A, T_s_S, T_g, fc, L_reach, A_catch, a_Q, b_Q, k_M;
    double conc_TDPs_A, conc_TDPs_NC, PlabA_i, PlabNC_i, Msoil, TDPeff, TDPg, E_PP, P_inactive, Qg_min;
} ode_params;

/* ode_f, model.py:58-187.  y and dy have the reference's 12 slots. */
static void ode_f(const double* y, const ode_params* p, double* dy)
{
    double VsA_i = y[0], VsS_i = y[1], Vg_i = y[2], Vr_i = y[3], Qr_i = y[4];
    double Msus_i = y[6], TDPr_i = y[8], PPr_i = y[10];

    double QsA_i = (VsA_i - p->fc) * f_x(VsA_i, p->fc, 0.01) / p->T_s_A;                         /* :105 */
    double dVsA_dt = p->P * (1 - p->f_quick) - p->alpha * p->E * (1 - exp(-p->mu * VsA_i)) - QsA_i;  /* :106 */
    double QsS_i = (VsS_i - p->fc) * f_x(VsS_i, p->fc, 0.01) / p->T_s_S;                         /* :109 */
    double dVsS_dt = p->P * (1 - p->f_quick) - p->alpha * p->E * (1 - exp(-p->mu * VsS_i)) - QsS_i;  /* :110 */

    double QsNC_i = (p->NC_type == 1) ? QsA_i : QsS_i;                                           /* :113-118 */

    double f_Qg = f_x(Vg_i / p->T_g, p->Qg_min, 0.01);                                           /* :121 */
    double Qg_i = (1 - f_Qg) * p->Qg_min + f_Qg * (Vg_i / p->T_g);                               /* :122 */
    double dVg_dt = p->beta * (p->f_A * QsA_i + p->f_S * QsS_i) - Qg_i;                          /* :124 */

    double inflow = p->Qq_i + (1 - p->beta) * (p->f_A * QsA_i + p->f_S * QsS_i) + Qg_i + p->Qr_US_i - Qr_i;
    double dQr_dt = inflow * p->a_Q * pow(Qr_i, p->b_Q) * (8.64 * 10000) / ((1 - p->b_Q) * (p->L_reach));  /* :127-130 */
    double dVr_dt = inflow;                                                                      /* :131 */
    double dQr_av_dt = Qr_i;                                                                     /* :132 */

    double QrkM = pow(Qr_i, p->k_M);
    double Msus_in_A = p->Esus_A * QrkM, Msus_in_S = p->Esus_S * QrkM, Msus_in_IG = p->Esus_IG * QrkM;  /* :138 */
    double dMsus_dt = p->f_Ar * Msus_in_A + p->f_IG * Msus_in_IG + p->f_S * Msus_in_S
                      + p->Msus_US_i - (Msus_i / Vr_i) * Qr_i;                                   /* :141-145 */
    double dMsus_out_dt = (Msus_i / Vr_i) * Qr_i;                                                /* :147 */

    double dTDPr_dt = ((1 - p->beta) *
                       (p->f_A * (1 - p->f_NC_A) * QsA_i * (p->conc_TDPs_A)
                        + p->f_A * p->f_NC_A * QsNC_i * (p->conc_TDPs_NC)
                        + p->f_S * p->f_NC_S * QsNC_i * (p->conc_TDPs_NC))
                       + p->f_A * (1 - p->f_NC_A) * p->Qq_i * (p->conc_TDPs_A)
                       + p->f_A * p->f_NC_A * p->Qq_i * (p->conc_TDPs_NC)
                       + p->f_S * p->f_NC_S * p->Qq_i * (p->conc_TDPs_NC)
                       + Qg_i * (p->TDPg * p->A_catch)
                       + p->TDPeff
                       + p->TDPr_US_i
                       - Qr_i * (TDPr_i / Vr_i));                                                /* :154-166 */
    double dTDPr_out_dt = Qr_i * (TDPr_i / Vr_i);                                                /* :168 */

    double dPPr_dt = (p->E_PP * (p->f_Ar * (1 - p->f_NC_Ar) * Msus_in_A * (p->PlabA_i + p->P_inactive) / p->Msoil
                                 + p->f_IG * (1 - p->f_NC_IG) * Msus_in_IG * (p->PlabA_i + p->P_inactive) / p->Msoil
                                 + p->f_S * (1 - p->f_NC_S) * Msus_in_S * p->P_inactive / p->Msoil
                                 + p->f_Ar * p->f_NC_Ar * Msus_in_A * (p->PlabNC_i + p->P_inactive) / p->Msoil
                                 + p->f_IG * p->f_NC_IG * Msus_in_IG * (p->PlabNC_i + p->P_inactive) / p->Msoil
                                 + p->f_S * p->f_NC_S * Msus_in_S * (p->PlabNC_i + p->P_inactive) / p->Msoil)
                      + p->PPr_US_i
                      - Qr_i * (PPr_i / Vr_i));                                                  /* :171-178 */
    double dPPr_out_dt = Qr_i * PPr_i / Vr_i;                                                    /* :180 */

    dy[0] = dVsA_dt; dy[1] = dVsS_dt; dy[2] = dVg_dt; dy[3] = dVr_dt; dy[4] = dQr_dt; dy[5] = dQr_av_dt;
    dy[6] = dMsus_dt; dy[7] = dMsus_out_dt; dy[8] = dTDPr_dt; dy[9] = dTDPr_out_dt; dy[10] = dPPr_dt;
    dy[11] = dPPr_out_dt;                                                                        /* :184-185 */
}

/* ------------------------------------------------------------------------------------- */
/* Integrators over [0, T] for the autonomous 12-system.                                  */

#define NY 12

typedef struct { uint64_t rhs, steps, rejected; int capped, poisoned; } integ_stats;

static void rk4_day(double* y, const ode_params* p, double T, int n, integ_stats* st)
{
    double h = T / n, k1[NY], k2[NY], k3[NY], k4[NY], yt[NY];
    for (int s = 0; s < n; ++s) {
        ode_f(y, p, k1);
        for (int i = 0; i < NY; ++i) yt[i] = y[i] + 0.5 * h * k1[i];
        ode_f(yt, p, k2);
        for (int i = 0; i < NY; ++i) yt[i] = y[i] + 0.5 * h * k2[i];
        ode_f(yt, p, k3);
        for (int i = 0; i < NY; ++i) yt[i] = y[i] + h * k3[i];
        ode_f(yt, p, k4);
        for (int i = 0; i < NY; ++i) y[i] += h * (1.0 / 6.0) * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]);
    }
    st->rhs += 4u * (uint64_t)n; st->steps += (uint64_t)n;
}

/* An explicit embedded Runge-Kutta pair of six stages as data.  Cash-Karp 5(4) (Cash & Karp, ACM TOMS 16 (1990) 201-222) is what
 * cashkarp_day, erk_aug_day and the fp32 mirror step with; TAB_STIFF (below) is the second pair of opts.stiff_pair. */
#define ERK_STAGES 6
typedef struct {
    double A[ERK_STAGES][ERK_STAGES - 1];
    double B[ERK_STAGES], E[ERK_STAGES];      /* weights of the higher-order solution; b - bhat */
    double err_exp;                  /* step-size factor = SAFETY * err^err_exp: -1/5 for Cash-Karp, SIMPLYP_STIFF_ERR_EXP for the second pair */
} erk_tableau;

static const erk_tableau TAB_CASHKARP = {
    {{0}, {1.0 / 5}, {3.0 / 40, 9.0 / 40}, {3.0 / 10, -9.0 / 10, 6.0 / 5}, {-11.0 / 54, 5.0 / 2, -70.0 / 27, 35.0 / 27},
     {1631.0 / 55296, 175.0 / 512, 575.0 / 13824, 44275.0 / 110592, 253.0 / 4096}},
    {37.0 / 378, 0, 250.0 / 621, 125.0 / 594, 0, 512.0 / 1771},
    {37.0 / 378 - 2825.0 / 27648, 0, 250.0 / 621 - 18575.0 / 48384, 125.0 / 594 - 13525.0 / 55296, -277.0 / 14336, 512.0 / 1771 - 1.0 / 4},
    -0.2};

static int state_finite(const double* y)
{   /* the 8 carried states (slots 0-4, 6, 8, 10) */
    static const int idx[8] = {0, 1, 2, 3, 4, 6, 8, 10};
    for (int i = 0; i < 8; ++i) if (!(fabs(y[idx[i]]) < 1.0e300)) return 0;
    return 1;
}

/*
 * Adaptive step control -- the exact rule the device kernel implements (ck_day in
 * simplyp_amd/csrc/simplyp_kernels.hip.h):
 *   a day whose start state is non-finite is not integrated (member poisoned);
 *   trial step hh = h, except  rem <= 1.1 h -> hh = rem;  rem < 2 h -> hh = rem/2   (rem = T - t);
 *   the max_steps-th attempt of a day takes hh = rem and is accepted whatever its error (STEPCAP);
 *   err = max_i |hh e_i| / (atol + rtol * max(|y_i|, |y_i + hh k1_i|)) over all 12 components (Euler predictor in the
 *   scale; the four daily integrals use their new value);
 *   a non-finite trial is rejected with factor 0.2; at hh <= 1e-9 T (or on the last attempt) the
 *   member is poisoned (state := NaN) instead;
 *   accept iff err <= 1;  h <- hh * clamp(0.9 * err^(-1/5), 0.2, 5)   (err == 0 -> 5);
 *   *h_carry (the controller's h) persists from day to day.
 */
static void cashkarp_day(double* y, const ode_params* p, double T, double rtol, double atol,
                         int max_steps, double* h_carry, integ_stats* st)
{
    double k[6][NY], yt[NY], yn[NY];
    double t = 0.0, h = *h_carry;
    int attempts = 0;
    if (!(h > 0.0) || h > T) h = T;
    if (!state_finite(y)) { y[5] = y[7] = y[9] = y[11] = NAN; st->poisoned = 1; return; }
    while (t < T) {
        double rem = T - t, hh = h;
        if (rem <= 1.1 * h) hh = rem; else if (rem < 2.0 * h) hh = 0.5 * rem;
        int last_chance = (attempts + 1 >= max_steps);
        if (last_chance) hh = rem;
        ode_f(y, p, k[0]);
        for (int s = 1; s < 6; ++s) {
            for (int i = 0; i < NY; ++i) {
                double acc = 0.0;
                for (int j = 0; j < s; ++j) acc += TAB_CASHKARP.A[s][j] * k[j][i];
                yt[i] = y[i] + hh * acc;
            }
            ode_f(yt, p, k[s]);
        }
        st->rhs += 6;
        double err = 0.0; int bad = 0;
        for (int i = 0; i < NY; ++i) {
            double inc = 0.0, ee = 0.0;
            for (int s = 0; s < 6; ++s) { inc += TAB_CASHKARP.B[s] * k[s][i]; ee += TAB_CASHKARP.E[s] * k[s][i]; }
            yn[i] = y[i] + hh * inc;
            /* scale: the state and its Euler predictor (the kernel forms the 5th-order increment only for accepted steps);
             * the four daily integrals (5, 7, 9, 11), accumulated outside the stages there, use their new value */
            const int is_quad = (i == 5 || i == 7 || i == 9 || i == 11);
            double sc = atol + rtol * fmax(fabs(y[i]), is_quad ? fabs(yn[i]) : fabs(y[i] + hh * k[0][i]));
            double r = fabs(hh * ee) / sc;
            if (r > err) err = r;                 /* NaN terms drop out, like v_max_f64 */
        }
        if (!(err < 1.0e300) || !state_finite(yn)) bad = 1;
        ++attempts;
        if (last_chance) st->capped = 1;
        if (bad && (last_chance || hh <= 1.0e-9 * T)) {
            for (int i = 0; i < NY; ++i) y[i] = NAN;
            st->poisoned = 1;
            break;
        } else if (!bad && (err <= 1.0 || last_chance)) {
            memcpy(y, yn, sizeof(yn));
            t = (hh == rem) ? T : t + hh;
            st->steps++;
        } else {
            st->rejected++;
        }
        double fac;
        if (bad) fac = SIMPLYP_CTRL_FAC_MIN;
        else if (err == 0.0) fac = SIMPLYP_CTRL_FAC_MAX;
        else { fac = SIMPLYP_CTRL_SAFETY * pow(err, -0.2); if (fac < SIMPLYP_CTRL_FAC_MIN) fac = SIMPLYP_CTRL_FAC_MIN; if (fac > SIMPLYP_CTRL_FAC_MAX) fac = SIMPLYP_CTRL_FAC_MAX; }
        h = hh * fac;
    }
    *h_carry = h;
}

/* ------------------------------------------------------------------------------------- */
/*
 * SIMPLYP_INTEG_CASHKARP_AUG -- Cash-Karp on an augmented, transcendental-free form of the same system.
 *
 * ode_f spends almost all of its arithmetic on exp(-mu*Vs) (x2, :106,:110) and Qr**b_Q, Qr**k_M (:130,:138).
 * Each of those is a smooth function of a state variable, so it obeys an ODE that is an exact consequence
 * of the reference's equations:
 *     EA = exp(-mu VsA)   ->  dEA/dt = -mu EA dVsA/dt        (same for ES)
 *     pb = Qr**b_Q        ->  dpb/dt = b_Q pb (dQr/dt) / Qr   (same for pk = Qr**k_M)
 * and Vr is not a free variable at all: (:127-131) and Vr0 (:457-459) give Vr == L Qr**(1-b_Q) / (a_Q 86400),
 * i.e. Qr/Vr = pb a_Q 86400 / L.  Carrying EA, ES, pb, pk as four extra Runge-Kutta states (re-evaluated
 * exactly from VsA, VsS, Qr at the start of every day, pb and pk also after every 8th attempted step within a day,
 * so they cannot drift) leaves a right-hand side of
 * ~70 multiply-adds and one reciprocal.  The solution is the same function of time; the truncation error
 * is of the same order and is held by the same error controller; its norm runs over the 7 physical states
 * (the auxiliary states are functions of them, the 4 daily integrals are quadratures of them: including those
 * 8 components costs 8 % more steps and buys no accuracy on any output, measured on the 30-year series and on
 * the Monte-Carlo members).  State vector z: VsA VsS Vg Qr Msus TDPr PPr EA ES pb pk | Qr_av Msus_out TDP_out PP_out.
 */
#define NZ 15
/* the controller's constants: include/simplyp_controller.h, the same macros the kernels' SysAug::* are defined from */
#define AUG_RESYNC SIMPLYP_CTRL_RESYNC_EVERY
#define AUG_NERR SIMPLYP_CTRL_N_ERR
#define AUG_AUX_WEIGHT SIMPLYP_CTRL_AUX_WEIGHT       /* SysAug::AUX_WEIGHT */
#define AUG_KINK_SOIL SIMPLYP_CTRL_KINK_SOIL         /* SysAug::KINK_SOIL: a step across a knee of a soil-water gate */
#define AUG_KINK_REACH SIMPLYP_CTRL_KINK_REACH       /* SysAug::KINK_REACH: the end of the step is looked for this far along the first slope */
#define AUG_KNEE_LO SIMPLYP_CTRL_KNEE_LO             /* SysAug::KNEE_LO, KNEE_HI, KNEE_OVER: a knee between 2 % and 90 % of the step, along the */
#define AUG_KNEE_HI SIMPLYP_CTRL_KNEE_HI             /* first slope, ends the step 5 % past the knee (no inflation for such a step)            */
#define AUG_KNEE_OVER SIMPLYP_CTRL_KNEE_OVER
#define AUG_DAY_START SIMPLYP_CTRL_DAY_START         /* SysAug::DAY_START: share of the carried step size a new day starts with */
#define AUG_KNEE_GW SIMPLYP_CTRL_KNEE_GW             /* SysAug::KNEE_GW: a step aimed at a knee of the groundwater gate keeps this factor */
#define AUG_KINK_GW SIMPLYP_CTRL_KINK_GW             /* SysAug::KINK_GW: across a knee of the groundwater gate (zone 1 % of Qg_min wide) */
static void ode_aug(const double* z, const ode_params* p, double invKv, double* dz)
{
    double VsA = z[0], VsS = z[1], Vg = z[2], Qr = z[3], Msus = z[4], TDPr = z[5], PPr = z[6];
    double EA = z[7], ES = z[8], pb = z[9], pk = z[10];
    double QsA = (VsA - p->fc) * f_x(VsA, p->fc, 0.01) / p->T_s_A;                              /* :105 */
    double dVsA = p->P * (1 - p->f_quick) - p->alpha * p->E * (1 - EA) - QsA;                   /* :106 */
    double QsS = (VsS - p->fc) * f_x(VsS, p->fc, 0.01) / p->T_s_S;                              /* :109 */
    double dVsS = p->P * (1 - p->f_quick) - p->alpha * p->E * (1 - ES) - QsS;                   /* :110 */
    double QsNC = (p->NC_type == 1) ? QsA : QsS;
    double f_Qg = f_x(Vg / p->T_g, p->Qg_min, 0.01);
    double Qg = (1 - f_Qg) * p->Qg_min + f_Qg * (Vg / p->T_g);                                  /* :121-122 */
    double dVg = p->beta * (p->f_A * QsA + p->f_S * QsS) - Qg;                                  /* :124 */
    double inflow = p->Qq_i + (1 - p->beta) * (p->f_A * QsA + p->f_S * QsS) + Qg + p->Qr_US_i - Qr;
    double dQr = inflow * p->a_Q * pb * (8.64 * 10000) / ((1 - p->b_Q) * (p->L_reach));         /* :127-130 */
    double kap = pb * invKv;                                                                    /* Qr / Vr */
    double MA = p->Esus_A * pk, MS = p->Esus_S * pk, MIG = p->Esus_IG * pk;                     /* :138 */
    double oM = Msus * kap, oT = TDPr * kap, oP = PPr * kap;
    double dMsus = p->f_Ar * MA + p->f_IG * MIG + p->f_S * MS + p->Msus_US_i - oM;              /* :141-145 */
    double dTDPr = ((1 - p->beta) * (p->f_A * (1 - p->f_NC_A) * QsA * p->conc_TDPs_A
                                     + p->f_A * p->f_NC_A * QsNC * p->conc_TDPs_NC
                                     + p->f_S * p->f_NC_S * QsNC * p->conc_TDPs_NC)
                    + p->f_A * (1 - p->f_NC_A) * p->Qq_i * p->conc_TDPs_A
                    + p->f_A * p->f_NC_A * p->Qq_i * p->conc_TDPs_NC
                    + p->f_S * p->f_NC_S * p->Qq_i * p->conc_TDPs_NC
                    + Qg * (p->TDPg * p->A_catch) + p->TDPeff + p->TDPr_US_i - oT);             /* :154-166 */
    double dPPr = (p->E_PP * (p->f_Ar * (1 - p->f_NC_Ar) * MA * (p->PlabA_i + p->P_inactive) / p->Msoil
                              + p->f_IG * (1 - p->f_NC_IG) * MIG * (p->PlabA_i + p->P_inactive) / p->Msoil
                              + p->f_S * (1 - p->f_NC_S) * MS * p->P_inactive / p->Msoil
                              + p->f_Ar * p->f_NC_Ar * MA * (p->PlabNC_i + p->P_inactive) / p->Msoil
                              + p->f_IG * p->f_NC_IG * MIG * (p->PlabNC_i + p->P_inactive) / p->Msoil
                              + p->f_S * p->f_NC_S * MS * (p->PlabNC_i + p->P_inactive) / p->Msoil)
                   + p->PPr_US_i - oP);                                                         /* :171-178 */
    double r = dQr / Qr;
    dz[0] = dVsA; dz[1] = dVsS; dz[2] = dVg; dz[3] = dQr; dz[4] = dMsus; dz[5] = dTDPr; dz[6] = dPPr;
    dz[7] = -p->mu * EA * dVsA; dz[8] = -p->mu * ES * dVsS;
    dz[9] = p->b_Q * pb * r; dz[10] = p->k_M * pk * r;
    dz[11] = Qr; dz[12] = oM; dz[13] = oT; dz[14] = oP;                                         /* :132,:147,:168,:180 */
}

/* The stability-optimised pair of integrator 2 (opts.stiff_pair; include/simplyp_controller.h SIMPLYP_STIFF_*, derived by
 * tools/derive_stiff_pair.py): 6 stages, order 4 with an embedded order 3, stable on the real axis down to -9.01 with every
 * stage polynomial <= 1.5 there, the sparsity of Cash-Karp's weights.  erk_aug_day uses it, attempt by attempt, where the
 * step is bound by the stability of Cash-Karp (|h x rate| <= 3.73, rate = cQ Qr**b_Q: a reach far down a network), not by
 * accuracy -- the rule is in erk_aug_day and mirrored by ck_day<SysAug, true> / ck_day_quad<true> in the kernels. */
static const erk_tableau TAB_STIFF = {
    {{0}, {SIMPLYP_STIFF_A21}, {SIMPLYP_STIFF_A31, SIMPLYP_STIFF_A32}, {SIMPLYP_STIFF_A41, SIMPLYP_STIFF_A42, SIMPLYP_STIFF_A43},
     {SIMPLYP_STIFF_A51, SIMPLYP_STIFF_A52, SIMPLYP_STIFF_A53, SIMPLYP_STIFF_A54},
     {SIMPLYP_STIFF_A61, SIMPLYP_STIFF_A62, SIMPLYP_STIFF_A63, SIMPLYP_STIFF_A64, SIMPLYP_STIFF_A65}},
    {SIMPLYP_STIFF_B1, 0, SIMPLYP_STIFF_B3, SIMPLYP_STIFF_B4, 0, SIMPLYP_STIFF_B6},
    {SIMPLYP_STIFF_E1, 0, SIMPLYP_STIFF_E3, SIMPLYP_STIFF_E4, SIMPLYP_STIFF_E5, SIMPLYP_STIFF_E6},
    SIMPLYP_STIFF_ERR_EXP};

/* Same step-size rule as cashkarp_day (the kernel mirrors both) with Cash-Karp ck, and the second pair where the step is bound by
 * stability when stiff is not NULL.  y is the reference's 12-vector; slot 3 (Vr) is returned on its invariant. */
static void erk_aug_day(const erk_tableau* ck, const erk_tableau* stiff, double* y, const ode_params* p, double T, double rtol, double atol,
                        int max_steps, double* h_carry, integ_stats* st)
{
    double k[ERK_STAGES][NZ], zt[NZ], zn[NZ], z[NZ];
    /* (the step size carried over the day boundary belongs to the smooth end of a day; the forcing jumps at midnight and the first
     * attempt of the new day with it was rejected on 85 % of the member-days: SysAug::DAY_START of it is the better guess) */
    double t = 0.0, h = *h_carry * AUG_DAY_START;
    int attempts = 0;
    const double Kv = p->L_reach / (p->a_Q * 8.64 * 10000), invKv = 1.0 / Kv;
    if (!(h > 0.0) || h > T) h = T;
    if (!state_finite(y)) { y[5] = y[7] = y[9] = y[11] = NAN; st->poisoned = 1; return; }
    z[0] = y[0]; z[1] = y[1]; z[2] = y[2]; z[3] = y[4]; z[4] = y[6]; z[5] = y[8]; z[6] = y[10];
    z[7] = exp(-p->mu * y[0]); z[8] = exp(-p->mu * y[1]);
    z[9] = pow(y[4], p->b_Q); z[10] = pow(y[4], p->k_M);
    z[11] = z[12] = z[13] = z[14] = 0.0;
    if (stiff) {      /* opts.stiff_pair: the day's first step reaches at most SIMPLYP_STIFF_Z_START relaxation times of the reach */
        const double rate0 = (p->a_Q * (8.64 * 10000) / ((1 - p->b_Q) * (p->L_reach))) * z[9];
        if (h * rate0 > SIMPLYP_STIFF_Z_START) h = SIMPLYP_STIFF_Z_START / rate0;
    }
    while (t < T) {
        double rem = T - t, hh = h;
        if (rem <= 1.1 * h) hh = rem; else if (rem < 2.0 * h) hh = 0.5 * rem;
        int last_chance = (attempts + 1 >= max_steps);
        if (last_chance) hh = rem;
        /* opts.stiff_pair: an attempt never reaches further than SIMPLYP_STIFF_CAP relaxation times of the reach (the second pair's real
         * stability interval ends at 9.01); the rate is the carried state cQ Qr**b_Q itself */
        const double stiff_rate = (p->a_Q * (8.64 * 10000) / ((1 - p->b_Q) * (p->L_reach))) * z[9];
        if (stiff && !last_chance && hh * stiff_rate > SIMPLYP_STIFF_CAP) hh = SIMPLYP_STIFF_CAP / stiff_rate;
        ode_aug(z, p, invKv, k[0]);
        /* Aim at the knee (SysAug::KNEE_*): time to the nearest knee of a gate along the first slope; a knee inside the step
         * ends the step just past it, so that the right-hand side is smooth over all but its last few percent. */
        int targeted = 0, kink = 0, kink_gw = 0;
        {
            double hs = 1.0e300, hg = 1.0e300, ugd = 0.0;      /* soil boxes, groundwater; Qg gate: upper knee minus Vg / T_g - Qg_min */
            const double tlo = AUG_KNEE_LO * hh, invTg = 1.0 / p->T_g;
            for (int i = 0; i < 3; ++i) {
                const double g = (i < 2) ? z[i] - p->fc : z[2] * invTg - p->Qg_min;
                const double sl = (i < 2) ? k[0][i] : k[0][2] * invTg;
                const double gd = (i < 2) ? 0.01 * p->fc : 0.01 * p->Qg_min;
                const double gdg = gd - g;
                const double t0 = (0.0 - g) / sl, t1 = gdg / sl;
                double tn = 1.0e300;
                if (t0 > tlo && t0 < tn) tn = t0;
                if (t1 > tlo && t1 < tn) tn = t1;
                if (i < 2) { if (tn < hs) hs = tn; } else { hg = tn; ugd = gdg; }
            }
            const double hk = fmin(hs, hg);
            if (!last_chance && hk * AUG_KNEE_OVER < AUG_KNEE_HI * hh) { hh = hk * AUG_KNEE_OVER; targeted = 1; }
            /* A knee within AUG_KINK_REACH x the step along the first slope that the step was not aimed at: its estimate is not
             * trusted (SysAug::KINK_*).  A soil box that starts to drain within the step can lift Vg through its gate within the
             * same step, which the slope at the step's start (-Qg) cannot see: a soil knee within reach while Vg / T_g is below
             * the upper knee of its gate counts as a groundwater knee too. */
            const double look = AUG_KINK_REACH * hh;
            kink = hs < look;
            kink_gw = (hg < look) | (kink & (ugd > 0.0));
        }
        /* Which pair takes this attempt.  Cash-Karp (5th order) unless the step is longer than SIMPLYP_STIFF_Z_ON relaxation times of the
         * reach, where Cash-Karp's own stability ends (3.73): then the stability-optimised 4(3) pair -- except for an attempt that has a
         * knee of a gate within reach or was aimed at one: its estimate is what the knee rules were tuned on (with the second pair there a
         * storm day of a 256-reach chain came out at 4.7e-7 instead of 1.2e-7), so such an attempt is shortened to Cash-Karp's interval
         * instead.  A lane's choice depends on its own state only: results do not depend on which members share a wavefront. */
        const erk_tableau* tab = ck;
        if (stiff && hh * stiff_rate > SIMPLYP_STIFF_Z_ON) {
            if (!(kink || kink_gw || targeted)) tab = stiff;
            else if (!last_chance) hh = SIMPLYP_STIFF_Z_ON / stiff_rate;
        }
        for (int s = 1; s < ERK_STAGES; ++s) {
            for (int i = 0; i < NZ; ++i) {
                double acc = 0.0;
                for (int j = 0; j < s; ++j) acc += tab->A[s][j] * k[j][i];
                zt[i] = z[i] + hh * acc;
            }
            ode_aug(zt, p, invKv, k[s]);
        }
        st->rhs += ERK_STAGES;
        double err = 0.0, err_fast = 0.0; int bad = 0;
        for (int i = 0; i < NZ; ++i) {
            double inc = 0.0, ee = 0.0;
            for (int s = 0; s < ERK_STAGES; ++s) { inc += tab->B[s] * k[s][i]; ee += tab->E[s] * k[s][i]; }
            zn[i] = z[i] + hh * inc;
            /* error norm: the 7 physical states (see below), and Qr**k_M (z[10]) at AUG_AUX_WEIGHT x the tolerance: on a day
             * when a nearly dry reach is wetted it grows 200-fold, and its own truncation error then showed in the sediment
             * flux (SysAug::AUX_WEIGHT in simplyp_kernels.hip.h) */
            if (i >= AUG_NERR && i != 10) continue;
            /* Error scale: rtol * max(|z|, |Euler predictor|) + atol, as in the kernel -- with the two soil boxes measured from
             * field capacity and floored by the gate width 0.01 fc: what the rest of the system sees of a soil box is
             * Vs - fc (gate argument and flow, model.py:105-110), ~1 mm out of ~300, so an error of 1e-8 |Vs| would be
             * 3e-6 of the flow.  (SysAug::SOIL_REL in simplyp_kernels.hip.h.) */
            const double dgate = 0.01 * p->fc;
            double ref = (i < 2) ? z[i] - p->fc : z[i];
            double pred = ref + hh * k[0][i];
            double w = fmax(fabs(ref), fabs(pred));
            if (i < 2) w = fmax(w, dgate);
            double sc = atol + rtol * w;
            if (i == 10) sc = AUG_AUX_WEIGHT * atol + (AUG_AUX_WEIGHT * rtol) * w;
            double r = fabs(hh * ee) / sc;
            /* (the reach's flow, its three masses and Qr**k_M apart: their estimate may be discounted, below) */
            if ((i >= 3 && i <= 6) || i == 10) { if (r > err_fast) err_fast = r; }
            else if (r > err) err = r;
        }
        if (stiff) {
            /* opts.stiff_pair: damping-aware weights (include/simplyp_controller.h, SIMPLYP_DAMP_*) -- what the reach forgets at rate lam is
             * allowed F x the tolerance */
            double lam = stiff_rate - p->b_Q * k[0][3] / z[3];
            if (lam > stiff_rate) lam = stiff_rate;
            double F = fmin(lam * T * (1.0 / SIMPLYP_DAMP_PHI), 1.0 + lam * (rem - hh));
            F = fmin(fmax(F, 1.0), SIMPLYP_DAMP_FMAX);
            err_fast = err_fast / F;
        }
        if (err_fast > err) err = err_fast;
        {   /* expansive reach (SIMPLYP_CTRL_EXPAND, SysAug::EXPAND): d(dQr/dt)/dQr > 0  <=>  b_Q x (net inflow) > Qr; k[0][3] = inflow cQ pb */
            const double cQ = p->a_Q * (8.64 * 10000) / ((1 - p->b_Q) * (p->L_reach));
            if (p->b_Q * k[0][3] > z[3] * (cQ * z[9])) err *= SIMPLYP_CTRL_EXPAND;
        }
        if (kink_gw) err *= targeted ? AUG_KNEE_GW : AUG_KINK_GW;     /* a crossing the first slope did not announce: accepted only if short */
        else if (kink && !targeted) err *= AUG_KINK_SOIL;            /* (a step that ends at a soil knee: no inflation) */
        if (!(err < 1.0e300)) bad = 1;
        for (int i = 0; i < 11; ++i) if (!(fabs(zn[i]) < 1.0e300)) bad = 1;
        ++attempts;
        if (last_chance) st->capped = 1;
        if (bad && (last_chance || hh <= 1.0e-9 * T)) {
            for (int i = 0; i < NY; ++i) y[i] = NAN;
            st->poisoned = 1;
            *h_carry = h;
            return;
        } else if (!bad && (err <= 1.0 || last_chance)) {
            memcpy(z, zn, sizeof(zn));
            t = (hh == rem) ? T : t + hh;
            st->steps++;
        } else {
            st->rejected++;
        }
        /* pb, pk ride a neutrally stable manifold (nothing damps their drift from Qr**b, Qr**k) and are not in the error
         * norm, so on a storm day of 100+ steps the local errors would add up: re-evaluate them after every AUG_RESYNC-th
         * attempt of the day, accepted or not (a member's attempts are its own history; in the kernel the lanes of a
         * wavefront attempt in lockstep, so this test is wave-uniform there) */
        if (attempts % AUG_RESYNC == 0 && t < T) { z[9] = pow(z[3], p->b_Q); z[10] = pow(z[3], p->k_M); }
        double fac;
        if (bad) fac = SIMPLYP_CTRL_FAC_MIN;
        else if (err == 0.0) fac = SIMPLYP_CTRL_FAC_MAX;
        else { fac = SIMPLYP_CTRL_SAFETY * pow(err, tab->err_exp); if (fac < SIMPLYP_CTRL_FAC_MIN) fac = SIMPLYP_CTRL_FAC_MIN; if (fac > SIMPLYP_CTRL_FAC_MAX) fac = SIMPLYP_CTRL_FAC_MAX; }
        /* (a step that was cut to end at a knee and accepted does not shorten the step size carried on) */
        if (!(targeted && !bad && err <= 1.0 && hh * fac < h)) h = hh * fac;
    }
    *h_carry = h;
    y[0] = z[0]; y[1] = z[1]; y[2] = z[2]; y[4] = z[3]; y[6] = z[4]; y[8] = z[5]; y[10] = z[6];
    y[5] = z[11]; y[7] = z[12]; y[9] = z[13]; y[11] = z[14];
    y[3] = Kv * pow(y[4], 1.0 - p->b_Q);
}

static void cashkarp_aug_day(double* y, const ode_params* p, double T, double rtol, double atol,
                             int max_steps, double* h_carry, integ_stats* st, int stiff)
{
    erk_aug_day(&TAB_CASHKARP, stiff ? &TAB_STIFF : NULL, y, p, T, rtol, atol, max_steps, h_carry, st);
}

/* ------------------------------------------------------------------------------------- */
/*
 * SIMPLYP_INTEG_CASHKARP_AUG_F32 -- the same-arithmetic mirror of the kernel's reduced-precision mode (BASELINE config
 * C5: "fp32 state + fp64 mass-balance accumulators"; SysAugF / DayConstF / ck_day<SysAugF> in
 * simplyp_amd/csrc/simplyp_kernels.hip.h).  NOT a parity-grade mode: fp32 stages cannot resolve rtol below ~3e-6; this
 * mirror exists so that the fp32 kernel has a checker that does the same thing, not one that is merely close.
 *   - the 11 Runge-Kutta states, every stage, the error norm and the step-size control are `float`;
 *   - the day constants are formed in double exactly as the kernel hoists them (DayConst) and rounded to float once per day;
 *   - the auxiliary states start each day from double-precision exp / pow rounded to float, and are re-evaluated in float
 *     after every 8th attempt;
 *   - the four daily integrals are accumulated in double from float increments; the state carried to the next day, Vr on
 *     its invariant, the soil-P update and everything else outside the day's integration stay double.
 * Remaining differences to the kernel: libm logf/expf/powf against v_log_f32 / v_exp_f32 (1-2 ulp of float), a true float
 * division against v_rcp_f32 (+ one Newton step), and 0.9 err^-0.2 through powf -- all far below the step controller's
 * own tolerance; an accept/reject decision may flip on them, after which the two runs are two valid integrations at the
 * same rtol.  Tests compare at 10 x rtol.
 */
typedef struct {
    float c0, aE, mu, fc, inv_d, invTsA, invTsS, invTg, Qgmin, inv_dg, beta, fA, fS, qin, omb, cQ, bQ, kM,
          Esum, MsusUS, tA, tS, tg, tconst, cPP, PPrUS, invKv;
} dayconst_f;

static float gate_f(float u, float inv_d)            /* f_x as one clamped cubic, like the kernel's gate() */
{
    float s = u * inv_d;
    s = fminf(fmaxf(s, 0.0f), 1.0f);
    return s * s * fmaf(-2.0f, s, 3.0f);
}

static void dayconst_from_params(const ode_params* p, dayconst_f* c)
{
    const double omb = 1.0 - p->beta;
    const double wA = p->f_A * (1 - p->f_NC_A);                       /* TDP source weights (:155-161) */
    const double wNC = p->f_A * p->f_NC_A + p->f_S * p->f_NC_S;
    const double tNC = omb * wNC * p->conc_TDPs_NC;
    const double Kv = p->L_reach / (p->a_Q * 8.64 * 10000);
    const double pA = (p->PlabA_i + p->P_inactive) / p->Msoil, pN = (p->PlabNC_i + p->P_inactive) / p->Msoil;
    const double p0 = p->P_inactive / p->Msoil;
    const double inv_dg = (p->Qg_min * 0.01 > 0.0) ? 1.0 / (p->Qg_min * 0.01) : 1.0e300;
    c->c0 = (float)(p->P * (1 - p->f_quick));
    c->aE = (float)(p->alpha * p->E);
    c->mu = (float)p->mu; c->fc = (float)p->fc; c->inv_d = (float)(1.0 / (0.01 * p->fc));
    c->invTsA = (float)(1.0 / p->T_s_A); c->invTsS = (float)(1.0 / p->T_s_S);
    c->invTg = (float)(1.0 / p->T_g); c->Qgmin = (float)p->Qg_min;
    c->inv_dg = (float)fmin(inv_dg, 1.0e30);
    c->beta = (float)p->beta; c->fA = (float)p->f_A; c->fS = (float)p->f_S;
    c->qin = (float)(p->Qq_i + p->Qr_US_i);
    c->omb = (float)omb;
    c->cQ = (float)(p->a_Q * (8.64 * 10000) / ((1 - p->b_Q) * p->L_reach));
    c->bQ = (float)p->b_Q; c->kM = (float)p->k_M;
    c->Esum = (float)(p->f_Ar * p->Esus_A + p->f_IG * p->Esus_IG + p->f_S * p->Esus_S);
    c->MsusUS = (float)p->Msus_US_i;
    c->tA = (float)(omb * wA * p->conc_TDPs_A + (p->NC_type == 1 ? tNC : 0.0));
    c->tS = (float)(p->NC_type == 1 ? 0.0 : tNC);
    c->tg = (float)(p->TDPg * p->A_catch);
    c->tconst = (float)(p->Qq_i * (wA * p->conc_TDPs_A + wNC * p->conc_TDPs_NC) + p->TDPeff + p->TDPr_US_i);
    c->cPP = (float)(p->E_PP * (p->f_Ar * p->Esus_A * ((1 - p->f_NC_Ar) * pA + p->f_NC_Ar * pN)
                                + p->f_IG * p->Esus_IG * ((1 - p->f_NC_IG) * pA + p->f_NC_IG * pN)
                                + p->f_S * p->Esus_S * ((1 - p->f_NC_S) * p0 + p->f_NC_S * pN)));
    c->PPrUS = (float)p->PPr_US_i;
    c->invKv = (float)(1.0 / Kv);
}

/* SysAugF::f, operation for operation.  z[11] = VsA VsS Vg Qr Msus TDPr PPr EA ES pb pk; q[4] = integrands of the
 * daily integrals. */
static void ode_aug_f32(const float* z, const dayconst_f* c, float* dz, float* q)
{
    const float uA = z[0] - c->fc, uS = z[1] - c->fc;
    const float QsA = uA * gate_f(uA, c->inv_d) * c->invTsA;
    const float QsS = uS * gate_f(uS, c->inv_d) * c->invTsS;
    dz[0] = fmaf(c->aE, z[7] - 1.0f, c->c0) - QsA;
    dz[1] = fmaf(c->aE, z[8] - 1.0f, c->c0) - QsS;
    const float Qsum = fmaf(c->fA, QsA, c->fS * QsS);
    const float ug = fmaf(z[2], c->invTg, -c->Qgmin);
    const float Qg = fmaf(gate_f(ug, c->inv_dg), ug, c->Qgmin);
    dz[2] = fmaf(c->beta, Qsum, -Qg);
    const float Qr = z[3], pb = z[9], pk = z[10];
    const float inflow = fmaf(c->omb, Qsum, c->qin) + Qg - Qr;
    const float dQr = inflow * c->cQ * pb;
    dz[3] = dQr;
    const float kap = pb * c->invKv;
    const float oM = z[4] * kap, oT = z[5] * kap, oP = z[6] * kap;
    dz[4] = fmaf(c->Esum, pk, c->MsusUS) - oM;
    dz[5] = fmaf(c->tA, QsA, fmaf(c->tS, QsS, fmaf(c->tg, Qg, c->tconst))) - oT;
    dz[6] = fmaf(c->cPP, pk, c->PPrUS) - oP;
    dz[7] = -c->mu * z[7] * dz[0];
    dz[8] = -c->mu * z[8] * dz[1];
    const float r = dQr * (1.0f / Qr);
    dz[9] = c->bQ * pb * r;
    dz[10] = c->kM * pk * r;
    q[0] = Qr; q[1] = oM; q[2] = oT; q[3] = oP;
}

static void cashkarp_aug_f32_day(double* y, const ode_params* p, double T_, double rtol_, double atol_,
                                 int max_steps, double* h_carry, integ_stats* st)
{
    enum { NS = 11 };
    const float T = (float)T_, rtol = (float)rtol_, atol = (float)atol_;
    float A[6][5], B[6], Ee[6];
    for (int s = 0; s < 6; ++s) {
        B[s] = (float)TAB_CASHKARP.B[s]; Ee[s] = (float)TAB_CASHKARP.E[s];
        for (int j = 0; j < 5; ++j) A[s][j] = (float)TAB_CASHKARP.A[s][j];
    }
    float z[NS], zt[NS], k[6][NS], kq[4], sq[4];
    double yq[4] = {0.0, 0.0, 0.0, 0.0};
    float t = 0.0f, h = (float)*h_carry;
    int attempts = 0;
    const double Kv = p->L_reach / (p->a_Q * 8.64 * 10000);
    if (!(h > 0.0f) || h > T) h = T;
    dayconst_f c;
    dayconst_from_params(p, &c);
    z[0] = (float)y[0]; z[1] = (float)y[1]; z[2] = (float)y[2]; z[3] = (float)y[4];
    z[4] = (float)y[6]; z[5] = (float)y[8]; z[6] = (float)y[10];
    z[7] = (float)exp(-p->mu * y[0]); z[8] = (float)exp(-p->mu * y[1]);
    z[9] = (float)pow(y[4], p->b_Q); z[10] = (float)pow(y[4], p->k_M);
    int alive = 1;
    for (int i = 0; i < NS; ++i) if (!(fabsf(z[i]) < 1.0e30f)) alive = 0;      /* (the kernel tests the float states) */
    if (!alive) { y[5] = y[7] = y[9] = y[11] = NAN; st->poisoned = 1; return; }
    while (t < T) {
        const float rem = T - t;
        float hh = h;
        if (rem < 2.0f * h) hh = 0.5f * rem;
        if (rem <= 1.1f * h) hh = rem;
        const int last_chance = (attempts + 1 >= max_steps);
        if (last_chance) hh = rem;
        ode_aug_f32(z, &c, k[0], kq);
        for (int i = 0; i < 4; ++i) sq[i] = B[0] * kq[i];
        for (int s = 1; s < 6; ++s) {
            /* stage weights premultiplied by the step, nested FMAs from the first stage outwards -- the kernel's order */
            float hw[5];
            for (int j = 0; j < s; ++j) hw[j] = hh * A[s][j];
            for (int i = 0; i < NS; ++i) {
                float acc = z[i];
                for (int j = 0; j < s; ++j) acc = fmaf(hw[j], k[j][i], acc);
                zt[i] = acc;
            }
            ode_aug_f32(zt, &c, k[s], kq);
            if (s == 2 || s == 3 || s == 5) for (int i = 0; i < 4; ++i) sq[i] = fmaf(B[s], kq[i], sq[i]);
        }
        st->rhs += 6;
        float err = 0.0f, chk = 0.0f;
        const float he[6] = {hh * Ee[0], 0.0f, hh * Ee[2], hh * Ee[3], hh * Ee[4], hh * Ee[5]};
        for (int i = 0; i < AUG_NERR; ++i) {          /* the plain controller: SysAugF has no knee logic (see the kernel) */
            const float e = fmaf(he[0], k[0][i], fmaf(he[2], k[2][i], fmaf(he[3], k[3][i], fmaf(he[4], k[4][i], he[5] * k[5][i]))));
            if (i >= 3) chk += e;
            const float sc = fmaf(rtol, fmaxf(fabsf(z[i]), fabsf(fmaf(hh, k[0][i], z[i]))), atol);
            const float r = fabsf(e) * (1.0f / sc);
            if (r > err) err = r;
        }
        const int bad = !(err < 1.0e30f) || !(fabsf(chk) < 1.0e30f);
        ++attempts;
        if (last_chance) st->capped = 1;
        const int accept = !bad && (err <= 1.0f || last_chance);
        if (bad && (last_chance || hh <= 1.0e-9f * T)) {
            for (int i = 0; i < NY; ++i) y[i] = NAN;
            st->poisoned = 1;
            *h_carry = (double)h;
            return;
        }
        if (accept) {
            const float hb0 = hh * B[0], hb2 = hh * B[2], hb3 = hh * B[3], hb5 = hh * B[5];
            for (int i = 0; i < NS; ++i)
                z[i] = fmaf(hb5, k[5][i], fmaf(hb3, k[3][i], fmaf(hb2, k[2][i], fmaf(hb0, k[0][i], z[i]))));
            for (int i = 0; i < 4; ++i) yq[i] = fma(1.0, (double)(hh * sq[i]), yq[i]);
            t = (hh == rem) ? T : t + hh;
            st->steps++;
        } else {
            st->rejected++;
        }
        float fac;
        if (bad) fac = (float)SIMPLYP_CTRL_FAC_MIN;
        else {
            fac = (float)SIMPLYP_CTRL_SAFETY * powf(err, -0.2f);               /* err == 0 -> +inf -> 5 */
            fac = fminf(fmaxf(fac, (float)SIMPLYP_CTRL_FAC_MIN), (float)SIMPLYP_CTRL_FAC_MAX);
        }
        h = hh * fac;
        if (attempts % AUG_RESYNC == 0 && t < T) {
            const float lq = logf(z[3]);
            z[9] = expf(c.bQ * lq); z[10] = expf(c.kM * lq);
        }
    }
    *h_carry = (double)h;
    y[0] = z[0]; y[1] = z[1]; y[2] = z[2]; y[4] = z[3]; y[6] = z[4]; y[8] = z[5]; y[10] = z[6];
    y[5] = yq[0]; y[7] = yq[1]; y[9] = yq[2]; y[11] = yq[3];
    y[3] = Kv * pow(y[4], 1.0 - p->b_Q);
}

/* ------------------------------------------------------------------------------------- */
/* One member: the SC loop (model.py:365) around the day loop (model.py:491).              */

#define MP(name) (mp[(size_t)SIMPLYP_PM_##name * E + e])
#define RP(name, s) (rp[((size_t)SIMPLYP_PR_##name * S + (s)) * E + e])

static int nc_type_of(double f_NC_A, double f_NC_S)     /* model.py:325-334 */
{
    if (f_NC_A > 0) return 1;
    else if (f_NC_S > 0) return 2;
    return 0;
}

static void run_member(int e, const simplyp_dims* dims, const simplyp_opts* o, const double* forcing,
                       const int32_t* doy, const int32_t* fom, const double* mp, const double* rp,
                       const int32_t* up_ptr, const int32_t* up_idx, const int32_t* out_slot,
                       int n_out_reaches, int n_integ, double* out, int32_t* status, integ_stats* st)
{
    const int E = dims->E, S = dims->S, D = dims->D;
    /* opts.stiff_pair: 0 = auto (reach networks), > 0 on, < 0 off -- SIMPLYP_STIFF_PAIR_ON in include/simplyp_controller.h, the rule the library uses */
    const int stiff_pair = SIMPLYP_STIFF_PAIR_ON(o->stiff_pair, S) && n_integ == SIMPLYP_INTEG_CASHKARP_AUG;
    const double* Pser = forcing + (size_t)(fom ? fom[e] : 0) * (o->snow ? 3 : 2) * D;   /* Precipitation when o->snow */
    const double* Eser = Pser + D;
    const double* Tser = Eser + D;                                                        /* T_air (o->snow only) */
    /* daily series of every reach of this member that a downstream reach may read (:524-528) */
    double* route = (double*)malloc(sizeof(double) * 4 * (size_t)S * D);

    int col_of[SIMPLYP_N_OUT], ncols = 0;
    for (int c = 0; c < SIMPLYP_N_OUT; ++c) col_of[c] = (o->out_mask >> c) & 1u ? ncols++ : -1;
    int32_t stat = 0;

    const double fc = MP(FC), f_quick = MP(F_QUICK), alpha = MP(ALPHA), beta = MP(BETA), T_g = MP(T_G);
    const double Qg_min = MP(QG_MIN), a_Q = MP(A_Q), b_Q = MP(B_Q), E_M = MP(E_M), k_M = MP(K_M);
    const double T_s_A = MP(T_S_A), T_s_S = MP(T_S_S);
    const double mu = -log(0.01) / fc;                                                           /* :349 */
    const double E_risk_period = 60.0;                                                           /* :354 */
    const double d_mid[2] = {MP(D_MAXE_SPR), MP(D_MAXE_AUT)};
    const double d_start[2] = {d_mid[0] - E_risk_period / 2., d_mid[1] - E_risk_period / 2.};    /* :358 */
    const double d_end[2] = {d_mid[0] + E_risk_period / 2., d_mid[1] + E_risk_period / 2.};      /* :359 */

    /* the Python variable NC_type left over from the validation loop (:321-335) = last SC's */
    const int NC_type_leak = nc_type_of(RP(F_AR, S - 1) * RP(F_NC_AR, S - 1) + RP(F_NC_IG, S - 1) * RP(F_IG, S - 1),
                                        RP(F_NC_S, S - 1));

    for (int s = 0; s < S; ++s) {                                                                /* :365 */
        const double A_catch = RP(A_CATCH, s);
        const double f_Ar = RP(F_AR, s), f_IG = RP(F_IG, s), f_S = RP(F_S, s);
        const double f_NC_Ar = RP(F_NC_AR, s), f_NC_IG = RP(F_NC_IG, s), f_NC_S = RP(F_NC_S, s);
        const double f_A = f_IG + f_Ar;                                                          /* :318 */
        const double f_NC_A = (f_Ar * f_NC_Ar) + (f_NC_IG * f_IG);                               /* :319 */
        const int NC_type = nc_type_of(f_NC_A, f_NC_S);

        double VsA0 = fc, VsS0 = VsA0;                                                           /* :377-378 */
        double Qr0 = MP(QR0_INIT) * 86400 / (1000 * RP(A_CATCH, o->sc_qr0));                     /* :386, hf.py:29 */
        double Qg0 = beta * Qr0;                                                                 /* :389 */
        double Vg0 = Qg0 * T_g;                                                                  /* :390 */
        double TDPr0 = 0.0, PPr0 = 0.0, Msus0 = 0.0;                                             /* :396 */
        const double Msoil = MP(MSOIL_M2) * 1000000 * A_catch;                                   /* :404 */
        const double P_inactive = 1e-6 * MP(SOILPCONC_S) * Msoil;                                /* :407 */
        const double EPC0_0_A = MP(EPC0_INIT_A) * A_catch;                                       /* :412, hf.py:56 */
        const double EPC0_0_S = MP(EPC0_INIT_S) * A_catch;
        const double Plab0_A_init = 1e-6 * (MP(SOILPCONC_A) - MP(SOILPCONC_S)) * Msoil;          /* :415 */
        const double TDPs0_A_init = EPC0_0_A * VsA0;                                             /* :420 */
        const double TDPs0_S_init = 0;                                                           /* :422 */
        double Plab0_A = Plab0_A_init, TDPs0_A = TDPs0_A_init;                                   /* :426 */
        double Plab0_NC, TDPs0_NC;
        if (NC_type == 2) { Plab0_NC = Plab0_A; TDPs0_NC = TDPs0_A; }                            /* :429-431 */
        else { Plab0_NC = 0.0; TDPs0_NC = TDPs0_S_init; }                                        /* :433-434 */
        double conc_TDPs_A = TDPs0_A / VsA0;                                                     /* :438 */
        double VsNC0 = (NC_type_leak == 1) ? VsA0 : VsS0;                                        /* :442-445 */
        double conc_TDPs_NC = TDPs0_NC / VsNC0;                                                  /* :446 */
        double Kf;
        if (o->run_mode_cal) Kf = 1e-6 * (MP(SOILPCONC_A) - MP(SOILPCONC_S)) / EPC0_0_A;         /* :451 */
        else Kf = MP(KF);                                                                        /* :453 */
        const double L_reach = RP(L_REACH, s);
        double Tr0 = L_reach / (a_Q * pow(Qr0, b_Q) * 8.64 * 10000);                             /* :457-458 */
        double Vr0 = Tr0 * Qr0;                                                                  /* :459 */
        double TDPeff = RP(TDPEFF, s);
        if (isnan(TDPeff)) TDPeff = 0.;                                                          /* :462-463 */
        const double slope_A = RP(S_AR, s), slope_IG = RP(S_IG, s), slope_S = RP(S_SN, s);       /* :469 */
        const double S_reach = RP(S_REACH, s), f_spr = RP(F_SPR, s);

        double h_carry = o->step_len / (o->substeps > 0 ? o->substeps : 1);
        double D_snow = o->snow ? MP(D_SNOW_0) : 0.0;                                            /* inputs.py:198 */

        for (int idx = 0; idx < D; ++idx) {                                                      /* :491 */
            double P = Pser[idx], Ev = Eser[idx];                                                /* :497-498 */
            if (o->snow) {      /* snow_hydrol_inputs, inputs.py:183-208, for this member and day */
                const double T_air = Tser[idx];
                const double P_snow = (T_air < 0.0) ? P : 0.0;                                   /* :183-184 */
                const double P_rain = P - P_snow;                                                /* :187 */
                double P_melt = MP(F_DDSM) * (T_air - 0);                                        /* :190 */
                if (P_melt < 0.0) P_melt = 0.0;                                                  /* :191 */
                P_melt = (D_snow < P_melt) ? D_snow : P_melt;                                    /* :199, :204 */
                D_snow = D_snow + P_snow - P_melt;                                               /* :200, :205 */
                P = P_rain + P_melt;                                                             /* :208 */
            }
            double Qq_i = f_quick * P;                                                           /* :501 */

            double Qr_US_i = 0.0, Msus_US_i = 0.0, TDPr_US_i = 0.0, PPr_US_i = 0.0;              /* :544 */
            for (int k = up_ptr[s]; k < up_ptr[s + 1]; ++k) {                                    /* :521-538 */
                int u = up_idx[k];
                const double* r = route + ((size_t)u * D + idx) * 4;
                Qr_US_i += r[0] * (RP(A_CATCH, u) / A_catch);                                    /* :524-525 */
                Msus_US_i += r[1]; TDPr_US_i += r[2]; PPr_US_i += r[3];                          /* :526-528 */
            }

            /* sediment input coefficients, :549-594 */
            double C_cover_A;
            if (o->dynamic_erod) {
                int dayNo = doy[idx];                                                            /* :550 */
                double C_season[2];
                for (int q = 0; q < 2; ++q) {
                    /* `dayNo in np.arange(d_start, d_end)` (:567): exact float membership */
                    double kk = (double)dayNo - d_start[q];
                    int in_window = (kk >= 0.0 && kk == floor(kk) && kk < ceil(d_end[q] - d_start[q])
                                     && d_start[q] + kk == (double)dayNo);
                    if (in_window) {
                        if (dayNo < d_mid[q])                                                    /* :568-570, hf.py:90 */
                            C_season[q] = MP(C_COVER_A) + (1.0 - MP(C_COVER_A)) * (dayNo - d_start[q]) / (d_mid[q] - d_start[q]);
                        else                                                                     /* :572-573 */
                            C_season[q] = 1.0 + (MP(C_COVER_A) - 1.0) * (dayNo - d_mid[q]) / (d_end[q] - d_mid[q]);
                    } else {
                        C_season[q] = (MP(C_COVER_A) - (E_risk_period * (1 - MP(C_COVER_A))
                                                       / (2 * (365 - E_risk_period))));          /* :575-576 */
                    }
                }
                C_cover_A = (f_spr * C_season[0] + (1 - f_spr) * C_season[1]);                   /* :579-580 */
            } else {
                C_cover_A = MP(C_COVER_A);                                                       /* :583 */
            }
            double Esus_A = (E_M * S_reach * slope_A * C_cover_A * (1 - MP(C_MEAS_A)));          /* :591-594 */
            double Esus_S = (E_M * S_reach * slope_S * MP(C_COVER_S) * (1 - MP(C_MEAS_S)));
            double Esus_IG = (E_M * S_reach * slope_IG * MP(C_COVER_IG) * (1 - MP(C_MEAS_IG)));

            double EPC0_A_i, EPC0_NC_i;
            if (o->dynamic_epc0) {
                EPC0_A_i = fmax(Plab0_A / (Kf * Msoil), 0);                                      /* :602 */
                EPC0_NC_i = fmax(Plab0_NC / (Kf * Msoil), 0);                                    /* :603 */
            } else {
                EPC0_A_i = EPC0_0_A;                                                             /* :607 */
                EPC0_NC_i = (NC_type == 2) ? EPC0_0_A : EPC0_0_S;                                /* :608-611 */
            }

            double y[NY] = {VsA0, VsS0, Vg0, Vr0, Qr0, 0.0, Msus0, 0.0, TDPr0, 0.0, PPr0, 0.0};  /* :618 */
            ode_params op;                                                                       /* :622-632 */
            op.P = P; op.E = Ev; op.mu = mu; op.Qq_i = Qq_i; op.Qr_US_i = Qr_US_i;
            op.Esus_A = Esus_A; op.Esus_S = Esus_S; op.Esus_IG = Esus_IG;
            op.Msus_US_i = Msus_US_i; op.TDPr_US_i = TDPr_US_i; op.PPr_US_i = PPr_US_i;
            op.f_A = f_A; op.f_Ar = f_Ar; op.f_IG = f_IG; op.f_S = f_S; op.f_NC_A = f_NC_A;
            op.f_NC_Ar = f_NC_Ar; op.f_NC_IG = f_NC_IG; op.f_NC_S = f_NC_S; op.NC_type = NC_type;
            op.f_quick = f_quick; op.alpha = alpha; op.beta = beta; op.T_s_A = T_s_A; op.T_s_S = T_s_S;
            op.T_g = T_g; op.fc = fc; op.L_reach = L_reach; op.A_catch = A_catch; op.a_Q = a_Q; op.b_Q = b_Q;
            op.k_M = k_M; op.conc_TDPs_A = conc_TDPs_A; op.conc_TDPs_NC = conc_TDPs_NC;
            op.PlabA_i = Plab0_A; op.PlabNC_i = Plab0_NC; op.Msoil = Msoil; op.TDPeff = TDPeff;
            op.TDPg = MP(TDPG); op.E_PP = MP(E_PP); op.P_inactive = P_inactive; op.Qg_min = Qg_min;

            /* model.py:640 -- the one place that is not a restatement (see header) */
            if (n_integ == SIMPLYP_INTEG_RK4) rk4_day(y, &op, o->step_len, o->substeps, st);
            else if (n_integ == SIMPLYP_INTEG_CASHKARP_AUG)
                cashkarp_aug_day(y, &op, o->step_len, o->rtol, o->atol, o->max_steps, &h_carry, st, stiff_pair);
            else if (n_integ == SIMPLYP_INTEG_CASHKARP_AUG_F32)
                cashkarp_aug_f32_day(y, &op, o->step_len, o->rtol, o->atol, o->max_steps, &h_carry, st);
            else cashkarp_day(y, &op, o->step_len, o->rtol, o->atol, o->max_steps, &h_carry, st);      /* SIMPLYP_INTEG_CASHKARP */
            if (o->project_vr && (n_integ == SIMPLYP_INTEG_RK4 || n_integ == SIMPLYP_INTEG_CASHKARP)) {
                /* Drift control (not in the reference).  The reference's own equations (:127-131) imply
                 * dVr = dQr * (1-b_Q) L / (a_Q 86400 Qr^b_Q), and Vr0 (:457-459) starts on that curve, so
                 * Vr == L Qr^(1-b_Q) / (a_Q 86400) for all t; Vr has no restoring term and a one-step
                 * integrator random-walks off it.  Re-impose it once per day. */
                y[3] = L_reach * pow(y[4], 1.0 - b_Q) / (a_Q * 8.64 * 10000);
            }
            const double* res = y;                                                               /* :643 */
            for (int i = 0; i < NY; ++i) if (!isfinite(res[i])) stat |= SIMPLYP_STATUS_NONFINITE;

            VsA0 = res[0]; VsS0 = res[1]; Vg0 = res[2]; Vr0 = res[3]; Qr0 = res[4];              /* :648-652 */
            Msus0 = res[6]; TDPr0 = res[8]; PPr0 = res[10];                                      /* :654-658 */

            double QsA0 = (VsA0 - fc) * f_x(VsA0, fc, 0.01) / T_s_A;                             /* :663 */
            double QsS0 = (VsS0 - fc) * f_x(VsS0, fc, 0.01) / T_s_S;                             /* :664 */
            double f_Qg = f_x(Vg0 / T_g, Qg_min, 0.01);                                          /* :668 */
            Qg0 = (1 - f_Qg) * Qg_min + f_Qg * (Vg0 / T_g);                                      /* :669 */
            Vg0 = Qg0 * T_g;                                                                     /* :670 */

            double QsNC0;
            if (NC_type_leak == 1) { VsNC0 = VsA0; QsNC0 = QsA0; }                               /* :676-678 */
            else { VsNC0 = VsS0; QsNC0 = QsS0; }                                                 /* :680-681 */

            if (o->dynamic_epc0) {                                                               /* :684 */
                discretized_soilP(MP(P_NETINPUT_A), A_catch, Kf, Msoil, EPC0_A_i, QsA0, Qq_i, VsA0,
                                  TDPs0_A, Plab0_A, &TDPs0_A, &Plab0_A);                         /* :688-689 */
                discretized_soilP(MP(P_NETINPUT_NC), A_catch, Kf, Msoil, EPC0_NC_i, QsNC0, Qq_i, VsNC0,
                                  TDPs0_NC, Plab0_NC, &TDPs0_NC, &Plab0_NC);                     /* :692-693 */
                /* Python max(a, 0.) returns a when a is NaN; fmax would return 0 */
                TDPs0_A = (0. > TDPs0_A) ? 0. : TDPs0_A;                                         /* :696 */
                Plab0_A = (0. > Plab0_A) ? 0. : Plab0_A;                                         /* :697 */
                TDPs0_NC = (0. > TDPs0_NC) ? 0. : TDPs0_NC;                                      /* :698 */
                Plab0_NC = (0. > Plab0_NC) ? 0. : Plab0_NC;                                      /* :699 */
                conc_TDPs_A = TDPs0_A / VsA0;                                                    /* :702 */
                conc_TDPs_NC = TDPs0_NC / VsNC0;                                                 /* :703 */
            } else {
                conc_TDPs_A = EPC0_A_i;                                                          /* :711 */
                conc_TDPs_NC = EPC0_NC_i;                                                        /* :715 */
            }

            double* r = route + ((size_t)s * D + idx) * 4;
            r[0] = res[5]; r[1] = res[7]; r[2] = res[9]; r[3] = res[11];

            int slot = out_slot[s];
            if (slot >= 0) {
                double row[SIMPLYP_N_OUT];
                for (int i = 0; i < NY; ++i) row[i] = res[i];                                    /* :644 */
                row[12] = Qq_i; row[13] = QsA0; row[14] = QsS0; row[15] = Qg0; row[16] = C_cover_A;   /* :721 */
                row[17] = EPC0_A_i; row[18] = EPC0_NC_i; row[19] = TDPs0_A; row[20] = Plab0_A;
                row[21] = conc_TDPs_A; row[22] = TDPs0_NC; row[23] = Plab0_NC; row[24] = conc_TDPs_NC; /* :722-723 */
                row[SIMPLYP_OUT_D_SNOW] = D_snow;      /* met_df['D_snow_end'], inputs.py:200, :205 (written only with o->snow) */
                for (int c = 0; c < SIMPLYP_N_OUT; ++c)
                    if (col_of[c] >= 0)
                        out[(((size_t)col_of[c] * D + idx) * n_out_reaches + slot) * E + e] = row[c];
            }
        }
    }
    if (st->capped) stat |= SIMPLYP_STATUS_STEPCAP;
    if (st->poisoned) stat |= SIMPLYP_STATUS_NONFINITE;
    status[e] = stat;
    free(route);
}

/* Same arguments as simplyp_run() minus the context; every pointer is a host pointer.
 * n_threads > 1 runs members in parallel with OpenMP (cpu_baseline 'all cores' leg). */
int simplyp_oracle_run(const simplyp_dims* dims, const simplyp_opts* opts,
                       const double* forcing, const int32_t* doy, const int32_t* forcing_of_member,
                       const double* member_params, const double* reach_params,
                       const int32_t* up_ptr, const int32_t* up_idx,
                       const int32_t* out_reaches, int32_t n_out_reaches,
                       double* out, int32_t* member_status, simplyp_stats* stats, int n_threads)
{
    if (!dims || !opts || dims->E <= 0 || dims->S <= 0 || dims->D <= 0) return SIMPLYP_ERR_ARG;
    /* the integrators the library accepts (check_args in simplyp_amd/csrc/simplyp_hip.hip); any other id is refused, not run as another */
    if (opts->integrator != SIMPLYP_INTEG_RK4 && opts->integrator != SIMPLYP_INTEG_CASHKARP &&
        opts->integrator != SIMPLYP_INTEG_CASHKARP_AUG && opts->integrator != SIMPLYP_INTEG_CASHKARP_AUG_F32)
        return SIMPLYP_ERR_ARG;
    if (!(opts->step_len > 0.0) || !isfinite(opts->step_len)) return SIMPLYP_ERR_ARG;      /* as check_args */
    const int S = dims->S;
    int32_t* out_slot = (int32_t*)malloc(sizeof(int32_t) * S);
    for (int s = 0; s < S; ++s) out_slot[s] = out_reaches ? -1 : s;
    if (out_reaches) for (int k = 0; k < n_out_reaches; ++k) out_slot[out_reaches[k]] = k;
    else n_out_reaches = S;
    for (int s = 0; s < S; ++s)
        for (int k = up_ptr[s]; k < up_ptr[s + 1]; ++k)
            if (up_idx[k] < 0 || up_idx[k] >= s) { free(out_slot); return SIMPLYP_ERR_TOPOLOGY; }
    uint64_t rhs = 0, steps = 0, rej = 0;
    (void)n_threads;
#ifdef _OPENMP
    if (n_threads > 0) omp_set_num_threads(n_threads);
#pragma omp parallel for schedule(dynamic, 4) reduction(+ : rhs, steps, rej)
#endif
    for (int e = 0; e < dims->E; ++e) {
        integ_stats st = {0, 0, 0, 0, 0};
        run_member(e, dims, opts, forcing, doy, forcing_of_member, member_params, reach_params, up_ptr, up_idx,
                   out_slot, n_out_reaches, opts->integrator, out, member_status, &st);
        rhs += st.rhs; steps += st.steps; rej += st.rejected;
    }
    if (stats) { memset(stats, 0, sizeof(*stats)); stats->rhs_evals = rhs; stats->steps = steps; stats->rejected = rej; }
    free(out_slot);
    return SIMPLYP_OK;
}

/* ---- scalar entry points used to pin the restatement against tests/golden/unit_vectors.npz */
double simplyp_oracle_fx(double x, double threshold, double reld) { return f_x(x, threshold, reld); }

void simplyp_oracle_soilp(const double* in10, double* out2)
{   /* in10 = P_netInput, A_catch, Kf, Msoil, EPC0, Qs, Qq, Vs, TDPs, Plab */
    discretized_soilP(in10[0], in10[1], in10[2], in10[3], in10[4], in10[5], in10[6], in10[7], in10[8], in10[9],
                      &out2[0], &out2[1]);
}

static void params_from_p43(const double* p43, ode_params* pp)
{   /* p43 in the order of unit_vectors.npz 'ode_p_names' */
    ode_params p;
    p.P = p43[0]; p.E = p43[1]; p.mu = p43[2]; p.Qq_i = p43[3]; p.Qr_US_i = p43[4];
    p.Esus_A = p43[5]; p.Esus_S = p43[6]; p.Esus_IG = p43[7];
    p.Msus_US_i = p43[8]; p.TDPr_US_i = p43[9]; p.PPr_US_i = p43[10];
    p.f_A = p43[11]; p.f_Ar = p43[12]; p.f_IG = p43[13]; p.f_S = p43[14]; p.f_NC_A = p43[15];
    p.f_NC_Ar = p43[16]; p.f_NC_IG = p43[17]; p.f_NC_S = p43[18]; p.NC_type = (int)p43[19];
    p.f_quick = p43[20]; p.alpha = p43[21]; p.beta = p43[22]; p.T_s_A = p43[23]; p.T_s_S = p43[24];
    p.T_g = p43[25]; p.fc = p43[26]; p.L_reach = p43[27]; p.A_catch = p43[28]; p.a_Q = p43[29];
    p.b_Q = p43[30]; /* p43[31] = E_M, unused inside ode_f */ p.k_M = p43[32];
    p.conc_TDPs_A = p43[33]; p.conc_TDPs_NC = p43[34]; p.PlabA_i = p43[35]; p.PlabNC_i = p43[36];
    p.Msoil = p43[37]; p.TDPeff = p43[38]; p.TDPg = p43[39]; p.E_PP = p43[40]; p.P_inactive = p43[41];
    p.Qg_min = p43[42];
    *pp = p;
}

void simplyp_oracle_ode_f(const double* y12, const double* p43, double* dy12)
{
    ode_params p;
    params_from_p43(p43, &p);
    ode_f(y12, &p, dy12);
}

/* ode_aug at the state y12 (slot 3, Vr, is not read: the form takes it from its invariant), the auxiliary states and invKv formed
 * the way erk_aug_day forms them.  dz15 = d/dt of VsA VsS Vg Qr Msus TDPr PPr EA ES pb pk | the four daily integrands. */
void simplyp_oracle_ode_aug(const double* y12, const double* p43, double* dz15)
{
    ode_params p;
    double z[NZ];
    params_from_p43(p43, &p);
    const double Kv = p.L_reach / (p.a_Q * 8.64 * 10000), invKv = 1.0 / Kv;
    z[0] = y12[0]; z[1] = y12[1]; z[2] = y12[2]; z[3] = y12[4]; z[4] = y12[6]; z[5] = y12[8]; z[6] = y12[10];
    z[7] = exp(-p.mu * y12[0]); z[8] = exp(-p.mu * y12[1]);
    z[9] = pow(y12[4], p.b_Q); z[10] = pow(y12[4], p.k_M);
    z[11] = z[12] = z[13] = z[14] = 0.0;
    ode_aug(z, &p, invKv, dz15);
}

/* ode_aug_f32 at the state y12, states and constants rounded to float the way cashkarp_aug_f32_day rounds them; widened. */
void simplyp_oracle_ode_aug_f32(const double* y12, const double* p43, double* dz15)
{
    ode_params p;
    dayconst_f c;
    float z[11], dz[11], q[4];
    params_from_p43(p43, &p);
    dayconst_from_params(&p, &c);
    z[0] = (float)y12[0]; z[1] = (float)y12[1]; z[2] = (float)y12[2]; z[3] = (float)y12[4];
    z[4] = (float)y12[6]; z[5] = (float)y12[8]; z[6] = (float)y12[10];
    z[7] = (float)exp(-p.mu * y12[0]); z[8] = (float)exp(-p.mu * y12[1]);
    z[9] = (float)pow(y12[4], p.b_Q); z[10] = (float)pow(y12[4], p.k_M);
    ode_aug_f32(z, &c, dz, q);
    for (int i = 0; i < 11; ++i) dz15[i] = (double)dz[i];
    for (int i = 0; i < 4; ++i) dz15[11 + i] = (double)q[i];
}
