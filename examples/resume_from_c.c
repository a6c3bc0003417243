/* resume_from_c.c -- warm start through the C ABI (include/simplyp.h): a run made in two halves through
 * simplyp_set_state equals the one-piece run, bit for bit.
 *
 * The problem of run_from_c.c (one sub-catchment with the Tarland workbook's parameters, synthetic forcing, E members
 * that differ in T_g).  Three runs on one context:
 *   1. days [0, D) in one piece, the end state saved;
 *   2. days [0, D1), the end state saved into `d_state`;
 *   3. days [D1, D) started from `d_state`, the end state written back into the same buffer (the two may alias).
 * The tables of 2 and 3 laid end to end, the final state and the summed right-hand-side counts are then compared with 1.
 *
 *   gcc -O2 -Iinclude examples/resume_from_c.c -o resume_from_c -Lsimplyp_amd/csrc -lsimplyp_hip -Wl,-rpath,$PWD/simplyp_amd/csrc -lm
 *   ./resume_from_c [E] [D] [D1]
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "simplyp.h"

#define CHECK(call)                                                                                       \
    do {                                                                                                  \
        int rc__ = (call);                                                                                \
        if (rc__ != SIMPLYP_OK) {                                                                         \
            fprintf(stderr, "%s failed (%d): %s\n", #call, rc__, simplyp_last_error(ctx));                \
            return 1;                                                                                     \
        }                                                                                                 \
    } while (0)

#define N_COLS 5      /* SIMPLYP_MASK_REACH5 */

int main(int argc, char** argv)
{
    const int E = argc > 1 ? atoi(argv[1]) : 128, D = argc > 2 ? atoi(argv[2]) : 730, S = 1;
    const int D1 = argc > 3 ? atoi(argv[3]) : D / 2 + (D > 40 ? 17 : 0);      /* not a time-chunk boundary */
    simplyp_ctx* ctx = NULL;
    if (E < 1 || D < 2 || D1 < 1 || D1 >= D) { fprintf(stderr, "need E >= 1 and 0 < D1 < D\n"); return 1; }
    if (simplyp_abi_version() != SIMPLYP_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 1; }
    if (simplyp_device_count() < 1) { fprintf(stderr, "no HIP device\n"); return 2; }
    CHECK(simplyp_ctx_create(0, &ctx));

    const size_t n_mp = (size_t)SIMPLYP_NP_M * E, n_rp = (size_t)SIMPLYP_NP_R * S * E;
    double* P = (double*)malloc((size_t)D * sizeof(double));
    double* PET = (double*)malloc((size_t)D * sizeof(double));
    int32_t* doy = (int32_t*)malloc((size_t)D * sizeof(int32_t));
    double* mp = (double*)malloc(n_mp * sizeof(double));
    double* rp = (double*)malloc(n_rp * sizeof(double));
    if (!P || !PET || !doy || !mp || !rp) { fprintf(stderr, "host alloc failed\n"); return 1; }
    for (int d = 0; d < D; ++d) {
        const double season = 0.5 - 0.5 * cos(2.0 * M_PI * d / 365.25);
        P[d] = (d % 5 == 0) ? 9.0 + 6.0 * sin(0.37 * d) : ((d % 3 == 0) ? 1.5 : 0.0);      /* mm/day */
        PET[d] = 0.2 + 2.8 * season;                                                      /* mm/day */
        doy[d] = d % 365 + 1;
    }
    static const double pm[SIMPLYP_NP_M] = {
        /* f_quick alpha fc beta T_g Qg_min a_Q b_Q Qr0_init Msoil_m2 Kf */ 0.02, 1, 290, 0.7, 65, 0.4, 0.5, 0.42, 1, 95, 1.131528046e-4,
        /* TDPg E_PP E_M k_M d_maxE_spr d_maxE_aut */ 0.02, 1.6, 1500, 2, 60, 304,
        /* T_s A,S  SoilPconc A,S  P_netInput A,NC  EPC0_init A,S */ 2, 10, 1458, 873, 10, 10, 0.1, 0,
        /* C_cover A,S,IG  C_measures A,S,IG */ 0.2, 0.021, 0.09, 0, 0, 0,
        /* f_DDSM D_snow_0 */ 2.74, 0};
    static const double pr[SIMPLYP_NP_R] = {/* A_catch f_Ar f_IG f_S f_NC_Ar f_NC_IG f_NC_S f_spr */ 51.7, 0.2, 0.3, 0.5, 0, 0, 0, 0.65,
                                            /* S_Ar S_IG S_SN L_reach S_reach TDPeff */ 4, 4, 10, 10000, 0.8, 0.1};
    for (int i = 0; i < SIMPLYP_NP_M; ++i) for (int e = 0; e < E; ++e) mp[(size_t)i * E + e] = pm[i];
    for (int i = 0; i < SIMPLYP_NP_R; ++i) for (int e = 0; e < E; ++e) rp[(size_t)i * E + e] = pr[i];
    for (int e = 0; e < E; ++e) mp[(size_t)SIMPLYP_PM_T_G * E + e] = 40.0 + 60.0 * e / (E > 1 ? E - 1 : 1);

    simplyp_opts opts;
    memset(&opts, 0, sizeof(opts));
    opts.integrator = SIMPLYP_INTEG_CASHKARP_AUG; opts.substeps = 8; opts.rtol = 1e-7; opts.atol = 1e-12; opts.max_steps = 4000;
    opts.dynamic_epc0 = 1; opts.run_mode_cal = 1; opts.out_mask = SIMPLYP_MASK_REACH5; opts.step_len = 1.0; opts.project_vr = 1;
    opts.balance = 2;
    const int32_t up_ptr[2] = {0, 0};

    /* the three runs: first day, number of days */
    const int first[3] = {0, 0, D1}, days[3] = {D, D1, D - D1};
    const simplyp_dims dims_all = {E, S, D, 1};
    const int64_t state_bytes = simplyp_state_bytes(&dims_all);
    const size_t row = (size_t)E;                     /* doubles per table row (one output reach) */
    double* d_mp = (double*)simplyp_device_alloc(ctx, (int64_t)(n_mp * sizeof(double)));
    double* d_rp = (double*)simplyp_device_alloc(ctx, (int64_t)(n_rp * sizeof(double)));
    double* d_forcing = (double*)simplyp_device_alloc(ctx, (int64_t)((size_t)2 * D * sizeof(double)));
    int32_t* d_doy = (int32_t*)simplyp_device_alloc(ctx, (int64_t)((size_t)D * sizeof(int32_t)));
    double* d_out = (double*)simplyp_device_alloc(ctx, simplyp_out_bytes(&dims_all, &opts, 1));
    int32_t* d_status = (int32_t*)simplyp_device_alloc(ctx, (int64_t)((size_t)E * sizeof(int32_t)));
    double* d_state_whole = (double*)simplyp_device_alloc(ctx, state_bytes);
    double* d_state = (double*)simplyp_device_alloc(ctx, state_bytes);
    if (!d_mp || !d_rp || !d_forcing || !d_doy || !d_out || !d_status || !d_state_whole || !d_state) {
        fprintf(stderr, "device alloc failed: %s\n", simplyp_last_error(ctx));
        return 1;
    }
    CHECK(simplyp_memcpy_h2d(ctx, d_mp, mp, (int64_t)(n_mp * sizeof(double))));
    CHECK(simplyp_memcpy_h2d(ctx, d_rp, rp, (int64_t)(n_rp * sizeof(double))));

    double* whole = (double*)malloc((size_t)N_COLS * D * row * sizeof(double));       /* [col][D][E] */
    double* pieces = (double*)malloc((size_t)N_COLS * D * row * sizeof(double));      /* the halves, laid end to end */
    double* part = (double*)malloc((size_t)N_COLS * D * row * sizeof(double));
    double* forcing = (double*)malloc((size_t)2 * D * sizeof(double));
    double* st_whole = (double*)malloc((size_t)state_bytes);
    double* st_pieces = (double*)malloc((size_t)state_bytes);
    int32_t* status = (int32_t*)malloc((size_t)E * sizeof(int32_t));
    int32_t* status_or = (int32_t*)calloc((size_t)E, sizeof(int32_t));
    int32_t* status_whole = (int32_t*)calloc((size_t)E, sizeof(int32_t));
    if (!whole || !pieces || !part || !forcing || !st_whole || !st_pieces || !status || !status_or || !status_whole) { fprintf(stderr, "host alloc failed\n"); return 1; }
    unsigned long long rhs[3] = {0, 0, 0};
    int flagged_whole = 0;
    for (int r = 0; r < 3; ++r) {
        const int d0 = first[r], n = days[r];
        const simplyp_dims dims = {E, S, n, 1};
        memcpy(forcing, P + d0, (size_t)n * sizeof(double));                  /* [1][2][n]: rows P, PET of this run's days */
        memcpy(forcing + n, PET + d0, (size_t)n * sizeof(double));
        CHECK(simplyp_memcpy_h2d(ctx, d_forcing, forcing, (int64_t)((size_t)2 * n * sizeof(double))));
        CHECK(simplyp_memcpy_h2d(ctx, d_doy, doy + d0, (int64_t)((size_t)n * sizeof(int32_t))));
        /* one-shot: consumed by the run that follows */
        if (r == 0) CHECK(simplyp_set_state(ctx, NULL, d_state_whole));
        if (r == 1) CHECK(simplyp_set_state(ctx, NULL, d_state));
        if (r == 2) CHECK(simplyp_set_state(ctx, d_state, d_state));
        simplyp_stats stats;
        CHECK(simplyp_run(ctx, &dims, &opts, d_forcing, d_doy, NULL, NULL, d_mp, d_rp, up_ptr, NULL, NULL, 0, d_out, d_status, NULL, NULL,
                          &stats));
        rhs[r] = (unsigned long long)stats.rhs_evals;
        CHECK(simplyp_memcpy_d2h(ctx, part, d_out, simplyp_out_bytes(&dims, &opts, 1)));
        CHECK(simplyp_memcpy_d2h(ctx, status, d_status, (int64_t)((size_t)E * sizeof(int32_t))));
        for (int c = 0; c < N_COLS; ++c)
            memcpy((r == 0 ? whole : pieces) + ((size_t)c * D + d0) * row, part + (size_t)c * n * row, (size_t)n * row * sizeof(double));
        for (int e = 0; e < E; ++e) {
            if (r == 0) { status_whole[e] = status[e]; flagged_whole += status[e] != 0; }
            else status_or[e] |= status[e];                                   /* the status of a run in pieces: OR over the pieces */
        }
        if (r == 0) CHECK(simplyp_memcpy_d2h(ctx, st_whole, d_state_whole, state_bytes));
    }
    CHECK(simplyp_memcpy_d2h(ctx, st_pieces, d_state, state_bytes));
    int status_differs = 0;
    for (int e = 0; e < E; ++e) status_differs += status_whole[e] != status_or[e];

    const int table_equal = memcmp(whole, pieces, (size_t)N_COLS * D * row * sizeof(double)) == 0;
    const int state_equal = memcmp(st_whole, st_pieces, (size_t)state_bytes) == 0;
    const int rhs_equal = rhs[0] == rhs[1] + rhs[2];
    printf("E=%d D=%d cut=%d flagged=%d rhs_evals=%llu = %llu + %llu\n", E, D, D1, flagged_whole, rhs[0], rhs[1], rhs[2]);
    printf("member %d: Qr_EndOfDay %.9f mm/d, next trial step %.6f d at the end\n", E - 1,
           st_whole[(size_t)SIMPLYP_STATE_QR * E + (E - 1)], st_whole[(size_t)SIMPLYP_STATE_H_NEXT * E + (E - 1)]);
    printf("table %s, state %s, status %s, rhs_evals %s\n", table_equal ? "identical" : "DIFFERS", state_equal ? "identical" : "DIFFERS",
           status_differs ? "DIFFERS" : "identical", rhs_equal ? "identical" : "DIFFER");

    simplyp_device_free(ctx, d_forcing); simplyp_device_free(ctx, d_doy); simplyp_device_free(ctx, d_mp); simplyp_device_free(ctx, d_rp);
    simplyp_device_free(ctx, d_out); simplyp_device_free(ctx, d_status); simplyp_device_free(ctx, d_state_whole); simplyp_device_free(ctx, d_state);
    free(P); free(PET); free(doy); free(mp); free(rp); free(whole); free(pieces); free(part); free(forcing);
    free(st_whole); free(st_pieces); free(status); free(status_or); free(status_whole);
    simplyp_ctx_destroy(ctx);
    return (table_equal && state_equal && rhs_equal && !status_differs) ? 0 : 4;
}
