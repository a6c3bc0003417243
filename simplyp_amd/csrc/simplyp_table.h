// simplyp_table.h -- the rules the reductions over a daily table share, in plain C++ (no HIP, no context): what a table is
// (sizes, output reaches, column slots), what a series id means, what a probability is and which ranks numpy's 'linear'
// method takes for it, how period_of_day becomes day lists, and what a prior box with its targets must satisfy.  One
// definition each; the entries of simplyp_hip.hip call them and keep only what differs between them.
//
// Every function returns SIMPLYP_OK or SIMPLYP_ERR_ARG and, on error, leaves a message in `msg` that begins with `me`, the
// name of the entry that was called.  Nothing here touches the device, so a rejected call has written nothing.
#pragma once

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/simplyp.h"

namespace simplyp_table {

constexpr int TARGET_F_TDP = -1, TARGET_NONE = -2;      // targets of a box dimension below the rows of member_params
constexpr uint32_t DAILY_COLUMNS = SIMPLYP_MASK_ALL | SIMPLYP_MASK_D_SNOW;     // the legal bits of a daily table's out_mask

__attribute__((format(printf, 3, 4))) inline int reject(std::string& msg, const char* me, const char* fmt, ...)
{
    char text[400];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(text, sizeof(text), fmt, ap);
    va_end(ap);
    msg = std::string(me) + ": " + text;
    return SIMPLYP_ERR_ARG;
}

// ---- the table ----------------------------------------------------------------------------------------------------------
struct View {
    int E = 0, S = 0, D = 0, R = 0;
    std::vector<int32_t> reach_of;      // [R] the reach of each output row
};

// A table [n_cols][D][R][E] written with `mask` (no bit outside `legal`) for `dims`; its rows are the S reaches in order
// (out_reaches == NULL) or the n_out_reaches listed.  The bounds on E, S and D are the caller's.
inline int view(const char* me, const simplyp_dims& dims, uint32_t mask, uint32_t legal, const int32_t* out_reaches,
                int32_t n_out_reaches, View& t, std::string& msg)
{
    if (mask == 0u || (mask & ~legal) != 0u) return reject(msg, me, "the mask must select 1..%d of the columns", __builtin_popcount(legal));
    t.E = dims.E; t.S = dims.S; t.D = dims.D;
    t.R = out_reaches ? n_out_reaches : t.S;
    if (t.R <= 0 || t.R > t.S) return reject(msg, me, "bad n_out_reaches");
    t.reach_of.resize(t.R);
    for (int r = 0; r < t.R; ++r) {
        t.reach_of[r] = out_reaches ? out_reaches[r] : r;
        if (t.reach_of[r] < 0 || t.reach_of[r] >= t.S) return reject(msg, me, "out_reaches[%d] out of range", r);
    }
    return SIMPLYP_OK;
}

// The discharge and the three daily fluxes: the columns every df_R series is built from.
constexpr int FLUX_COLS[4] = {SIMPLYP_OUT_QR, SIMPLYP_OUT_MSUS_FLUX, SIMPLYP_OUT_TDP_FLUX, SIMPLYP_OUT_PP_FLUX};
constexpr int WB_FLUX_COLS[4] = {SIMPLYP_WB_Q_CUMECS, SIMPLYP_WB_MSUS_FLUX, SIMPLYP_WB_TDP_FLUX, SIMPLYP_WB_PP_FLUX};

// The slot of column `c` among the columns of `mask`.
inline int slot_of(uint32_t mask, int c) { return __builtin_popcount(mask & ((1u << c) - 1u)); }

// The slots of the four columns `want` names; false when `mask` lacks one of them (the slots are set all the same).
inline bool flux_slots(uint32_t mask, const int (&want)[4], int (&col)[4])
{
    uint32_t need = 0u;
    for (int i = 0; i < 4; ++i) { need |= 1u << want[i]; col[i] = slot_of(mask, want[i]); }
    return (mask & need) == need;
}

// ---- series ids -----------------------------------------------------------------------------------------------------------
struct Series {
    bool derived = false;           // some series is a df_R series
    int64_t loads = 0;              // table values read per (day, reach, member), all series together
};

// series[i] is a column of `mask` or SIMPLYP_TQ_DERIVED + SIMPLYP_GOF_*; a derived series needs the four flux columns,
// f_tdp and reach_params.  R: the table's output reaches (a launch takes n_series * R as one grid dimension).  Writes into the
// kernel argument's arrays (room for max_series each): code[i] is what the kernels take -- >= 0 the column's slot, < 0 derived:
// -1 - SIMPLYP_GOF_* -- and id[i] (unless NULL) the id as passed.
inline int resolve_series(const char* me, const int32_t* series, int32_t n_series, int max_series, uint32_t mask, int R,
                          bool have_f_tdp, bool have_reach_params, int* code, uint32_t* id_out, Series& s, std::string& msg)
{
    if (n_series < 1 || n_series > max_series || !series)
        return reject(msg, me, "n_series must be in [1, %d] (got %d) and series not NULL", max_series, (int)n_series);
    if ((long long)n_series * R > 65535) return reject(msg, me, "n_series * n_out_reaches must not exceed 65535");
    int col[4];
    const bool fluxes = flux_slots(mask, FLUX_COLS, col);
    s = Series();
    for (int i = 0; i < n_series; ++i) {
        const int id = series[i];
        if (id >= 0 && id < SIMPLYP_N_OUT) {
            if (!((mask >> id) & 1u)) return reject(msg, me, "series[%d] = column %d is not in out_mask", i, id);
            code[i] = slot_of(mask, id);
            s.loads += 1;
        } else if (id >= SIMPLYP_TQ_DERIVED && id < SIMPLYP_TQ_DERIVED + SIMPLYP_N_GOF_VARS) {
            if (!fluxes)
                return reject(msg, me, "series[%d] is derived: out_mask must contain Qr, Msus_kg/day, TDP_kg/day and PP_kg/day", i);
            if (!have_f_tdp || !have_reach_params)
                return reject(msg, me, "series[%d] is derived: f_tdp and reach_params must not be NULL", i);
            const int var = id - SIMPLYP_TQ_DERIVED;
            code[i] = -1 - var;
            s.loads += var == SIMPLYP_GOF_Q ? 1 : var == SIMPLYP_GOF_TP ? 3 : 2;
            s.derived = true;
        } else {
            return reject(msg, me, "series[%d] = %d is neither a column nor SIMPLYP_TQ_DERIVED + a variable", i, id);
        }
        if (id_out) id_out[i] = (uint32_t)id;
    }
    return SIMPLYP_OK;
}

// ---- probabilities and ranks ----------------------------------------------------------------------------------------------
inline int check_probabilities(const char* me, const double* q, int32_t K, int max_K, std::string& msg)
{
    if (K < 1 || K > max_K) return reject(msg, me, "K must be in [1, %d] (got %d)", max_K, (int)K);
    if (!q) return reject(msg, me, "q must not be NULL");
    for (int k = 0; k < K; ++k)
        if (!(q[k] >= 0.0 && q[k] <= 1.0)) return reject(msg, me, "q[%d] = %g is not a probability in [0, 1]", k, q[k]);
    return SIMPLYP_OK;
}

// numpy's 'linear' indices of probability q among n >= 1 sorted elements: h = q (n - 1) in fp64, k_lo = floor(h),
// k_hi = min(k_lo + 1, n - 1).  This is the rule include/simplyp.h promises bit for bit.
inline void linear_ranks(double q, long long n, long long& k_lo, long long& k_hi)
{
    const double h = q * (double)(n - 1);
    k_lo = std::min<long long>(std::max<long long>((long long)std::floor(h), 0), n - 1);
    k_hi = std::min<long long>(k_lo + 1, n - 1);
}

// ---- periods ----------------------------------------------------------------------------------------------------------------
// The periods' day lists: days[day_ptr[p] .. day_ptr[p + 1]) are the days of period p, ascending.  period_of_day [D] holds
// -1 (the day takes part in no period) or a period in [0, P), and its non-negative entries do not decrease: a period is a day
// range with holes.  NULL: one period holding every day.
inline int period_days(const char* me, const int32_t* period_of_day, int D, int P, std::vector<int32_t>& days,
                       std::vector<int32_t>& day_ptr, std::string& msg)
{
    day_ptr.assign(P + 1, 0);
    days.clear();
    days.reserve((size_t)D);
    if (!period_of_day) {
        for (int d = 0; d < D; ++d) days.push_back(d);
        day_ptr[1] = D;
        return SIMPLYP_OK;
    }
    int last = 0;
    std::vector<int32_t> count(P, 0);
    for (int d = 0; d < D; ++d) {
        const int p = period_of_day[d];
        if (p < -1 || p >= P) return reject(msg, me, "period_of_day[%d] = %d is outside [-1, %d)", d, p, P);
        if (p < 0) continue;
        if (p < last) return reject(msg, me, "period_of_day decreases at day %d (%d after %d)", d, p, last);
        last = p;
        days.push_back(d);
        ++count[p];
    }
    for (int p = 0; p < P; ++p) day_ptr[p + 1] = day_ptr[p] + count[p];
    return SIMPLYP_OK;
}

// ---- the prior box ------------------------------------------------------------------------------------------------------------
// lo[d] < hi[d]; target[d] is a row of member_params, TARGET_F_TDP or TARGET_NONE, no row named twice, and what is named is
// there.  Copies the three into the kernel argument's arrays (each with room for n_dim entries).
inline int check_box(const char* me, int n_dim, const double* lo, const double* hi, const int32_t* target,
                     bool have_member_params, bool have_f_tdp, double* g_lo, double* g_hi, int* g_target, std::string& msg)
{
    if (!lo || !hi || !target) return reject(msg, me, "lo, hi and target must not be NULL");
    bool to_params = false, to_f_tdp = false;
    for (int d = 0; d < n_dim; ++d) {
        if (!(lo[d] < hi[d])) return reject(msg, me, "the box needs lo[%d] < hi[%d] (got %g, %g)", d, d, lo[d], hi[d]);
        if (target[d] < TARGET_NONE || target[d] >= SIMPLYP_NP_M)
            return reject(msg, me, "target[%d] = %d is outside [-2, %d)", d, (int)target[d], (int)SIMPLYP_NP_M);
        for (int e = 0; e < d; ++e)
            if (target[d] != TARGET_NONE && target[e] == target[d])
                return reject(msg, me, "target[%d] and target[%d] name the same row (%d)", e, d, (int)target[d]);
        to_params = to_params || target[d] >= 0;
        to_f_tdp = to_f_tdp || target[d] == TARGET_F_TDP;
    }
    if ((to_params && !have_member_params) || (to_f_tdp && !have_f_tdp))
        return reject(msg, me, "a target names member_params or f_tdp, which is NULL");
    for (int d = 0; d < n_dim; ++d) { g_lo[d] = lo[d]; g_hi[d] = hi[d]; g_target[d] = target[d]; }
    return SIMPLYP_OK;
}

// ---- (variable, output reach) pairs -------------------------------------------------------------------------------------------
// 1 <= n_pairs <= max_pairs; every pair names a goodness-of-fit variable and one of the table's R output reaches.  Copies the
// two lists into the kernel argument's arrays (each with room for max_pairs entries).
inline int check_pairs(const char* me, const int32_t* pair_var, const int32_t* pair_reach, int32_t n_pairs, int max_pairs, int R,
                       int* g_var, int* g_reach, std::string& msg)
{
    if (n_pairs < 1 || n_pairs > max_pairs) return reject(msg, me, "n_pairs must be in [1, %d] (got %d)", max_pairs, (int)n_pairs);
    for (int p = 0; p < n_pairs; ++p) {
        if (pair_var[p] < 0 || pair_var[p] >= SIMPLYP_N_GOF_VARS || pair_reach[p] < 0 || pair_reach[p] >= R)
            return reject(msg, me, "pair %d = (variable %d, output reach %d) is out of range", p, (int)pair_var[p], (int)pair_reach[p]);
        g_var[p] = pair_var[p]; g_reach[p] = pair_reach[p];
    }
    return SIMPLYP_OK;
}

}  // namespace simplyp_table
