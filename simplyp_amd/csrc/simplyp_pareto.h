// simplyp_pareto.h -- Pareto dominance among the members of an ensemble, in plain C++ (no HIP, no context): the order-preserving
// key of an objective, who takes part, the O(n^2) reference of the three outputs, and what simplyp_pareto's arguments must
// satisfy.  The entry of simplyp_hip.hip and a host program (tests/pareto_host_main.cpp) share it; simplyp_amd/pareto.py states
// the same rule with NumPy and Python integers.
//
// obj[M][E] fp64 (E the fastest axis, in the table's column order), sense[M] in {+1 larger is better, -1 smaller is better}:
//   a member takes part iff its include flag is set (include == NULL: all) and none of its M objectives is NaN; +-inf are
//   ordinary values, -0.0 and +0.0 are equal; n = the members that take part
//   with y = sense x, a dominates b iff y_a[m] >= y_b[m] for every m and y_a[m] > y_b[m] for some m; equal members do not
//   dominate each other.  Dominance is invariant under a strictly increasing map of an objective, so the comparisons are made
//   on 64-bit keys: simplyp_quantiles' key with the sense folded in and the two zeros made one
//   dominated_by[i] = participants that dominate i;  dominates[i] = participants that i dominates
//   rank[i] = 0 when nobody dominates i, else 1 + the largest rank among its dominators: the longest chain of dominators above
//             it, which is the index of the front it leaves with when fronts are peeled off one at a time (NSGA-II's rank)
//   a member that does not take part gets SIMPLYP_PARETO_EXCLUDED in all three; with max_fronts = F > 0 a participant of
//   rank >= F gets SIMPLYP_PARETO_UNRANKED as its rank, its counts stay exact
// Integer arithmetic on exact comparisons: every correct implementation returns the same integers.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "simplyp_table.h"

namespace simplyp_pareto_rules {

constexpr int MAX_OBJ = SIMPLYP_PARETO_MAX_OBJ;
constexpr int MAX_E = 1 << 24;                     // n^2 pair tests stay far inside int64, the j splits inside one grid axis

// y = sense x as an unsigned integer that keeps y's order; -0.0 and +0.0 give one key.  x must not be NaN.
inline uint64_t key(double x, int sense)
{
    uint64_t b;
    std::memcpy(&b, &x, sizeof b);
    if (sense < 0) b ^= 0x8000000000000000ull;
    if (b == 0x8000000000000000ull) b = 0;
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// simplyp_pareto's arguments, before anything is touched.
inline int check_args(const char* me, int64_t E, int64_t M, const void* obj, const int32_t* sense, int64_t max_fronts,
                      const void* dominated_by, const void* dominates, const void* rank, std::string& msg)
{
    if (E < 1 || E > MAX_E) return simplyp_table::reject(msg, me, "E must be in [1, 2^24] (got %lld)", (long long)E);
    if (M < 1 || M > MAX_OBJ) return simplyp_table::reject(msg, me, "M must be in [1, %d] (got %lld)", MAX_OBJ, (long long)M);
    if (!obj) return simplyp_table::reject(msg, me, "obj must not be NULL");
    if (!sense) return simplyp_table::reject(msg, me, "sense must not be NULL");
    for (int m = 0; m < M; ++m)
        if (sense[m] != 1 && sense[m] != -1) return simplyp_table::reject(msg, me, "sense[%d] must be +1 or -1 (got %d)", m, (int)sense[m]);
    if (max_fronts < 0) return simplyp_table::reject(msg, me, "max_fronts must be >= 0 (got %lld)", (long long)max_fronts);
    if (!dominated_by && !dominates && !rank) return simplyp_table::reject(msg, me, "dominated_by, dominates and rank are all NULL: nothing to compute");
    return SIMPLYP_OK;
}

struct Result {
    std::vector<int32_t> dominated_by, dominates, rank;     // [E] member order
    int64_t pair_tests = 0;                                 // n^2 of the counts, front x remaining of the peeling
    int32_t n_used = 0, n_fronts = 0, n_front0 = 0, n_unranked = 0;
};

// The reference: all pairs for the counts, then fronts peeled one at a time.  Column j of obj holds member member_of_slot[j]
// (NULL: j); include is in member order.
inline Result reference(const double* obj, const int32_t* sense, int M, int E, const int32_t* member_of_slot, const uint8_t* include,
                        int max_fronts)
{
    Result r;
    r.dominated_by.assign((size_t)E, SIMPLYP_PARETO_EXCLUDED);
    r.dominates.assign((size_t)E, SIMPLYP_PARETO_EXCLUDED);
    r.rank.assign((size_t)E, SIMPLYP_PARETO_EXCLUDED);
    std::vector<int> member_of;                             // the participants in column order
    std::vector<uint64_t> k;                                // [n][M]
    for (int j = 0; j < E; ++j) {
        const int mem = member_of_slot ? member_of_slot[j] : j;
        bool ok = mem >= 0 && mem < E && (!include || include[mem]);
        for (int m = 0; m < M && ok; ++m) ok = !(obj[(size_t)m * E + j] != obj[(size_t)m * E + j]);
        if (!ok) continue;
        member_of.push_back(mem);
        for (int m = 0; m < M; ++m) k.push_back(key(obj[(size_t)m * E + j], sense[m]));
    }
    const int n = (int)member_of.size();
    r.n_used = n;
    auto dominates = [&](int a, int b) {                    // does participant a dominate participant b?
        bool ge = true, le = true;
        for (int m = 0; m < M; ++m) {
            ge = ge && k[(size_t)a * M + m] >= k[(size_t)b * M + m];
            le = le && k[(size_t)a * M + m] <= k[(size_t)b * M + m];
        }
        return ge && !le;
    };
    std::vector<int32_t> by((size_t)n, 0), of((size_t)n, 0);
    for (int a = 0; a < n; ++a)
        for (int b = 0; b < n; ++b)
            if (dominates(a, b)) { ++of[a]; ++by[b]; }
    r.pair_tests = (int64_t)n * n;
    std::vector<int32_t> rank((size_t)n, SIMPLYP_PARETO_UNRANKED), left(by);
    std::vector<int> alive((size_t)n), front, next;
    for (int i = 0; i < n; ++i) alive[i] = i;
    while (!alive.empty() && (max_fronts == 0 || r.n_fronts < max_fronts)) {
        front.clear(); next.clear();
        for (int i : alive) (left[i] == 0 ? front : next).push_back(i);
        for (int i : front) rank[i] = r.n_fronts;
        if (r.n_fronts == 0) r.n_front0 = (int32_t)front.size();
        ++r.n_fronts;
        if (!next.empty() && (max_fronts == 0 || r.n_fronts < max_fronts)) {      // (nothing is peeled after the last front asked for)
            r.pair_tests += (int64_t)front.size() * (int64_t)next.size();
            for (int i : next)
                for (int f : front) if (dominates(f, i)) --left[i];
        }
        alive.swap(next);
    }
    r.n_unranked = (int32_t)alive.size();
    for (int i = 0; i < n; ++i) {
        r.dominated_by[member_of[i]] = by[i];
        r.dominates[member_of[i]] = of[i];
        r.rank[member_of[i]] = rank[i];
    }
    return r;
}

}  // namespace simplyp_pareto_rules
