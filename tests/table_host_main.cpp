// Driver of tests/test_table_host.py: the rules of simplyp_amd/csrc/simplyp_table.h, called from plain host C++ (built with
// AddressSanitizer and UBSan by the test).  Reads one case per line from stdin, writes one line per case:
//   "<rc> <values ...>" when the rule accepts, "<rc> <message>" when it rejects.
// Numbers are decimal integers or C hex floats; "null" stands for a NULL array.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../simplyp_amd/csrc/simplyp_table.h"

namespace st = simplyp_table;

static const char* ME = "entry_under_test";

static double num(std::istream& in)
{
    std::string w;
    in >> w;
    return strtod(w.c_str(), nullptr);
}

// "null", or a count followed by that many numbers
template <class T>
static bool list(std::istream& in, std::vector<T>& v)
{
    std::string w;
    in >> w;
    if (w == "null") return false;
    v.resize((size_t)atoll(w.c_str()));
    for (T& x : v) x = (T)num(in);
    return true;
}

template <class T>
static void show(const std::vector<T>& v)
{
    std::cout << " " << v.size();
    for (const T& x : v) std::cout << " " << (long long)x;
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what, msg;
        in >> what;
        int rc = 0;
        std::ostringstream keep;
        std::streambuf* out = std::cout.rdbuf(keep.rdbuf());       // a case's values are printed only if it was accepted
        if (what == "ranks") {
            const double q = num(in);
            const long long n = (long long)num(in);
            long long lo = -1, hi = -1;
            st::linear_ranks(q, n, lo, hi);
            std::cout << " " << lo << " " << hi;
        } else if (what == "probs") {
            const int max_K = (int)num(in), K = (int)num(in);
            std::vector<double> q;
            const bool have = list(in, q);
            rc = st::check_probabilities(ME, have ? q.data() : nullptr, K, max_K, msg);
        } else if (what == "view") {
            simplyp_dims dims = {};
            dims.E = (int)num(in); dims.S = (int)num(in); dims.D = (int)num(in);
            const uint32_t mask = (uint32_t)num(in), legal = (uint32_t)num(in);
            const int n_out = (int)num(in);
            std::vector<int32_t> reaches;
            const bool have = list(in, reaches);
            st::View t;
            rc = st::view(ME, dims, mask, legal, have ? reaches.data() : nullptr, n_out, t, msg);
            std::cout << " " << t.E << " " << t.S << " " << t.D << " " << t.R;
            show(t.reach_of);
        } else if (what == "slots") {
            const uint32_t mask = (uint32_t)num(in);
            const bool wb = num(in) != 0.0;
            int col[4];
            const bool all = st::flux_slots(mask, wb ? st::WB_FLUX_COLS : st::FLUX_COLS, col);
            std::cout << " " << (all ? 1 : 0) << " " << col[0] << " " << col[1] << " " << col[2] << " " << col[3];
        } else if (what == "series") {
            const int max_series = (int)num(in);
            const uint32_t mask = (uint32_t)num(in);
            const int R = (int)num(in);
            const bool have_f = num(in) != 0.0, have_rp = num(in) != 0.0;
            const int n_series = (int)num(in);
            std::vector<int32_t> ids;
            const bool have = list(in, ids);
            st::Series s;
            std::vector<int> code((size_t)max_series, 0);
            std::vector<uint32_t> raw((size_t)max_series, 0u);
            rc = st::resolve_series(ME, have ? ids.data() : nullptr, n_series, max_series, mask, R, have_f, have_rp, code.data(),
                                    raw.data(), s, msg);
            if (rc == 0) { code.resize((size_t)n_series); raw.resize((size_t)n_series); }
            std::cout << " " << (s.derived ? 1 : 0) << " " << (long long)s.loads;
            show(code);
            show(raw);
        } else if (what == "periods") {
            const int D = (int)num(in), P = (int)num(in);
            std::vector<int32_t> pod, days, day_ptr;
            const bool have = list(in, pod);
            rc = st::period_days(ME, have ? pod.data() : nullptr, D, P, days, day_ptr, msg);
            show(days);
            show(day_ptr);
        } else if (what == "box") {
            const int n_dim = (int)num(in);
            const bool have_mp = num(in) != 0.0, have_f = num(in) != 0.0;
            std::vector<double> lo, hi;
            std::vector<int32_t> target;
            list(in, lo); list(in, hi); list(in, target);
            std::vector<double> g_lo(n_dim, -1.0), g_hi(n_dim, -1.0);
            std::vector<int> g_target(n_dim, -99);
            rc = st::check_box(ME, n_dim, lo.data(), hi.data(), target.data(), have_mp, have_f, g_lo.data(), g_hi.data(),
                               g_target.data(), msg);
            for (int d = 0; d < n_dim; ++d) std::cout << " " << (g_lo[d] == lo[d] && g_hi[d] == hi[d] && g_target[d] == target[d] ? 1 : 0);
        } else {
            rc = 99;
            msg = "unknown case " + what;
        }
        std::cout.rdbuf(out);
        std::cout << rc << (rc ? " " + msg : keep.str()) << "\n";
    }
    return 0;
}
