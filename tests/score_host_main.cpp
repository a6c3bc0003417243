// Driver of tests/test_score_host.py: the rules of simplyp_amd/csrc/simplyp_score.h, called from plain host C++ (built with
// AddressSanitizer and UBSan by the test).  Reads one case per line from stdin, writes one line per case:
//   "<rc> <values ...>" when the rule accepts, "<rc> <message>" when it rejects.
// Observations and table values are C hex floats, weights and counts decimal integers; "null" stands for a NULL array.
//   row <y> <n> <x ...> <null | n w ...> <null | n flags ...>  -> the bits of abs_err and spread, below, at_or_below, T
//   terms <x> <y> <q> <lo> <hi> <C> <T>                        -> the bits of abs_err_term(x, y, q, T) and spread_term(lo, hi, C, T)
//   check <E> <n_rows> <table?> <y?> <sums?> <counts?>         (the flags: 1 = a pointer, 0 = NULL)
//   obs <n> <y ...>                                            -> the scored rows
//   chunk <n_scored> <row_bytes> <budget> <env | null>         -> rows per chunk
//   pit <below> <at_or_below> <T>                              -> the bits of the mid-point
//   hist <n_bins> <T> <n> <below at_or_below ...>              -> the bits of the n_bins counts
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../simplyp_amd/csrc/simplyp_score.h"

namespace ss = simplyp_score;

static const char* ME = "entry_under_test";

static std::string word(std::istream& in)
{
    std::string w;
    in >> w;
    return w;
}

static double real(std::istream& in) { return strtod(word(in).c_str(), nullptr); }
static uint64_t integer(std::istream& in) { return strtoull(word(in).c_str(), nullptr, 10); }

static uint64_t bits(double v)
{
    uint64_t b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what = word(in), msg;
        int rc = 0;
        std::ostringstream keep;
        if (what == "row") {
            const double y = real(in);
            std::vector<double> x((size_t)integer(in));
            for (double& v : x) v = real(in);
            std::vector<uint64_t> w;
            std::vector<uint8_t> inc;
            std::string n = word(in);
            const bool have_w = n != "null";
            if (have_w) {
                w.resize((size_t)atoll(n.c_str()));
                for (uint64_t& v : w) v = integer(in);
            }
            n = word(in);
            const bool have_inc = n != "null";
            if (have_inc) {
                inc.resize((size_t)atoll(n.c_str()));
                for (uint8_t& v : inc) v = (uint8_t)integer(in);
            }
            if ((have_w && w.size() != x.size()) || (have_inc && inc.size() != x.size())) { rc = 98; msg = "lengths differ"; }
            else {
                const ss::RowScore s = ss::score_row(x.data(), have_w ? w.data() : nullptr, have_inc ? inc.data() : nullptr, (int)x.size(), y);
                keep << " " << bits(s.abs_err) << " " << bits(s.spread) << " " << s.below << " " << s.at_or_below << " " << s.T;
            }
        } else if (what == "terms") {
            const double x = real(in), y = real(in);
            const uint64_t q = integer(in);
            const double lo = real(in), hi = real(in);
            const uint64_t C = integer(in), T = integer(in);
            keep << " " << bits(ss::abs_err_term(x, y, q, T)) << " " << bits(ss::spread_term(lo, hi, C, T));
        } else if (what == "check") {
            const long long E = atoll(word(in).c_str()), n_rows = atoll(word(in).c_str());
            const bool table = integer(in) != 0, y = integer(in) != 0, sums = integer(in) != 0, counts = integer(in) != 0;
            const int there = 0;
            rc = ss::check_table(ME, E, n_rows, table ? &there : nullptr, y ? &there : nullptr, sums ? &there : nullptr,
                                 counts ? &there : nullptr, msg);
        } else if (what == "obs") {
            std::vector<double> y((size_t)integer(in));
            for (double& v : y) v = real(in);
            std::vector<int64_t> rows;
            rc = ss::scored_rows(ME, y.data(), (int64_t)y.size(), rows, msg);
            for (int64_t r : rows) keep << " " << r;
        } else if (what == "chunk") {
            const int64_t n_scored = (int64_t)integer(in);
            const uint64_t row_bytes = integer(in), budget = integer(in);
            const std::string env = word(in);
            keep << " " << ss::chunk_rows(n_scored, row_bytes, budget, env == "null" ? nullptr : env.c_str());
        } else if (what == "pit") {
            const uint64_t lo = integer(in), hi = integer(in), T = integer(in);
            keep << " " << bits(ss::pit(lo, hi, T));
        } else if (what == "hist") {
            const int n_bins = (int)integer(in);
            const uint64_t T = integer(in);
            const size_t n = (size_t)integer(in);
            std::vector<double> hist((size_t)n_bins, 0.0);
            for (size_t i = 0; i < n; ++i) {
                const uint64_t lo = integer(in), hi = integer(in);
                ss::pit_histogram_add(lo, hi, T, n_bins, hist.data());
            }
            for (double h : hist) keep << " " << bits(h);
        } else {
            rc = 99;
            msg = "unknown case " + what;
        }
        std::cout << rc << (rc ? " " + msg : keep.str()) << "\n";
    }
    return 0;
}
