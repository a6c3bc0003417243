// Driver of tests/test_weighted_host.py: the rules of simplyp_amd/csrc/simplyp_weighted.h, called from plain host C++ (built
// with AddressSanitizer and UBSan by the test).  Reads one case per line from stdin, writes one line per case:
//   "<rc> <values ...>" when the rule accepts, "<rc> <message>" when it rejects.
// Probabilities and table values are C hex floats, weights and sums decimal integers; "null" stands for a NULL array.
//   thr <p> <T>                                          -> t
//   row <p> <n> <x ...> <n> <w ...> <null | n flags ...> -> the selected value's bits, T
//   check <E> <n_rows> <table?> <weights?> <order_stats?> <K> <null | n q ...>   (the flags: 1 = a pointer, 0 = NULL)
//   bad <n_bad>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../simplyp_amd/csrc/simplyp_weighted.h"

namespace sw = simplyp_weighted;

static const char* ME = "entry_under_test";

static std::string word(std::istream& in)
{
    std::string w;
    in >> w;
    return w;
}

static double real(std::istream& in) { return strtod(word(in).c_str(), nullptr); }
static uint64_t integer(std::istream& in) { return strtoull(word(in).c_str(), nullptr, 10); }

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what = word(in), msg;
        int rc = 0;
        std::ostringstream keep;
        if (what == "thr") {
            const double p = real(in);
            const uint64_t T = integer(in);
            keep << " " << sw::weighted_threshold(p, T);
        } else if (what == "row") {
            const double p = real(in);
            std::vector<double> x((size_t)integer(in));
            for (double& v : x) v = real(in);
            std::vector<uint64_t> w((size_t)integer(in));
            for (uint64_t& v : w) v = integer(in);
            std::vector<uint8_t> inc;
            const std::string flags = word(in);
            const bool have = flags != "null";
            if (have) {
                inc.resize((size_t)atoll(flags.c_str()));
                for (uint8_t& v : inc) v = (uint8_t)integer(in);
            }
            if (x.size() != w.size() || (have && inc.size() != x.size())) { rc = 98; msg = "lengths differ"; }
            else {
                const double v = sw::select_row(x.data(), w.data(), have ? inc.data() : nullptr, (int)x.size(), p);
                uint64_t bits;
                std::memcpy(&bits, &v, sizeof bits);
                keep << " " << bits << " " << sw::row_total(w.data(), have ? inc.data() : nullptr, (int)x.size());
            }
        } else if (what == "check") {
            const long long E = atoll(word(in).c_str()), n_rows = atoll(word(in).c_str());
            const bool table = integer(in) != 0, weights = integer(in) != 0, order = integer(in) != 0;
            const int K = atoi(word(in).c_str());
            std::vector<double> q;
            const std::string n = word(in);
            const bool have = n != "null";
            if (have) {
                q.resize((size_t)atoll(n.c_str()));
                for (double& v : q) v = real(in);
            }
            const int there = 0;
            rc = sw::check_table(ME, E, n_rows, table ? &there : nullptr, weights ? &there : nullptr, have ? q.data() : nullptr, K,
                                 order ? &there : nullptr, msg);
        } else if (what == "bad") {
            rc = sw::check_weights(ME, (int)integer(in), msg);
        } else {
            rc = 99;
            msg = "unknown case " + what;
        }
        std::cout << rc << (rc ? " " + msg : keep.str()) << "\n";
    }
    return 0;
}
