// Driver of tests/test_pareto_host.py: the rules of simplyp_amd/csrc/simplyp_pareto.h, called from plain host C++ (built with
// AddressSanitizer and UBSan by the test).  Reads one case per line from stdin, writes one line per case:
//   "<rc> <values ...>" when the rule accepts, "<rc> <message>" when it rejects.
// Objectives are C hex floats ("nan", "inf", "-inf" too); "null" stands for a NULL array.
//   key <x> <sense>                                   -> the key
//   ref <M> <E> <max_fronts> <sense x M> <obj x M*E> <null | E member_of_slot ...> <null | E flags ...>
//       -> n_used n_fronts n_front0 n_unranked pair_tests, then dominated_by x E, dominates x E, rank x E
//   check <E> <M> <obj?> <max_fronts> <dominated_by?> <dominates?> <rank?> <null | n sense ...>   (the flags: 1 = a pointer, 0 = NULL)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../simplyp_amd/csrc/simplyp_pareto.h"

namespace sp = simplyp_pareto_rules;

static const char* ME = "entry_under_test";

static std::string word(std::istream& in)
{
    std::string w;
    in >> w;
    return w;
}

static double real(std::istream& in) { return strtod(word(in).c_str(), nullptr); }
static long long integer(std::istream& in) { return strtoll(word(in).c_str(), nullptr, 10); }

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what = word(in), msg;
        int rc = 0;
        std::ostringstream keep;
        if (what == "key") {
            const double x = real(in);
            keep << " " << sp::key(x, (int)integer(in));
        } else if (what == "ref") {
            const int M = (int)integer(in), E = (int)integer(in), F = (int)integer(in);
            std::vector<int32_t> sense((size_t)M);
            for (int32_t& v : sense) v = (int32_t)integer(in);
            std::vector<double> obj((size_t)M * E);
            for (double& v : obj) v = real(in);
            std::vector<int32_t> mos;
            std::vector<uint8_t> inc;
            std::string w = word(in);
            const bool have_mos = w != "null";
            if (have_mos) {
                mos.resize((size_t)atoll(w.c_str()));
                for (int32_t& v : mos) v = (int32_t)integer(in);
            }
            w = word(in);
            const bool have_inc = w != "null";
            if (have_inc) {
                inc.resize((size_t)atoll(w.c_str()));
                for (uint8_t& v : inc) v = (uint8_t)integer(in);
            }
            if ((have_mos && mos.size() != (size_t)E) || (have_inc && inc.size() != (size_t)E)) { rc = 98; msg = "lengths differ"; }
            else if ((rc = sp::check_args(ME, E, M, obj.data(), sense.data(), F, &rc, &rc, &rc, msg)) == 0) {
                const sp::Result r = sp::reference(obj.data(), sense.data(), M, E, have_mos ? mos.data() : nullptr,
                                                   have_inc ? inc.data() : nullptr, F);
                keep << " " << r.n_used << " " << r.n_fronts << " " << r.n_front0 << " " << r.n_unranked << " " << r.pair_tests;
                for (const std::vector<int32_t>* v : {&r.dominated_by, &r.dominates, &r.rank})
                    for (int32_t x : *v) keep << " " << x;
            }
        } else if (what == "check") {
            const long long E = integer(in), M = integer(in);
            const bool obj = integer(in) != 0;
            const long long F = integer(in);
            const bool by = integer(in) != 0, of = integer(in) != 0, rank = integer(in) != 0;
            std::vector<int32_t> sense;
            const std::string n = word(in);
            const bool have = n != "null";
            if (have) {
                sense.resize((size_t)atoll(n.c_str()));
                for (int32_t& v : sense) v = (int32_t)integer(in);
            }
            if (have && M >= 1 && M <= sp::MAX_OBJ && sense.size() < (size_t)M) { rc = 98; msg = "too few senses"; }
            else {
                const int there = 0;
                rc = sp::check_args(ME, E, M, obj ? &there : nullptr, have ? sense.data() : nullptr, F, by ? &there : nullptr,
                                    of ? &there : nullptr, rank ? &there : nullptr, msg);
            }
        } else {
            rc = 99;
            msg = "unknown case " + what;
        }
        std::cout << rc << (rc ? " " + msg : keep.str()) << "\n";
    }
    return 0;
}
