// Driver of tests/test_nsga2_host.py: the variation and the argument checks of simplyp_amd/csrc/simplyp_nsga2.h, called from plain
// host C++ (built with -ffp-contract=off under AddressSanitizer and UBSan by the test).  Reads one case per line from stdin,
// writes one line per case: "<rc> <values ...>" when the rule accepts, "<rc> <message>" when it rejects.  Doubles are C hex
// floats both ways; a flag says whether a pointer is there (1) or NULL (0).
//   vary <x1> <x2> <lo> <hi> <k_c> <k_m> <p_mut> <cross> <u> <u_take> <u_swap> <u_do_a> <u_a> <u_do_b> <u_b>  -> child A, child B
//   powk <x> <k>, rootk <x> <k>                                                   -> the value
//   init <N> <n_dim> <theta?>
//   offspring <N> <n_dim> <k_c> <k_m> <p_cross> <p_mut> <theta?> <rank?> <crowd?> <child?>
//   crowding <n> <M> <obj?> <rank?> <crowd?> <null | count sense ...>
//   select <n> <N> <rank?> <crowd?> <position?> <survivor?> <n_rows> <rows_in?> <rows_out?>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../simplyp_amd/csrc/simplyp_nsga2.h"

namespace sn = simplyp_nsga2;

static const char* ME = "entry_under_test";

static std::string word(std::istream& in)
{
    std::string w;
    in >> w;
    return w;
}

static double real(std::istream& in) { return strtod(word(in).c_str(), nullptr); }
static long long integer(std::istream& in) { return strtoll(word(in).c_str(), nullptr, 10); }

static std::string hexf(double v)
{
    char buf[64];
    snprintf(buf, sizeof buf, "%a", v);
    return buf;
}

int main()
{
    std::string line;
    const int there = 0;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what = word(in), msg;
        int rc = 0;
        std::ostringstream keep;
        auto ptr = [&]() -> const void* { return integer(in) != 0 ? &there : nullptr; };
        if (what == "vary") {
            const double x1 = real(in), x2 = real(in), lo = real(in), hi = real(in);
            const int k_c = (int)integer(in), k_m = (int)integer(in);
            const double p_mut = real(in);
            const bool cross = integer(in) != 0;
            double u[7];
            for (double& v : u) v = real(in);
            double a, b;
            sn::vary_dim(x1, x2, lo, hi, k_c, k_m, p_mut, cross, u[0], u[1], u[2], u[3], u[4], u[5], u[6], a, b);
            keep << " " << hexf(a) << " " << hexf(b);
        } else if (what == "powk" || what == "rootk") {
            const double x = real(in);
            const int k = (int)integer(in);
            keep << " " << hexf(what == "powk" ? sn::powk(x, k) : sn::rootk(x, k));
        } else if (what == "init") {
            const long long N = integer(in), n_dim = integer(in);
            rc = sn::check_init(ME, N, n_dim, ptr(), msg);
        } else if (what == "offspring") {
            const long long N = integer(in), n_dim = integer(in), k_c = integer(in), k_m = integer(in);
            const double p_cross = real(in), p_mut = real(in);
            const void* theta = ptr();
            const void* rank = ptr();
            const void* crowd = ptr();
            const void* child = ptr();
            rc = sn::check_offspring(ME, N, n_dim, k_c, k_m, p_cross, p_mut, theta, rank, crowd, child, msg);
        } else if (what == "crowding") {
            const long long n = integer(in), M = integer(in);
            const void* obj = ptr();
            const void* rank = ptr();
            const void* crowd = ptr();
            std::vector<int32_t> sense;
            const std::string count = word(in);
            const bool have = count != "null";
            if (have) {
                sense.resize((size_t)atoll(count.c_str()));
                for (int32_t& v : sense) v = (int32_t)integer(in);
            }
            if (have && M >= 1 && M <= sn::MAX_OBJ && sense.size() < (size_t)M) { rc = 98; msg = "too few senses"; }
            else rc = sn::check_crowding(ME, n, M, obj, have ? sense.data() : nullptr, rank, crowd, msg);
        } else if (what == "select") {
            const long long n = integer(in), N = integer(in);
            const void* rank = ptr();
            const void* crowd = ptr();
            const void* position = ptr();
            const void* survivor = ptr();
            const long long n_rows = integer(in);
            const void* rows_in = ptr();
            const void* rows_out = ptr();
            rc = sn::check_select(ME, n, N, rank, crowd, position, survivor, n_rows, rows_in, rows_out, msg);
        } else {
            rc = 99;
            msg = "unknown case " + what;
        }
        std::cout << rc << (rc ? " " + msg : keep.str()) << "\n";
    }
    return 0;
}
