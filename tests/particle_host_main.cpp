// Driver of tests/test_particle_host.py: the integer rules of simplyp_amd/csrc/simplyp_resample.h, called from plain host C++
// (built with AddressSanitizer and UBSan by the test).  Reads one case per line from stdin, writes one line per case.
//   mul a b              -> hi lo of the 128-bit product
//   offset x T           -> r
//   quantise w           -> q                                   (w a C hex float)
//   resample r E q_0 ..  -> the E ancestors                     (r: the offset, given by the caller)
//   uniform r E q        -> E, then the count of particles whose ancestor is not themselves, the first and the last ancestor
//                           (every q_i = q: what 2^22 particles are checked with)
// Integers are decimal and unsigned, up to 2^64 - 1.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../simplyp_amd/csrc/simplyp_resample.h"

namespace rs = simplyp_resample;

static uint64_t u64(std::istream& in)
{
    std::string w;
    in >> w;
    return strtoull(w.c_str(), nullptr, 10);
}

// the inclusive prefix sums, then every particle's ancestor
static std::vector<int32_t> ancestors(const std::vector<uint64_t>& q, uint64_t r)
{
    const int32_t E = (int32_t)q.size();
    std::vector<uint64_t> C(q.size());
    uint64_t c = 0;
    for (size_t i = 0; i < q.size(); ++i) { c += q[i]; C[i] = c; }
    std::vector<int32_t> a(q.size());
    for (int32_t k = 0; k < E; ++k) a[k] = rs::ancestor(C.data(), E, k, c, r);
    return a;
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        if (what == "mul") {
            const uint64_t a = u64(in), b = u64(in);
            const rs::U128 p = rs::mul_64x64(a, b);
            std::cout << p.hi << " " << p.lo;
        } else if (what == "offset") {
            const uint64_t x = u64(in), T = u64(in);
            std::cout << rs::offset(x, T);
        } else if (what == "quantise") {
            std::string w;
            in >> w;
            std::cout << rs::quantise(strtod(w.c_str(), nullptr));
        } else if (what == "resample") {
            const uint64_t r = u64(in);
            std::vector<uint64_t> q((size_t)u64(in));
            for (uint64_t& x : q) x = u64(in);
            const std::vector<int32_t> a = ancestors(q, r);
            for (size_t k = 0; k < a.size(); ++k) std::cout << (k ? " " : "") << a[k];
        } else if (what == "uniform") {
            const uint64_t r = u64(in), E = u64(in), each = u64(in);
            const std::vector<int32_t> a = ancestors(std::vector<uint64_t>((size_t)E, each), r);
            long long moved = 0;
            for (size_t k = 0; k < a.size(); ++k) moved += a[k] != (int32_t)k;
            std::cout << a.size() << " " << moved << " " << a.front() << " " << a.back();
        } else {
            std::cout << "unknown case";
        }
        std::cout << "\n";
    }
    return 0;
}
