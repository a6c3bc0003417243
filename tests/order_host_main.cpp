// Driver of tests/test_order_host.py: order_members of simplyp_amd/csrc/simplyp_order.h, called from plain host C++ (built with
// AddressSanitizer and UBSan by the test).
//   order_host_main E cost.bin out.bin
// cost.bin: the cost table [8][E], uint32 in host byte order.  out.bin: the permutation, E int32, then the 68 doubles of the
// rule's intermediate results (mean[8], inv[8], the 36 covariances, v2[8], v3[8]).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../simplyp_amd/csrc/simplyp_order.h"

int main(int argc, char** argv)
{
    if (argc != 4) { fprintf(stderr, "usage: %s E cost.bin out.bin\n", argv[0]); return 2; }
    const long long E = atoll(argv[1]);
    if (E < 1 || E > (1ll << 24)) { fprintf(stderr, "E out of range\n"); return 2; }
    constexpr int n_win = 8;
    std::vector<uint32_t> cost((size_t)n_win * (size_t)E);
    FILE* in = fopen(argv[2], "rb");
    if (!in) { perror(argv[2]); return 2; }
    const size_t got = fread(cost.data(), sizeof(uint32_t), cost.size(), in);
    const bool at_end = fgetc(in) == EOF;
    fclose(in);
    if (got != cost.size() || !at_end) { fprintf(stderr, "%s does not hold [8][%lld] uint32\n", argv[2], E); return 2; }
    std::vector<int32_t> perm;
    double diag[simplyp_order::DIAG_DOUBLES];
    simplyp_order::order_members(cost, n_win, (int)E, perm, diag);
    FILE* out = fopen(argv[3], "wb");
    if (!out) { perror(argv[3]); return 2; }
    const bool ok = fwrite(perm.data(), sizeof(int32_t), perm.size(), out) == perm.size() &&
                    fwrite(diag, sizeof(double), simplyp_order::DIAG_DOUBLES, out) == (size_t)simplyp_order::DIAG_DOUBLES;
    if (fclose(out) != 0 || !ok) { fprintf(stderr, "could not write %s\n", argv[3]); return 2; }
    return 0;
}
