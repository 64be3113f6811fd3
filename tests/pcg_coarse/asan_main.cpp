// TEST INFRASTRUCTURE (host only): a stand-alone program around ipc_amd/csrc/pcg_coarse.cpp for a sanitizer build (tests/test_pcg_coarse.py compiles it
// with -fsanitize=address,undefined and runs it).  Reads "nNodes nnz", then ja, rowBase, rowLen and the fixed mask as text; walks everything the unit emits
// the way the device code does and checks that every index stays inside the array it addresses.
#include "../../ipc_amd/csrc/pcg_coarse.h"
#include <cstdio>
#include <fstream>
#include <vector>
using namespace ipcgpu;

#define REQUIRE(c)                                              \
    do {                                                        \
        if (!(c)) {                                             \
            std::printf("failed: %s (line %d)\n", #c, __LINE__); \
            return 1;                                           \
        }                                                       \
    } while (0)

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    int n = 0, nnz = 0;
    in >> n >> nnz;
    std::vector<int> ja(nnz), rowBase(n), rowLen(n);
    std::vector<unsigned char> fixed(n);
    for (int& x : ja) in >> x;
    for (int& x : rowBase) in >> x;
    for (int& x : rowLen) in >> x;
    for (auto& x : fixed) {
        int v;
        in >> v;
        x = (unsigned char)v;
    }
    REQUIRE(in.good());
    long long sum = 0;
    for (int rep = 0; rep < 2; ++rep) { // (the second build reuses the vectors of the first)
        static PcgCoarse c;
        c.build(n, ja.data(), rowBase.data(), rowLen.data(), fixed.data());
        const int nPairs = (int)c.pairI.size(), cnnz = (int)c.cja.size();
        REQUIRE((int)c.aggOf.size() == n && (int)c.aggPtr.size() == c.nAgg + 1 && (int)c.cia.size() == 6 * c.nAgg + 1 && c.cia.back() == cnnz);
        REQUIRE((int)c.pairPtr.size() == nPairs + 1 && (int)c.pairSlot.size() == 4 * nPairs);
        for (int p = 0; p < nPairs; ++p) {
            for (int q = 0; q < 4; ++q) {
                const int s = c.pairSlot[4 * p + q];
                if (s < 0) continue;
                const int cn = 2 * c.pairI[p] + q / 2, len = c.cRowLen[cn];
                const bool diag = c.pairI[p] == c.pairJ[p] && (q == 0 || q == 3);
                const int last = diag ? s + 2 * len - 1 : s + 2 * len - 3 + 2;
                REQUIRE(s >= 0 && last < cnnz);
                sum += c.cja[s] + c.cja[last];
            }
            for (int e = c.pairPtr[p]; e < c.pairPtr[p + 1]; ++e) {
                const int u = c.entRow[e], w = c.entCol[e], s = c.entSlot[e], len = rowLen[u];
                REQUIRE(u >= 0 && u < n && w >= u && w < n);
                const int last = u == w ? s + 2 * len - 1 : s + 2 * len - 3 + 2;
                REQUIRE(s >= 0 && last < nnz);
                sum += ja[s] + ja[last] + c.entTrans[e];
            }
        }
        for (int I = 0; I < c.nAgg; ++I)
            for (int k = c.aggPtr[I]; k < c.aggPtr[I + 1]; ++k) REQUIRE(c.aggOf[c.aggNodes[k]] == I);
    }
    std::printf("ok %lld\n", sum);
    return 0;
}
