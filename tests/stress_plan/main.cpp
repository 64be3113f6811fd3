// Stand-alone driver of ipc_amd/csrc/stress_plan.cpp (the node -> element incidence list of the nodal stress pass) for tests/test_stress_plan_host.py.
// stdin: any number of cases `nV nT` followed by the 4 nT node indices of a column-major nT x 4 element table; stdout per case one line: `0` for a
// rejected table, else `1`, the nV + 1 row starts and the 4 nT element indices.
#include "stress_plan.h"
#include <cstdio>
#include <vector>

int main()
{
    int nV, nT;
    while (std::scanf("%d %d", &nV, &nT) == 2) {
        std::vector<int> F(nT > 0 ? 4 * (size_t)nT : 0);
        for (int& f : F)
            if (std::scanf("%d", &f) != 1) return 2;
        std::vector<int> ptr, elems;
        if (!ipcgpu::buildNodeElementIncidence(nV, nT, F.data(), ptr, elems)) {
            std::printf("0\n");
            continue;
        }
        std::printf("1");
        for (int p : ptr) std::printf(" %d", p);
        for (int e : elems) std::printf(" %d", e);
        std::printf("\n");
    }
    return 0;
}
