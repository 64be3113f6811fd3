// Stand-alone driver of ipc_amd/csrc/rod_plan.cpp for tests/test_rod_plan_host.py (plain g++, once more under the sanitizers).
// stdin, per mesh:  nV nSeg nTet nShellTri | 3 nV rest coordinates (node-major) | 2 nSeg node ids (segment-major) | nSeg x (r E rho) | 4 nTet node ids |
//                   3 nShellTri node ids
// stdout, per mesh: "0 <reason>" or
//   "1 nBend nPairs | 3 nBend triple nodes | nBend k_b | nBend rest |kb| | nSeg rest length | nSeg k_s | nV mass | nV isRodNode | 2 nPairs | lenSum"
#include "rod_plan.h"
#include <cstdio>
#include <iostream>

int main()
{
    int nV, nSeg, nTet, nTri;
    while (std::cin >> nV >> nSeg >> nTet >> nTri) {
        std::vector<double> V(3 * (size_t)nV), Vcm(3 * (size_t)nV), r(nSeg), E(nSeg), rho(nSeg);
        std::vector<int> seg(2 * (size_t)nSeg), scm(2 * (size_t)nSeg), tet(4 * (size_t)nTet), tri(3 * (size_t)nTri);
        for (auto& v : V) std::cin >> v;
        for (auto& v : seg) std::cin >> v;
        for (int s = 0; s < nSeg; ++s) std::cin >> r[s] >> E[s] >> rho[s];
        for (auto& v : tet) std::cin >> v;
        for (auto& v : tri) std::cin >> v;
        for (int v = 0; v < nV; ++v)
            for (int c = 0; c < 3; ++c) Vcm[v + (size_t)nV * c] = V[3 * (size_t)v + c];
        for (int s = 0; s < nSeg; ++s)
            for (int k = 0; k < 2; ++k) scm[s + (size_t)nSeg * k] = seg[2 * (size_t)s + k];
        ipcgpu::RodPlan p;
        std::string err;
        if (!ipcgpu::buildRodPlan(nV, nSeg, scm.data(), Vcm.data(), r.data(), E.data(), rho.data(), nTet, tet.data(), nTri, tri.data(), p, err)) {
            std::printf("0 %s\n", err.c_str());
            continue;
        }
        std::printf("1 %d %zu", p.nBend, p.pairs.size() / 2);
        for (int v : p.bend) std::printf(" %d", v);
        for (double v : p.bendK) std::printf(" %.17g", v);
        for (double v : p.restKb) std::printf(" %.17g", v);
        for (double v : p.segConst) std::printf(" %.17g", v);
        for (double v : p.mass) std::printf(" %.17g", v);
        for (char v : p.isRodNode) std::printf(" %d", (int)v);
        for (int v : p.pairs) std::printf(" %d", v);
        std::printf(" %.17g\n", p.lenSum);
    }
    return 0;
}
