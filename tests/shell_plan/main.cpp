// Stand-alone driver of ipc_amd/csrc/shell_plan.cpp for tests/test_shell_plan_host.py (plain g++, once more under the sanitizers).
// stdin, per mesh:  nV nTri nTet | 3 nV rest coordinates (node-major) | 3 nTri node ids (triangle-major) | nTri x (h E nu rho) | 4 nTet node ids (tet-major)
// stdout, per mesh: "0 <reason>" or
//   "1 nHinge nPairs | 4 nHinge hinge nodes | nHinge restAngle | nHinge weight | nHinge k_b | nTri area | 6 nTri constants (triangle-major) | nV mass | 2 nPairs | edgeLenSum"
#include "shell_plan.h"
#include <cstdio>
#include <iostream>

int main()
{
    int nV, nTri, nTet;
    while (std::cin >> nV >> nTri >> nTet) {
        std::vector<double> V(3 * (size_t)nV), Vcm(3 * (size_t)nV), h(nTri), E(nTri), nu(nTri), rho(nTri);
        std::vector<int> tri(3 * (size_t)nTri), tcm(3 * (size_t)nTri), tet(4 * (size_t)nTet), tetcm(4 * (size_t)nTet);
        for (auto& v : V) std::cin >> v;
        for (auto& v : tri) std::cin >> v;
        for (int t = 0; t < nTri; ++t) std::cin >> h[t] >> E[t] >> nu[t] >> rho[t];
        for (auto& v : tet) std::cin >> v;
        for (int v = 0; v < nV; ++v)
            for (int c = 0; c < 3; ++c) Vcm[v + (size_t)nV * c] = V[3 * (size_t)v + c];
        for (int t = 0; t < nTri; ++t)
            for (int k = 0; k < 3; ++k) tcm[t + (size_t)nTri * k] = tri[3 * (size_t)t + k];
        for (int t = 0; t < nTet; ++t)
            for (int k = 0; k < 4; ++k) tetcm[t + (size_t)nTet * k] = tet[4 * (size_t)t + k];
        ipcgpu::ShellPlan p;
        std::string err;
        if (!ipcgpu::buildShellPlan(nV, nTri, tcm.data(), Vcm.data(), h.data(), E.data(), nu.data(), rho.data(), nTet, tetcm.data(), p, err)) {
            std::printf("0 %s\n", err.c_str());
            continue;
        }
        std::printf("1 %d %zu", p.nHinge, p.pairs.size() / 2);
        for (int v : p.hinge) std::printf(" %d", v);
        for (double v : p.restAngle) std::printf(" %.17g", v);
        for (double v : p.hingeWeight) std::printf(" %.17g", v);
        for (double v : p.hingeK) std::printf(" %.17g", v);
        for (double v : p.area) std::printf(" %.17g", v);
        for (int t = 0; t < nTri; ++t)
            for (int k = 0; k < 6; ++k) std::printf(" %.17g", p.triConst[(size_t)k * nTri + t]);
        for (double v : p.mass) std::printf(" %.17g", v);
        for (int v : p.pairs) std::printf(" %d", v);
        std::printf(" %.17g\n", p.edgeLenSum);
    }
    return 0;
}
