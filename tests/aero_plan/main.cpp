// Stand-alone driver of ipc_amd/csrc/aero_plan.cpp for tests/test_aero_plan_host.py (plain g++, once more under the sanitizers).
// stdin, per set:   nV nSurf nTri | 3 nV rest coordinates (node-major) | nSurf triEnd | nTri x 3 node ids (triangle-major) |
//                   nSurf cn | nSurf ct | nSurf oneSided  (numbers are read with strtod: "nan" and "inf" are numbers here)
// stdout, per set:  "0 <reason>" or
//   "1 nSurf nTri nPairs | nSurf triEnd | 3 nTri node ids (SoA) | nTri surface ids | 4 nSurf coef | 8 nTri rest records | 2 nPairs"
#include "aero_plan.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>

static double number(std::istream& in)
{
    std::string tok;
    in >> tok;
    return std::strtod(tok.c_str(), nullptr);
}

int main()
{
    int nV, nSurf, nTri;
    while (std::cin >> nV >> nSurf >> nTri) {
        std::vector<double> Vcm(3 * (size_t)nV), cn((size_t)nSurf), ct((size_t)nSurf);
        std::vector<int> triEnd((size_t)nSurf), one((size_t)nSurf);
        for (int v = 0; v < nV; ++v)
            for (int c = 0; c < 3; ++c) Vcm[v + (size_t)nV * c] = number(std::cin);
        for (int s = 0; s < nSurf; ++s) std::cin >> triEnd[s];
        std::vector<int> tri(3 * (size_t)nTri); // column-major nTri x 3
        for (int t = 0; t < nTri; ++t)
            for (int k = 0; k < 3; ++k) std::cin >> tri[t + (size_t)nTri * k];
        for (int s = 0; s < nSurf; ++s) cn[s] = number(std::cin);
        for (int s = 0; s < nSurf; ++s) ct[s] = number(std::cin);
        for (int s = 0; s < nSurf; ++s) std::cin >> one[s];
        // (the plan reads the list with the stride triEnd[nSurf - 1], which a bad triEnd makes differ from nTri: hand it a list laid out with that stride)
        const int stride = nSurf ? triEnd[nSurf - 1] : 0;
        std::vector<int> triS(3 * (size_t)std::max(stride, 0));
        for (int t = 0; t < std::min(stride, nTri); ++t)
            for (int k = 0; k < 3; ++k) triS[t + (size_t)stride * k] = tri[t + (size_t)nTri * k];
        ipcgpu::AeroPlan plan;
        std::string err;
        if (!ipcgpu::buildAeroPlan(nV, Vcm.data(), nSurf, triEnd.data(), triS.data(), cn.data(), ct.data(), one.data(), plan, err)) {
            std::printf("0 %s\n", err.c_str());
            continue;
        }
        std::printf("1 %d %d %zu", plan.n, plan.nTri, plan.pairs.size() / 2);
        for (int v : plan.triEnd) std::printf(" %d", v);
        for (int v : plan.tri) std::printf(" %d", v);
        for (int v : plan.surfOf) std::printf(" %d", v);
        for (double v : plan.coef) std::printf(" %.17g", v);
        for (double v : plan.restRecord) std::printf(" %.17g", v);
        for (int v : plan.pairs) std::printf(" %d", v);
        std::printf("\n");
    }
    return 0;
}
