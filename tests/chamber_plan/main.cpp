// Stand-alone driver of ipc_amd/csrc/chamber_plan.cpp for tests/test_chamber_plan_host.py (plain g++, once more under the sanitizers).
// stdin, per set:   nV nCh nTri | 3 nV rest coordinates (node-major) | nCh triEnd | nTri x 3 node ids (triangle-major) |
//                   nCh pressures  (numbers are read with strtod: "nan" and "inf" are numbers here)
// stdout, per set:  "0 <reason>" or
//   "1 nCh nTri nPairs | nCh triEnd | 3 nTri node ids (SoA) | nTri chamber ids | nCh pressures | nCh rest volumes | 3 nCh rest reference points | 2 nPairs"
#include "chamber_plan.h"
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
    int nV, nCh, nTri;
    while (std::cin >> nV >> nCh >> nTri) {
        std::vector<double> Vcm(3 * (size_t)nV), p((size_t)nCh);
        std::vector<int> triEnd((size_t)nCh);
        for (int v = 0; v < nV; ++v)
            for (int c = 0; c < 3; ++c) Vcm[v + (size_t)nV * c] = number(std::cin);
        for (int c = 0; c < nCh; ++c) std::cin >> triEnd[c];
        std::vector<int> tri(3 * (size_t)nTri); // column-major nTri x 3
        for (int t = 0; t < nTri; ++t)
            for (int k = 0; k < 3; ++k) std::cin >> tri[t + (size_t)nTri * k];
        for (int c = 0; c < nCh; ++c) p[c] = number(std::cin);
        // (the plan reads the list with the stride triEnd[nCh - 1], which a bad triEnd makes differ from nTri: hand it a list laid out with that stride)
        const int stride = nCh ? triEnd[nCh - 1] : 0;
        std::vector<int> triS(3 * (size_t)std::max(stride, 0));
        for (int t = 0; t < std::min(stride, nTri); ++t)
            for (int k = 0; k < 3; ++k) triS[t + (size_t)stride * k] = tri[t + (size_t)nTri * k];
        ipcgpu::ChamberPlan plan;
        std::string err;
        if (!ipcgpu::buildChamberPlan(nV, Vcm.data(), nCh, triEnd.data(), triS.data(), p.data(), plan, err)) {
            std::printf("0 %s\n", err.c_str());
            continue;
        }
        std::printf("1 %d %d %zu", plan.n, plan.nTri, plan.pairs.size() / 2);
        for (int v : plan.triEnd) std::printf(" %d", v);
        for (int v : plan.tri) std::printf(" %d", v);
        for (int v : plan.chamberOf) std::printf(" %d", v);
        for (double v : plan.pressure) std::printf(" %.17g", v);
        for (double v : plan.restVolume) std::printf(" %.17g", v);
        for (double v : plan.restRef) std::printf(" %.17g", v);
        for (int v : plan.pairs) std::printf(" %d", v);
        std::printf("\n");
    }
    return 0;
}
