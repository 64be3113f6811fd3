// Stand-alone driver of ipc_amd/csrc/attach_plan.cpp for tests/test_attach_plan_host.py (plain g++, once more under the sanitizers).
// stdin, per set:   nV n | 3 nV rest coordinates (node-major) | n x (3 node ids of A, 3 weights of A, 3 node ids of B, 3 weights of B, k, L)
//                   (numbers are read with strtod: "nan" and "inf" are numbers here)
// stdout, per set:  "0 <reason>" or
//   "1 n nPairs | n counts | 6 n node ids (slot-major) | 6 n coefficients (slot-major) | n k | n L | n rest distances | 2 nPairs"
#include "attach_plan.h"
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
    int nV, n;
    while (std::cin >> nV >> n) {
        std::vector<double> Vcm(3 * (size_t)nV), wA(3 * (size_t)n), wB(3 * (size_t)n), k(n), L(n);
        std::vector<int> nA(3 * (size_t)n), nB(3 * (size_t)n);
        for (int v = 0; v < nV; ++v)
            for (int c = 0; c < 3; ++c) Vcm[v + (size_t)nV * c] = number(std::cin);
        for (int i = 0; i < n; ++i) {
            for (int s = 0; s < 3; ++s) std::cin >> nA[3 * (size_t)i + s];
            for (int s = 0; s < 3; ++s) wA[3 * (size_t)i + s] = number(std::cin);
            for (int s = 0; s < 3; ++s) std::cin >> nB[3 * (size_t)i + s];
            for (int s = 0; s < 3; ++s) wB[3 * (size_t)i + s] = number(std::cin);
            k[i] = number(std::cin);
            L[i] = number(std::cin);
        }
        ipcgpu::AttachPlan p;
        std::string err;
        if (!ipcgpu::buildAttachPlan(nV, n, nA.data(), wA.data(), nB.data(), wB.data(), k.data(), L.data(), p, err)) {
            std::printf("0 %s\n", err.c_str());
            continue;
        }
        std::printf("1 %d %zu", p.n, p.pairs.size() / 2);
        for (int v : p.count) std::printf(" %d", v);
        for (int v : p.node) std::printf(" %d", v);
        for (double v : p.coef) std::printf(" %.17g", v);
        for (double v : p.kL) std::printf(" %.17g", v);
        for (int i = 0; i < p.n; ++i) std::printf(" %.17g", ipcgpu::attachRestDistance(p, i, nV, Vcm.data()));
        for (int v : p.pairs) std::printf(" %d", v);
        std::printf("\n");
    }
    return 0;
}
