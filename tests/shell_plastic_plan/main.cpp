// Stand-alone driver of ipc_amd/csrc/shell_plastic_plan.cpp (with shell_plan.cpp for the shell it belongs to) for tests/test_shell_plastic_plan_host.py
// (plain g++, once more under the sanitizers).
// stdin, per set:   nV nTri | nV x 3 rest positions (row by row) | nTri x 3 node ids | nTri thicknesses | nTri rubber flags | nCalls |
//                   per call: triBegin triEnd yield bendYield creep harden  (numbers are read with strtod: "nan" and "inf" are numbers here)
//   the calls are applied in order to ONE plan, as ipcgpu_shell_set_plasticity applies them to a context
// stdout, per set:  one token per call, "1" or "0<reason with blanks as tildes>", then "| nTri nHinge nOn nHingeOn | yield | bendYield | creep | harden |
//                   hingeTri (2 nHinge) | hingeYield | hingeCreep | hingeHarden | hingeG" of the final plan
#include "shell_plastic_plan.h"
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
    int nV, nTri;
    while (std::cin >> nV >> nTri) {
        std::vector<double> V(3 * (size_t)nV), h((size_t)nTri), one((size_t)nTri, 1.0), nu((size_t)nTri, 0.3);
        std::vector<int> tri(3 * (size_t)nTri), rubber((size_t)nTri);
        for (int v = 0; v < nV; ++v)
            for (int k = 0; k < 3; ++k) V[v + (size_t)nV * k] = number(std::cin); // column-major
        for (int t = 0; t < nTri; ++t)
            for (int k = 0; k < 3; ++k) std::cin >> tri[t + (size_t)nTri * k];
        for (double& x : h) x = number(std::cin);
        bool anyRubber = false;
        for (int& r : rubber) {
            std::cin >> r;
            anyRubber = anyRubber || r;
        }
        ipcgpu::ShellPlan shell;
        std::string err;
        if (nTri > 0 && !ipcgpu::buildShellPlan(nV, nTri, tri.data(), V.data(), h.data(), one.data(), nu.data(), one.data(), 0, nullptr, shell, err)) {
            std::fprintf(stderr, "shell plan: %s\n", err.c_str());
            return 2;
        }
        int nCalls;
        std::cin >> nCalls;
        ipcgpu::ShellPlasticPlan plan;
        for (int i = 0; i < nCalls; ++i) {
            int b, e;
            std::cin >> b >> e;
            const double y = number(std::cin), yb = number(std::cin), c = number(std::cin), K = number(std::cin);
            if (ipcgpu::setShellPlasticRange(plan, shell, nV, V.data(), anyRubber ? rubber.data() : nullptr, b, e, y, yb, c, K, err)) std::printf("1 ");
            else {
                std::replace(err.begin(), err.end(), ' ', '~');
                std::printf("0%s ", err.c_str());
            }
        }
        std::printf("| %d %d %d %d", plan.nTri, plan.nHinge, plan.nOn, plan.nHingeOn);
        for (const std::vector<double>* a : { &plan.yield, &plan.bendYield, &plan.creep, &plan.harden }) {
            std::printf(" |");
            for (double v : *a) std::printf(" %.17g", v);
        }
        std::printf(" |");
        for (int v : plan.hingeTri) std::printf(" %d", v);
        for (const std::vector<double>* a : { &plan.hingeYield, &plan.hingeCreep, &plan.hingeHarden, &plan.hingeG }) {
            std::printf(" |");
            for (double v : *a) std::printf(" %.17g", v);
        }
        std::printf("\n");
    }
    return 0;
}
