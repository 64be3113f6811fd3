// Stand-alone driver of ipc_amd/csrc/plastic_plan.cpp for tests/test_plastic_plan_host.py (plain g++, once more under the sanitizers).
// stdin, per set:   nT nCalls | per call: tetBegin tetEnd yield creep harden  (numbers are read with strtod: "nan" and "inf" are numbers here)
//   the calls are applied in order to ONE plan, as ipcgpu_set_plasticity applies them to a context
// stdout, per set:  one token per call, "1" or "0<reason with blanks as tildes>", then "| nT nOn | nT yield | nT creep | nT harden" of the final plan
#include "plastic_plan.h"
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
    int nT, nCalls;
    while (std::cin >> nT >> nCalls) {
        ipcgpu::PlasticPlan plan;
        for (int i = 0; i < nCalls; ++i) {
            int b, e;
            std::cin >> b >> e;
            const double y = number(std::cin), c = number(std::cin), h = number(std::cin);
            std::string err;
            if (ipcgpu::setPlasticRange(plan, nT, b, e, y, c, h, err)) std::printf("1 ");
            else {
                std::replace(err.begin(), err.end(), ' ', '~');
                std::printf("0%s ", err.c_str());
            }
        }
        std::printf("| %d %d", plan.nT, plan.nOn);
        for (double v : plan.yield) std::printf(" %.17g", v);
        for (double v : plan.creep) std::printf(" %.17g", v);
        for (double v : plan.harden) std::printf(" %.17g", v);
        std::printf("\n");
    }
    return 0;
}
