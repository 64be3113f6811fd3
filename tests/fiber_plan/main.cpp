// Stand-alone driver of ipc_amd/csrc/fiber_plan.cpp for tests/test_fiber_plan_host.py (plain g++, once more under the sanitizers).
// stdin:  nT | 9 nT doubles restTriInv (SoA [9][nT]) | nT doubles vol | nCalls | per call either
//           F tetBegin tetEnd dirPerElement k law k2 tensionOnly group nDir <3 nDir doubles>     (nDir == 0: a null direction)
//           A group act
//         numbers are read with strtod: "nan" and "inf" are numbers here.  The calls are applied in order to ONE plan, as the C API applies them to a context.
// stdout: one token per call, "1" or "0<reason with blanks as tildes>", then one line per array of the final plan after buildFiberLists:
//         nT nF / fibTet / b / volK / k2F / flagsF / groupOf / l0 / dir / k / k2 / flags / group / act
#include "fiber_plan.h"
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
template <class T>
static void line(const std::vector<T>& v)
{
    for (const T& x : v) std::printf("%.17g ", (double)x);
    std::printf("\n");
}

int main()
{
    int nT, nCalls;
    std::cin >> nT;
    std::vector<double> A(9 * (size_t)std::max(nT, 0)), vol((size_t)std::max(nT, 0));
    for (double& v : A) v = number(std::cin);
    for (double& v : vol) v = number(std::cin);
    std::cin >> nCalls;
    ipcgpu::FiberPlan plan;
    for (int i = 0; i < nCalls; ++i) {
        std::string kind, err;
        std::cin >> kind;
        bool ok;
        if (kind == "F") {
            int b, e, per, law, tens, group, nDir;
            std::cin >> b >> e >> per;
            const double k = number(std::cin);
            std::cin >> law;
            const double k2 = number(std::cin);
            std::cin >> tens >> group >> nDir;
            std::vector<double> dir(3 * (size_t)nDir);
            for (double& v : dir) v = number(std::cin);
            ok = ipcgpu::setFiberRange(plan, nT, b, e, nDir ? dir.data() : nullptr, per != 0, k, law, k2, tens != 0, group, err);
        }
        else {
            int group;
            std::cin >> group;
            ok = ipcgpu::setFiberActivation(plan, group, number(std::cin), err);
        }
        if (ok) std::printf("1 ");
        else {
            std::replace(err.begin(), err.end(), ' ', '~');
            std::printf("0%s ", err.c_str());
        }
    }
    std::printf("\n");
    if (plan.nT) ipcgpu::buildFiberLists(plan, A.data(), vol.data());
    std::printf("%d %d\n", plan.nT, plan.nF);
    line(plan.fibTet);
    line(plan.b);
    line(plan.volK);
    line(plan.k2F);
    line(plan.flagsF);
    line(plan.groupOf);
    line(plan.l0);
    line(plan.dir);
    line(plan.k);
    line(plan.k2);
    line(plan.flags);
    line(plan.group);
    line(plan.act);
    return 0;
}
