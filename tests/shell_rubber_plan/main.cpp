// Stand-alone driver of ipc_amd/csrc/shell_rubber_plan.cpp for tests/test_shell_rubber_plan_host.py (plain g++, once more under the sanitizers).
// stdin, per request:  nTri hasModel hasAlpha | nTri membraneK | nTri model (if hasModel) | nTri alpha (if hasAlpha)      (real values may be nan / inf)
// stdout, per request: "0 <reason>" or "1 nRubber | nRubber triangle ids | 2 nRubber constants (k1, k2) | model (nTri) | alpha (nTri) (both none when
//                      nRubber == 0) | rows 4 and 5 (2 nTri) of shellTriConstWithoutRubber applied to a triConst whose entry i is i + 1"
#include "shell_rubber_plan.h"
#include <cstdio>
#include <cstdlib>
#include <iostream>

static bool readValues(std::vector<double>& a)
{
    std::string tok;
    for (auto& v : a) {
        if (!(std::cin >> tok)) return false;
        v = std::strtod(tok.c_str(), nullptr); // (operator>> does not read nan and inf)
    }
    return true;
}

int main()
{
    int nTri, hasModel, hasAlpha;
    while (std::cin >> nTri >> hasModel >> hasAlpha) {
        std::vector<double> K((size_t)nTri), modelD(hasModel ? (size_t)nTri : 0), alpha(hasAlpha ? (size_t)nTri : 0);
        if (!readValues(K) || !readValues(modelD) || !readValues(alpha)) return 2;
        std::vector<int> model(modelD.begin(), modelD.end());
        ipcgpu::ShellRubberPlan p;
        std::string err;
        if (!ipcgpu::buildShellRubberPlan(nTri, hasModel ? model.data() : nullptr, hasAlpha ? alpha.data() : nullptr, K.data(), p, err)) {
            std::printf("0 %s\n", err.c_str());
            if (p.nRubber || !p.tri.empty() || !p.rubConst.empty() || !p.model.empty() || !p.alpha.empty()) return 3; // a rejected request leaves the plan empty
            continue;
        }
        std::printf("1 %d", p.nRubber);
        for (int v : p.tri) std::printf(" %d", v);
        for (double v : p.rubConst) std::printf(" %.17g", v);
        for (int v : p.model) std::printf(" %d", v);
        for (double v : p.alpha) std::printf(" %.17g", v);
        std::vector<double> triConst(6 * (size_t)nTri);
        for (size_t i = 0; i < triConst.size(); ++i) triConst[i] = (double)(i + 1);
        const std::vector<double> z = ipcgpu::shellTriConstWithoutRubber(triConst, p);
        if (z.size() != triConst.size()) return 4;
        for (size_t i = 0; i < 4 * (size_t)nTri; ++i)
            if (z[i] != triConst[i]) return 5; // Dm^-1 is never touched
        for (size_t i = 4 * (size_t)nTri; i < z.size(); ++i) std::printf(" %.17g", z[i]);
        std::printf("\n");
    }
    return 0;
}
