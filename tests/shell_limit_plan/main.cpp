// Stand-alone driver of ipc_amd/csrc/shell_limit_plan.cpp for tests/test_shell_limit_plan_host.py (plain g++, once more under the sanitizers).
// stdin, per request:  nTri hasLimit hasOnset hasStiff | nTri membraneK | nTri limit (if hasLimit) | nTri onset (if hasOnset) | nTri stiff (if hasStiff)
//                      (values may be nan / inf)
// stdout, per request: "0 <reason>" or "1 nLimited | nLimited triangle ids | 3 nLimited constants (onset, limit, k) | triLimit (nTri, or none when nLimited == 0)"
#include "shell_limit_plan.h"
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
    int nTri, hasLimit, hasOnset, hasStiff;
    while (std::cin >> nTri >> hasLimit >> hasOnset >> hasStiff) {
        std::vector<double> K((size_t)nTri), limit(hasLimit ? (size_t)nTri : 0), onset(hasOnset ? (size_t)nTri : 0), stiff(hasStiff ? (size_t)nTri : 0);
        if (!readValues(K) || !readValues(limit) || !readValues(onset) || !readValues(stiff)) return 2;
        ipcgpu::ShellLimitPlan p;
        std::string err;
        if (!ipcgpu::buildShellLimitPlan(nTri, hasLimit ? limit.data() : nullptr, hasOnset ? onset.data() : nullptr, hasStiff ? stiff.data() : nullptr, K.data(), p, err)) {
            std::printf("0 %s\n", err.c_str());
            if (p.nLimited || !p.tri.empty() || !p.limConst.empty() || !p.triLimit.empty()) return 3; // a rejected request leaves the plan empty
            continue;
        }
        std::printf("1 %d", p.nLimited);
        for (int v : p.tri) std::printf(" %d", v);
        for (double v : p.limConst) std::printf(" %.17g", v);
        for (double v : p.triLimit) std::printf(" %.17g", v);
        std::printf("\n");
    }
    return 0;
}
