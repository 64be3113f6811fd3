// Stand-alone driver of ipc_amd/csrc/shell_weave_plan.cpp (over shell_plan.cpp) for tests/test_shell_weave_plan_host.py (plain g++, once more under the sanitizers).
// stdin, per request:  nV nTri hasWoven hasNu hasWarp hasWeft bendScale | Vrest (column-major, 3 nV) | tri (column-major, 3 nTri) | thickness (nTri) |
//                      woven (nTri, if hasWoven) | dir (3 nTri) | E1 | E2 | G12 (nTri each) | nu12, bendWarp, bendWeft (nTri each, if has...)   (values may be nan / inf)
// stdout, per request: "0 <reason>" or "1 nWoven nHinge | nWoven triangle ids | 6 nWoven constants | woven (nTri) a (2 nTri) const4 (4 nTri) (none when
//                      nWoven == 0) | per hinge: x0 x1 factor (factor 1 when nWoven == 0) | same: 1 where row 1 of hingeConst with the plan equals the shell
//                      plan's bit for bit | rows 4 and 5 (2 nTri) of shellTriConstWithoutWeave applied to a triConst whose entry i is i + 1"
#include "shell_weave_plan.h"
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
    int nV, nTri, hasWoven, hasNu, hasWarp, hasWeft;
    double bendScale;
    while (std::cin >> nV >> nTri >> hasWoven >> hasNu >> hasWarp >> hasWeft >> bendScale) {
        const size_t nt = (size_t)nTri;
        std::vector<double> V(3 * (size_t)nV), triD(3 * nt), h(nt), wovenD(hasWoven ? nt : 0), dir(3 * nt), E1(nt), E2(nt), G12(nt), nu(hasNu ? nt : 0),
            bw(hasWarp ? nt : 0), bf(hasWeft ? nt : 0);
        if (!readValues(V) || !readValues(triD) || !readValues(h) || !readValues(wovenD) || !readValues(dir) || !readValues(E1) || !readValues(E2) || !readValues(G12)
            || !readValues(nu) || !readValues(bw) || !readValues(bf))
            return 2;
        std::vector<int> tri(triD.begin(), triD.end()), woven(wovenD.begin(), wovenD.end());
        std::vector<double> YM(nt, 1e5), PR(nt, 0.3), rho(nt, 1000.0);
        ipcgpu::ShellPlan shell;
        std::string err;
        if (!ipcgpu::buildShellPlan(nV, nTri, tri.data(), V.data(), h.data(), YM.data(), PR.data(), rho.data(), 0, nullptr, shell, err)) return 6;
        ipcgpu::ShellWeavePlan p;
        if (!ipcgpu::buildShellWeavePlan(shell, nV, V.data(), hasWoven ? woven.data() : nullptr, dir.data(), E1.data(), E2.data(), G12.data(), hasNu ? nu.data() : nullptr,
                hasWarp ? bw.data() : nullptr, hasWeft ? bf.data() : nullptr, p, err)) {
            std::printf("0 %s\n", err.c_str());
            if (p.nWoven || p.nTri || !p.tri.empty() || !p.wovConst.empty() || !p.woven.empty() || !p.a.empty() || !p.const4.empty() || !p.hingeFactor.empty())
                return 3; // a rejected request leaves the plan empty
            continue;
        }
        std::printf("1 %d %d", p.nWoven, shell.nHinge);
        for (int v : p.tri) std::printf(" %d", v);
        for (double v : p.wovConst) std::printf(" %.17g", v);
        for (int v : p.woven) std::printf(" %d", v);
        for (double v : p.a) std::printf(" %.17g", v);
        for (double v : p.const4) std::printf(" %.17g", v);
        if (p.nWoven ? p.hingeFactor.size() != (size_t)shell.nHinge : !p.hingeFactor.empty()) return 7;
        for (int i = 0; i < shell.nHinge; ++i)
            std::printf(" %d %d %.17g", shell.hinge[4 * (size_t)i], shell.hinge[4 * (size_t)i + 1], p.nWoven ? p.hingeFactor[(size_t)i] : 1.0);
        const std::vector<double> k = ipcgpu::shellHingeStiffnessWithWeave(shell, bendScale, p);
        if (k.size() != (size_t)shell.nHinge) return 8;
        bool same = true;
        for (int i = 0; i < shell.nHinge; ++i) {
            const double plain = bendScale * shell.hingeK[(size_t)i] * shell.hingeWeight[(size_t)i];
            same = same && k[(size_t)i] == plain;
            if (p.nWoven && k[(size_t)i] != plain * p.hingeFactor[(size_t)i]) return 9;
        }
        std::printf(" %d", same ? 1 : 0);
        std::vector<double> triConst(6 * nt);
        for (size_t i = 0; i < triConst.size(); ++i) triConst[i] = (double)(i + 1);
        const std::vector<double> z = ipcgpu::shellTriConstWithoutWeave(triConst, p);
        if (z.size() != triConst.size()) return 4;
        for (size_t i = 0; i < 4 * nt; ++i)
            if (z[i] != triConst[i]) return 5; // Dm^-1 is never touched
        for (size_t i = 4 * nt; i < z.size(); ++i) std::printf(" %.17g", z[i]);
        std::printf("\n");
    }
    return 0;
}
