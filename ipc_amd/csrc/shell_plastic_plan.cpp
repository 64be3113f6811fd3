// Host side of the shells' plastic flow: see shell_plastic_plan.h.  Host only.
#include "shell_plastic_plan.h"
#include <array>
#include <cmath>
#include <cstddef>
#include <limits>
#include <map>
#include <utility>

namespace ipcgpu {

namespace {

// per hinge the two triangles: the one that traverses x0 -> x1 (it holds x2), then the one that traverses x1 -> x0 (it holds x3)
bool hingeTriangles(const ShellPlan& shell, std::vector<int>& hingeTri)
{
    std::map<std::pair<int, int>, std::array<int, 2>> byEdge;
    for (int t = 0; t < shell.nTri; ++t)
        for (int k = 0; k < 3; ++k) {
            const int a = shell.tri[3 * (std::size_t)t + k], b = shell.tri[3 * (std::size_t)t + (k + 1) % 3];
            auto it = byEdge.emplace(std::make_pair(a < b ? a : b, a < b ? b : a), std::array<int, 2>{ -1, -1 }).first;
            it->second[a < b ? 0 : 1] = t;
        }
    hingeTri.assign(2 * (std::size_t)shell.nHinge, -1);
    for (int i = 0; i < shell.nHinge; ++i) {
        const auto it = byEdge.find(std::make_pair(shell.hinge[4 * (std::size_t)i], shell.hinge[4 * (std::size_t)i + 1]));
        if (it == byEdge.end() || it->second[0] < 0 || it->second[1] < 0) return false;
        hingeTri[2 * (std::size_t)i] = it->second[0];
        hingeTri[2 * (std::size_t)i + 1] = it->second[1];
    }
    return true;
}

} // namespace

bool setShellPlasticRange(ShellPlasticPlan& plan, const ShellPlan& shell, int nV, const double* Vrest, const int* rubberModel, int triBegin, int triEnd,
    double yield, double bendYield, double creep, double harden, std::string& err)
{
    auto fail = [&](const std::string& what) {
        err = "shell_set_plasticity: " + what;
        return false;
    };
    const int nTri = shell.nTri, nHinge = shell.nHinge;
    if (nTri <= 0) return fail("no shell is set");
    if (!(0 <= triBegin && triBegin <= triEnd && triEnd <= nTri)) return fail("range out of bounds");
    if (std::isnan(yield) || std::isnan(bendYield) || std::isnan(creep) || std::isnan(harden)) return fail("a parameter is NaN");
    if (yield < 0.0) return fail("the yield strain is negative");
    if (bendYield < 0.0) return fail("the bending yield strain is negative");
    if (!(creep > 0.0)) return fail("the creep rate is not positive");
    if (harden < 0.0) return fail("the hardening modulus is negative");
    if (std::isinf(harden)) return fail("the hardening modulus is not finite");
    const double inf = std::numeric_limits<double>::infinity();
    if (rubberModel && (yield < inf || bendYield < inf))
        for (int t = triBegin; t < triEnd; ++t)
            if (rubberModel[t]) return fail("triangle " + std::to_string(t) + " carries the rubber membrane");
    std::vector<int> hingeTri = plan.hingeTri;
    const bool fresh = plan.nTri != nTri || plan.nHinge != nHinge;
    if (fresh && !hingeTriangles(shell, hingeTri)) return fail("a hinge of the shell has no two triangles");
    if (fresh && nHinge > 0 && (!Vrest || nV <= 0)) return fail("no rest positions");
    // nothing can fail from here on
    if (fresh) {
        plan = ShellPlasticPlan();
        plan.nTri = nTri;
        plan.nHinge = nHinge;
        plan.yield.assign((std::size_t)nTri, inf);
        plan.bendYield.assign((std::size_t)nTri, inf);
        plan.creep.assign((std::size_t)nTri, inf);
        plan.harden.assign((std::size_t)nTri, 0.0);
        plan.hingeTri = std::move(hingeTri);
        plan.hingeG.resize((std::size_t)nHinge);
        for (int i = 0; i < nHinge; ++i) {
            const int x0 = shell.hinge[4 * (std::size_t)i], x1 = shell.hinge[4 * (std::size_t)i + 1];
            double l2 = 0.0;
            for (int k = 0; k < 3; ++k) {
                const double d = Vrest[x1 + (std::size_t)nV * k] - Vrest[x0 + (std::size_t)nV * k];
                l2 += d * d;
            }
            const double hm = 0.5 * (shell.thickness[plan.hingeTri[2 * (std::size_t)i]] + shell.thickness[plan.hingeTri[2 * (std::size_t)i + 1]]);
            plan.hingeG[i] = hm * shell.hingeWeight[i] / (2.0 * std::sqrt(l2));
        }
    }
    for (int t = triBegin; t < triEnd; ++t) {
        plan.yield[t] = yield;
        plan.bendYield[t] = bendYield;
        plan.creep[t] = creep;
        plan.harden[t] = harden;
    }
    plan.nOn = 0;
    for (int t = 0; t < nTri; ++t) plan.nOn += plan.yield[t] < inf ? 1 : 0;
    plan.hingeYield.assign((std::size_t)nHinge, inf);
    plan.hingeCreep.assign((std::size_t)nHinge, inf);
    plan.hingeHarden.assign((std::size_t)nHinge, 0.0);
    plan.nHingeOn = 0;
    for (int i = 0; i < nHinge; ++i) {
        const int a = plan.hingeTri[2 * (std::size_t)i], b = plan.hingeTri[2 * (std::size_t)i + 1];
        if (!(plan.bendYield[a] < inf && plan.bendYield[b] < inf)) continue;
        plan.hingeYield[i] = 0.5 * (plan.bendYield[a] + plan.bendYield[b]);
        plan.hingeCreep[i] = 0.5 * (plan.creep[a] + plan.creep[b]);
        plan.hingeHarden[i] = 0.5 * (plan.harden[a] + plan.harden[b]);
        ++plan.nHingeOn;
    }
    return true;
}

bool shellPlasticTriOn(const ShellPlasticPlan& plan, int t)
{
    if (t < 0 || t >= plan.nTri) return false;
    const double inf = std::numeric_limits<double>::infinity();
    return plan.yield[t] < inf || plan.bendYield[t] < inf;
}

} // namespace ipcgpu
