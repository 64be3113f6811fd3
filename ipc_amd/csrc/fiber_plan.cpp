// Host side of the fibre reinforcement: see fiber_plan.h.  Host only.
#include "fiber_plan.h"
#include <cmath>
#include <cstddef>

namespace ipcgpu {

namespace {
void resetPlan(FiberPlan& plan, int nT)
{
    plan = FiberPlan();
    plan.nT = nT;
    plan.dir.assign(3 * (std::size_t)nT, 0.0);
    plan.k.assign((std::size_t)nT, 0.0);
    plan.k2.assign((std::size_t)nT, 0.0);
    plan.flags.assign((std::size_t)nT, 0);
    plan.group.assign((std::size_t)nT, 0);
    plan.act.assign(FIBER_MAX_GROUPS, 0.0);
    plan.l0.assign(FIBER_MAX_GROUPS, 1.0);
}
} // namespace

bool setFiberRange(FiberPlan& plan, int nT, int tetBegin, int tetEnd, const double* dir, bool dirPerElement, double k, int law, double k2, bool tensionOnly,
    int group, std::string& err)
{
    auto fail = [&](const std::string& what) {
        err = "set_fibers: " + what;
        return false;
    };
    if (nT <= 0) return fail("the mesh has no tetrahedron");
    if (!(0 <= tetBegin && tetBegin <= tetEnd && tetEnd <= nT)) return fail("range out of bounds");
    if (!(k >= 0.0) || std::isinf(k)) return fail("the stiffness is negative or not finite");
    const std::size_t n = (std::size_t)nT, m = (std::size_t)(tetEnd - tetBegin);
    std::vector<double> unit;
    if (k > 0.0) {
        if (law != FIBER_LAW_SPRING && law != FIBER_LAW_EXP) return fail("unknown law (0: spring, 1: exp)");
        if (law == FIBER_LAW_EXP && (!(k2 > 0.0) || std::isinf(k2))) return fail("the exp law needs a finite k2 > 0");
        if (!(0 <= group && group < FIBER_MAX_GROUPS)) return fail("the activation group is outside [0, 64)");
        if (law == FIBER_LAW_EXP && plan.nT == nT && plan.act[group] != 0.0) return fail("activation is not defined for the exp law: the group's activation is not 0");
        if (!dir) return fail("null direction");
        unit.resize(3 * m);
        for (std::size_t e = 0; e < m; ++e) {
            const double* a = dir + (dirPerElement ? 3 * e : 0);
            if (!(std::isfinite(a[0]) && std::isfinite(a[1]) && std::isfinite(a[2]))) return fail("a direction is not finite");
            const double s = std::fmax(std::fabs(a[0]), std::fmax(std::fabs(a[1]), std::fabs(a[2])));
            if (!(s > 0.0)) return fail("a direction is zero");
            const double x = a[0] / s, y = a[1] / s, z = a[2] / s, len = std::sqrt(x * x + y * y + z * z); // (scaled first: no overflow, no underflow)
            unit[3 * e] = x / len;
            unit[3 * e + 1] = y / len;
            unit[3 * e + 2] = z / len;
        }
    }
    if (plan.nT != nT) resetPlan(plan, nT);
    for (std::size_t e = 0; e < m; ++e) {
        const std::size_t t = (std::size_t)tetBegin + e;
        const bool on = k > 0.0;
        for (int r = 0; r < 3; ++r) plan.dir[r * n + t] = on ? unit[3 * e + r] : 0.0;
        plan.k[t] = k;
        plan.k2[t] = on && law == FIBER_LAW_EXP ? k2 : 0.0;
        plan.flags[t] = !on ? 0 : law == FIBER_LAW_EXP ? FIBER_FLAG_EXP : tensionOnly ? FIBER_FLAG_TENSION_ONLY : 0;
        plan.group[t] = on ? group : 0;
    }
    return true;
}

bool setFiberActivation(FiberPlan& plan, int group, double act, std::string& err)
{
    auto fail = [&](const std::string& what) {
        err = "fiber_set_activation: " + what;
        return false;
    };
    if (plan.nT <= 0) return fail("no fibres are set");
    if (!(0 <= group && group < FIBER_MAX_GROUPS)) return fail("the activation group is outside [0, 64)");
    if (!std::isfinite(act) || !(act < 1.0)) return fail("the activation must be finite and below 1 (the active rest stretch 1 - act stays positive)");
    if (act != 0.0)
        for (int t = 0; t < plan.nT; ++t)
            if (plan.k[t] > 0.0 && plan.group[t] == group && (plan.flags[t] & FIBER_FLAG_EXP)) return fail("activation is not defined for the exp law: the group holds an exp element");
    plan.act[group] = act;
    plan.l0[group] = 1.0 - act;
    return true;
}

void buildFiberLists(FiberPlan& plan, const double* A, const double* vol)
{
    const std::size_t n = (std::size_t)plan.nT;
    plan.fibTet.clear();
    for (int t = 0; t < plan.nT; ++t)
        if (plan.k[t] > 0.0 && vol[t] * plan.k[t] > 0.0) plan.fibTet.push_back(t);
    const std::size_t nF = plan.fibTet.size();
    plan.nF = (int)nF;
    plan.b.assign(3 * nF, 0.0);
    plan.volK.assign(nF, 0.0);
    plan.k2F.assign(nF, 0.0);
    plan.flagsF.assign(nF, 0);
    plan.groupOf.assign(nF, 0);
    for (std::size_t i = 0; i < nF; ++i) {
        const std::size_t t = (std::size_t)plan.fibTet[i];
        for (int r = 0; r < 3; ++r) {
            double s = 0.0;
            for (int c = 0; c < 3; ++c) s += A[(std::size_t)(r + 3 * c) * n + t] * plan.dir[c * n + t];
            plan.b[r * nF + i] = s;
        }
        plan.volK[i] = vol[t] * plan.k[t];
        plan.k2F[i] = plan.k2[t];
        plan.flagsF[i] = plan.flags[t];
        plan.groupOf[i] = plan.group[t];
    }
}

} // namespace ipcgpu
