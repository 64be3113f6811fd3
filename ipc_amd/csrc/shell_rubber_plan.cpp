// Host side of the shells' rubber membrane: see shell_rubber_plan.h.  Host only.
#include "shell_rubber_plan.h"
#include <cmath>
#include <cstddef>

namespace ipcgpu {

bool buildShellRubberPlan(int nTri, const int* model, const double* alpha, const double* membraneK, ShellRubberPlan& plan, std::string& err)
{
    plan = ShellRubberPlan();
    auto fail = [&](const std::string& what) {
        plan = ShellRubberPlan();
        err = what;
        return false;
    };
    if (nTri < 0) return fail("shell_set_membrane: bad sizes");
    plan.nTri = nTri;
    if (!model || nTri == 0) return true;
    if (!membraneK) return fail("shell_set_membrane: null argument");
    const std::size_t nt = (std::size_t)nTri;
    std::vector<double> k1, k2;
    for (std::size_t t = 0; t < nt; ++t) {
        const std::string name = "shell_set_membrane: triangle " + std::to_string(t);
        if (model[t] != SHELL_MEMBRANE_STVK && model[t] != SHELL_MEMBRANE_RUBBER) return fail(name + " has a model other than 0 (StVK) or 1 (rubber)");
        if (model[t] == SHELL_MEMBRANE_STVK) continue;
        const double a = alpha ? alpha[t] : 0.0;
        if (!std::isfinite(a)) return fail(name + " has an alpha that is not finite");
        if (a < 0.0 || a >= 1.0) return fail(name + " has an alpha outside [0, 1)");
        if (!(membraneK[t] > 0.0) || !std::isfinite(membraneK[t])) return fail(name + " has no membrane stiffness");
        plan.tri.push_back((int)t);
        k1.push_back(membraneK[t] * (1.0 - a) / 6.0);
        k2.push_back(membraneK[t] * a / 6.0);
    }
    plan.nRubber = (int)plan.tri.size();
    if (plan.nRubber == 0) return true;
    plan.rubConst.reserve(2 * k1.size());
    plan.rubConst.insert(plan.rubConst.end(), k1.begin(), k1.end());
    plan.rubConst.insert(plan.rubConst.end(), k2.begin(), k2.end());
    plan.model.assign(model, model + nt);
    plan.alpha.assign(nt, 0.0);
    for (int t : plan.tri) plan.alpha[(std::size_t)t] = alpha ? alpha[t] : 0.0;
    return true;
}

std::vector<double> shellTriConstWithoutRubber(const std::vector<double>& triConst, const ShellRubberPlan& plan)
{
    std::vector<double> c = triConst;
    const std::size_t nt = (std::size_t)plan.nTri;
    if (c.size() != 6 * nt) return c;
    for (int t : plan.tri) c[4 * nt + (std::size_t)t] = c[5 * nt + (std::size_t)t] = 0.0;
    return c;
}

} // namespace ipcgpu
