// Host side of the shells' strain limit: see shell_limit_plan.h.  Host only.
#include "shell_limit_plan.h"
#include <cmath>
#include <cstddef>

namespace ipcgpu {

bool buildShellLimitPlan(int nTri, const double* limit, const double* onset, const double* stiff, const double* membraneK, ShellLimitPlan& plan, std::string& err)
{
    plan = ShellLimitPlan();
    auto fail = [&](const std::string& what) {
        plan = ShellLimitPlan();
        err = what;
        return false;
    };
    if (nTri < 0) return fail("shell_set_strain_limit: bad sizes");
    plan.nTri = nTri;
    if (!limit || nTri == 0) return true;
    if (!membraneK) return fail("shell_set_strain_limit: null argument");
    const std::size_t nt = (std::size_t)nTri;
    std::vector<double> on, lim, k;
    for (std::size_t t = 0; t < nt; ++t) {
        const double s = limit[t];
        const std::string name = "shell_set_strain_limit: triangle " + std::to_string(t);
        if (!std::isfinite(s)) return fail(name + " has a limit that is not finite");
        if (s < 0.0) return fail(name + " has a negative limit");
        if (s == 0.0) continue;
        const double o = onset ? onset[t] : 1.0, f = stiff ? stiff[t] : 1.0;
        if (!std::isfinite(o) || !std::isfinite(f)) return fail(name + " has an onset or a stiffness that is not finite");
        if (o < 1.0) return fail(name + " has an onset below 1");
        if (s <= o) return fail(name + " has a limit that is not above its onset");
        if (!(f > 0.0)) return fail(name + " needs stiff > 0");
        if (!(membraneK[t] > 0.0) || !std::isfinite(membraneK[t])) return fail(name + " has no membrane stiffness");
        plan.tri.push_back((int)t);
        on.push_back(o);
        lim.push_back(s);
        k.push_back(f * membraneK[t]);
    }
    plan.nLimited = (int)plan.tri.size();
    if (plan.nLimited == 0) return true;
    plan.limConst.reserve(3 * on.size());
    plan.limConst.insert(plan.limConst.end(), on.begin(), on.end());
    plan.limConst.insert(plan.limConst.end(), lim.begin(), lim.end());
    plan.limConst.insert(plan.limConst.end(), k.begin(), k.end());
    plan.triLimit.assign(limit, limit + nt);
    return true;
}

} // namespace ipcgpu
