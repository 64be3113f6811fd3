// Host side of the plastic flow: see plastic_plan.h.  Host only.
#include "plastic_plan.h"
#include <cmath>
#include <cstddef>
#include <limits>

namespace ipcgpu {

bool setPlasticRange(PlasticPlan& plan, int nT, int tetBegin, int tetEnd, double yield, double creep, double harden, std::string& err)
{
    auto fail = [&](const std::string& what) {
        err = "set_plasticity: " + what;
        return false;
    };
    if (nT <= 0) return fail("the mesh has no tetrahedron");
    if (!(0 <= tetBegin && tetBegin <= tetEnd && tetEnd <= nT)) return fail("range out of bounds");
    if (std::isnan(yield) || std::isnan(creep) || std::isnan(harden)) return fail("a parameter is NaN");
    if (yield < 0.0) return fail("the yield strain is negative");
    if (!(creep > 0.0)) return fail("the creep rate is not positive");
    if (harden < 0.0) return fail("the hardening modulus is negative");
    if (std::isinf(harden)) return fail("the hardening modulus is not finite");
    const double inf = std::numeric_limits<double>::infinity();
    if (plan.nT != nT) {
        plan.nT = nT;
        plan.yield.assign((std::size_t)nT, inf);
        plan.creep.assign((std::size_t)nT, inf);
        plan.harden.assign((std::size_t)nT, 0.0);
    }
    for (int t = tetBegin; t < tetEnd; ++t) {
        plan.yield[t] = yield;
        plan.creep[t] = creep;
        plan.harden[t] = harden;
    }
    plan.nOn = 0;
    for (int t = 0; t < nT; ++t) plan.nOn += plan.yield[t] < inf ? 1 : 0;
    return true;
}

} // namespace ipcgpu
