// Host side of the plastic flow of tetrahedral bodies (ipcgpu_set_plasticity; plastic_kernels.hip): the three per-element parameters the kernel reads,
// SoA, kept current over calls that each set one contiguous range of elements (as ipcgpu_set_component_material; later calls overwrite).  Pure host
// arithmetic (no HIP header: tests/test_plastic_plan_host.py builds it with g++).  The reference has no plasticity; the model is stated in plastic_kernels.h.
#pragma once
#include <string>
#include <vector>

namespace ipcgpu {

struct PlasticPlan {
    int nT = 0; // elements of the mesh the arrays belong to; 0: ipcgpu_set_plasticity was never called
    int nOn = 0; // elements with a finite yield strain: 0 and the stepper launches nothing
    std::vector<double> yield; // nT: yield strain (deviatoric Hencky norm), +inf: the element is elastic
    std::vector<double> creep; // nT: rate of the return per unit of time, +inf: rate-independent
    std::vector<double> harden; // nT: isotropic hardening modulus K in y = yield + K alpha
};

// Elements [tetBegin, tetEnd) of a mesh of nT elements get (yield, creep, harden).  A plan of another nT (or an empty one) is first reset to "every
// element elastic": yield = +inf, creep = +inf, harden = 0.
// false, with the reason in err and the plan as it was: nT <= 0, a range outside 0 <= tetBegin <= tetEnd <= nT, yield negative (+inf switches the range
// off), creep not positive (+inf is the rate-independent return), harden negative or infinite, anything NaN.
bool setPlasticRange(PlasticPlan& plan, int nT, int tetBegin, int tetEnd, double yield, double creep, double harden, std::string& err);

} // namespace ipcgpu
