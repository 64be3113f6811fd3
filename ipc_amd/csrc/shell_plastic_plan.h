// Host side of the plastic flow of the elastic shells (ipcgpu_shell_set_plasticity; shell_plastic_kernels.hip): the four per-triangle parameters, kept
// current over calls that each set one contiguous range of triangles (later calls overwrite), and what follows from them per hinge -- whether it flows, its
// mean parameters and its rest constant g.  Pure host arithmetic (no HIP header: tests/test_shell_plastic_plan_host.py builds it with g++).  The model is
// stated in shell_plastic_kernels.h.
#pragma once
#include "shell_plan.h"
#include <string>
#include <vector>

namespace ipcgpu {

struct ShellPlasticPlan {
    int nTri = 0, nHinge = 0; // of the shell the arrays belong to; nTri == 0: ipcgpu_shell_set_plasticity was never called
    int nOn = 0; // triangles with a finite yield strain: 0 and the stepper launches no membrane flow
    int nHingeOn = 0; // hinges that flow: 0 and the stepper launches no hinge flow
    std::vector<double> yield; // nTri: membrane yield strain (deviatoric Hencky norm), +inf: the membrane is elastic
    std::vector<double> bendYield; // nTri: outer-fibre yield strain of the triangle's hinges, +inf: they do not flow
    std::vector<double> creep; // nTri: rate of the return per unit of time, +inf: rate-independent
    std::vector<double> harden; // nTri: isotropic hardening modulus K in y = yield + K alpha
    std::vector<int> hingeTri; // 2 nHinge: the triangle that holds (x0, x1, x2), then the one that holds (x0, x1, x3)
    // per hinge: the arithmetic means of the two triangles' bendYield, creep and harden -- hingeYield = +inf unless BOTH triangles have a finite bendYield --
    // and g = h_m w_e / (2 |eBar|) with h_m the mean rest thickness of the two triangles, w_e the ShellPlan's hingeWeight, |eBar| the rest length of the edge
    std::vector<double> hingeYield, hingeCreep, hingeHarden, hingeG;
};

// Triangles [triBegin, triEnd) of `shell` get (yield, bendYield, creep, harden); the hinge arrays are rebuilt.  Vrest: column-major nV x 3, the rest
// positions the shell was built from.  rubberModel (nullable, nTri): 1 where the triangle carries the rubber membrane.  A plan of another shell size (or
// an empty one) is first reset to "everything elastic": yield = bendYield = creep = +inf, harden = 0.
// false, with the reason in err and the plan as it was: no shell, a range outside 0 <= triBegin <= triEnd <= nTri, yield or bendYield negative (+inf switches
// that flow off), creep not positive (+inf is the rate-independent return), harden negative or infinite, anything NaN, or a rubber triangle in a range that
// switches a flow on.
bool setShellPlasticRange(ShellPlasticPlan& plan, const ShellPlan& shell, int nV, const double* Vrest, const int* rubberModel, int triBegin, int triEnd,
    double yield, double bendYield, double creep, double harden, std::string& err);

// true where the triangle has a finite yield or bendYield (false for an empty plan): what ipcgpu_shell_set_membrane refuses to turn into rubber
bool shellPlasticTriOn(const ShellPlasticPlan& plan, int t);

} // namespace ipcgpu
