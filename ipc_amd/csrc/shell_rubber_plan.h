// Host side of the rubber membrane of the elastic shells (ipcgpu_shell_set_membrane; shell_rubber_kernels.hip): validates the per-triangle model and
// Mooney-Rivlin fraction and builds what the kernels read -- the compact list of the rubber triangles with their two constants.  Pure host arithmetic (no
// HIP header: tests/test_shell_rubber_plan_host.py builds it with g++).  The energy is stated in shell_rubber_kernels.h.
#pragma once
#include <string>
#include <vector>

namespace ipcgpu {

enum { SHELL_MEMBRANE_STVK = 0, SHELL_MEMBRANE_RUBBER = 1 };

struct ShellRubberPlan {
    int nTri = 0, nRubber = 0;
    std::vector<int> tri; // nRubber: ascending indices of the triangles with model 1
    std::vector<double> rubConst; // SoA [2][nRubber]: k1 = h A mu (1 - alpha) / 2, k2 = h A mu alpha / 2 with mu = E / 3, as K (1 - alpha) / 6 and K alpha / 6
    std::vector<int> model; // nTri: 0 StVK, 1 rubber (empty when nRubber == 0)
    std::vector<double> alpha; // nTri: alpha of a rubber triangle, 0 for a StVK one (empty when nRubber == 0)
};

// model: per triangle, 0 = St. Venant-Kirchhoff, 1 = rubber (null: every triangle StVK); alpha: per triangle, null = 0 everywhere (read only where model is 1);
// membraneK: h A E per triangle (ShellPlan::membraneK).  false, with the reason in err and the plan empty: a model other than 0 or 1; on a rubber triangle an
// alpha that is not finite or outside [0, 1), or a membraneK that is not positive and finite.  All models zero (or null): true with nRubber == 0.
bool buildShellRubberPlan(int nTri, const int* model, const double* alpha, const double* membraneK, ShellRubberPlan& plan, std::string& err);

// triConst (SoA [6][nTri], ShellPlan::triConst) with the two StVK constants (rows 4 and 5: h A mu, h A lambda_ps) of the plan's rubber triangles set to zero:
// what the StVK kernels read while the plan is set, so that they add exact zeros there
std::vector<double> shellTriConstWithoutRubber(const std::vector<double>& triConst, const ShellRubberPlan& plan);

} // namespace ipcgpu
