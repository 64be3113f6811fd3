// Host side of the woven cloth of the elastic shells (ipcgpu_shell_set_weave; shell_weave_kernels.hip): validates the per-triangle selector, warp direction,
// moduli and bend factors and builds what the kernels read -- the compact list of the woven triangles with their in-plane warp direction and four constants --
// and the factor every hinge's bending stiffness is multiplied by.  Pure host arithmetic (no HIP header: tests/test_shell_weave_plan_host.py builds it with
// g++).  The energy is stated in shell_weave_kernels.h.
#pragma once
#include "shell_plan.h"
#include <string>
#include <vector>

namespace ipcgpu {

struct ShellWeavePlan {
    int nTri = 0, nWoven = 0;
    std::vector<int> tri; // nWoven: ascending indices of the triangles with selector 1
    // SoA [6][nWoven]: a_x, a_y (the unit warp direction in the triangle's rest frame of shell_plan.h: first axis along X1 - X0), then h A C11, h A C12,
    // h A C22, h A G12 with C11 = E1 / (1 - nu12 nu21), C22 = E2 / (1 - nu12 nu21), C12 = nu12 E2 / (1 - nu12 nu21), nu21 = nu12 E2 / E1
    std::vector<double> wovConst;
    // what ipcgpu_shell_weave_get returns; all empty when nWoven == 0
    std::vector<int> woven; // nTri: 0 or 1
    std::vector<double> a; // 2 per triangle (a_x, a_y), 0 0 on a triangle that is not woven
    std::vector<double> const4; // 4 per triangle (C11, C12, C22, G12, without h A), zeros on a triangle that is not woven
    // nHinge: the mean over the hinge's two triangles of bendWarp sin^2 phi + bendWeft cos^2 phi, phi the angle between the rest edge and the triangle's warp;
    // a triangle that is not woven counts 1.  Formed as bendWeft + (bendWarp - bendWeft) sin^2 phi, so that equal factors give exactly that factor
    std::vector<double> hingeFactor;
};

// woven: per triangle 0 or 1 (null: none); dir: 3 per triangle (x, y, z of triangle t at 3 t ..), a vector of rest space, projected into the triangle's rest
// plane and normalised; E1 (warp), E2 (weft), G12 (shear): per triangle; nu12 (null: 0), bendWarp, bendWeft (null: 1): per triangle.  All of them are read
// where the selector is 1 only.  Vrest: column-major nV x 3 (the positions the shell plan was built from).
// false, with the reason in err -- it names the triangle -- and the plan empty: a selector other than 0 or 1; on a woven triangle a value that is not finite,
// E1, E2 or G12 <= 0, nu12^2 >= E1 / E2 (the law is positive definite iff E1, E2, G12 > 0 and nu12^2 < E1 / E2), a bend factor <= 0, a direction of zero
// length, or a direction whose projection into the rest plane is shorter than 1e-6 of its length (normal to the triangle: it names no direction in it).
// All selectors zero (or null): true with nWoven == 0, the empty plan.
bool buildShellWeavePlan(const ShellPlan& shell, int nV, const double* Vrest, const int* woven, const double* dir, const double* E1, const double* E2,
    const double* G12, const double* nu12, const double* bendWarp, const double* bendWeft, ShellWeavePlan& plan, std::string& err);

// triConst (SoA [6][nTri]) with the two StVK constants (rows 4 and 5) of the plan's woven triangles set to zero: applied behind shellTriConstWithoutRubber, it
// is what the StVK kernels read while the plan is set, so that they add exact zeros there
std::vector<double> shellTriConstWithoutWeave(const std::vector<double>& triConst, const ShellWeavePlan& plan);

// row 1 of hingeConst, bendScale k_b w_e per hinge, times the plan's factor; without a woven triangle (or with every factor 1) bit for bit the shell plan's
std::vector<double> shellHingeStiffnessWithWeave(const ShellPlan& shell, double bendScale, const ShellWeavePlan& plan);

} // namespace ipcgpu
