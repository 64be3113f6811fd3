// Host side of the strain limit of the elastic shells (ipcgpu_shell_set_strain_limit; shell_limit_kernels.hip): validates the per-triangle limit, onset and
// stiffness and builds what the kernels read -- the compact list of the limited triangles with their constants, and the limit per triangle of the whole shell
// for the stretch query.  Pure host arithmetic (no HIP header: tests/test_shell_limit_plan_host.py builds it with g++).  The energy is stated in
// shell_limit_kernels.h.
#pragma once
#include <string>
#include <vector>

namespace ipcgpu {

struct ShellLimitPlan {
    int nTri = 0, nLimited = 0;
    std::vector<int> tri; // nLimited: ascending indices of the triangles with limit > 0
    std::vector<double> limConst; // SoA [3][nLimited]: onset, limit, k = stiff h A E
    std::vector<double> triLimit; // nTri: the limit of triangle t, 0 where it has none (empty when nLimited == 0)
};

// limit: per triangle, 0 = unlimited (null: every triangle unlimited); onset, stiff: per triangle, null = 1 everywhere (read only where limit > 0);
// membraneK: h A E per triangle (ShellPlan::membraneK).  false, with the reason in err and the plan empty: a limit, or the onset or stiffness of a limited
// triangle, that is not finite; a negative limit; 0 < limit <= onset; onset < 1; stiff <= 0.  All limits zero (or null): true with nLimited == 0.
bool buildShellLimitPlan(int nTri, const double* limit, const double* onset, const double* stiff, const double* membraneK, ShellLimitPlan& plan, std::string& err);

} // namespace ipcgpu
