// Host side of the elastic shells (ipcgpu_set_shell; shell_kernels.hip): from the triangle list and the rest positions, everything the kernels read and the
// mesh has to know -- validated triangles, their rest-plane constants, the hinges of the interior edges with their rest angles, the lumped masses, and
// the node pairs that must be in vNeighbor so that the CSR pattern holds every block the shell Hessian writes.  Pure host arithmetic (no HIP header:
// tests/test_shell_plan_host.py builds it with g++).  The reference has no shells; the energies are stated in shell_kernels.h.
#pragma once
#include <string>
#include <vector>

namespace ipcgpu {

struct ShellPlan {
    int nTri = 0, nHinge = 0;
    std::vector<int> tri; // 3 nTri, node ids of triangle t at 3 t .. 3 t + 2, as given
    // SoA [6][nTri]: Dm^-1 (b00, b10, b01, b11: column-major 2 x 2, Dm = [X1 - X0, X2 - X0] in an orthonormal frame of the rest plane whose first axis runs
    // along X1 - X0), then h A mu and h A lambda_ps with mu = E / (2 (1 + nu)), lambda_ps = E nu / (1 - nu^2)
    std::vector<double> triConst;
    std::vector<double> area; // nTri rest areas
    std::vector<double> membraneK; // nTri: h A E, the scale of the strain-limit barrier (shell_limit_plan.h) and of the rubber membrane (shell_rubber_plan.h)
    std::vector<double> thickness; // nTri: h at rest, as given (ipcgpu_shell_thickness)
    // hinges: one per edge shared by two triangles, ascending by (smaller edge node, larger edge node).  hinge[4 i ..] = x0 < x1 on the edge, x2 the node
    // opposite in the triangle that traverses x0 -> x1, x3 the node opposite in the one that traverses x1 -> x0
    std::vector<int> hinge;
    std::vector<double> restAngle; // signed dihedral angle at rest (0 = flat)
    std::vector<double> hingeWeight; // w_e = 3 |e|^2 / (A1 + A2), rest quantities
    std::vector<double> hingeK; // k_b = mean over the two triangles of E h^3 / (24 (1 - nu^2))
    std::vector<double> mass; // nV: sum over the node's triangles of rho h A / 3 (0 for a node of no shell triangle)
    std::vector<char> isShellNode; // nV
    std::vector<int> pairs; // 2 per pair (lo, hi), lo < hi, sorted, unique: triangle edges and, per hinge, (x2, x3)
    double edgeLenSum = 0.0; // sum of the rest lengths of the 3 nTri triangle sides (mean side = edgeLenSum / (3 nTri))
};

// The signed dihedral angle of the hinge (x0, x1 | x2, x3): atan2((n1 x n2) . e / |e|, n1 . n2) with e = x1 - x0, n1 = e x (x2 - x0), n2 = (x0 - x1) x (x3 - x1).
// 0 for a flat hinge, in (-pi, pi]; not unwrapped.
double shellHingeAngle(const double x0[3], const double x1[3], const double x2[3], const double x3[3]);

// tri: column-major nTri x 3 (tri[t + nTri k] = node k of triangle t); Vrest: column-major nV x 3; thickness, YM, PR, rho: per triangle;
// tets: column-major nTet x 4 (may be null when nTet == 0).  false, with the reason in err and the plan empty: a node id out of range, a triangle that repeats
// a node, zero rest area, an edge shared by more than two triangles, two triangles that traverse a shared edge in the same direction, a shell node that
// belongs to a tetrahedron, or a thickness, E or rho that is not positive, or PR outside (-1, 1) (plane stress: lambda_ps = E nu / (1 - nu^2)).
bool buildShellPlan(int nV, int nTri, const int* tri, const double* Vrest, const double* thickness, const double* YM, const double* PR, const double* rho,
    int nTet, const int* tets, ShellPlan& plan, std::string& err);

} // namespace ipcgpu
