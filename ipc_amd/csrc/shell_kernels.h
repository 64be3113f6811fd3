// Elastic shells on triangle components (gfx950, fp64): membrane and bending energy, their gradients and PSD Hessians.  A project extension: the
// reference has no shells.  The host side (validation, rest constants, hinges, masses, neighbour pairs) is shell_plan.h.
//
// Membrane, per triangle: St. Venant-Kirchhoff in plane stress.  Dm = [X1 - X0, X2 - X0] in the rest plane (2 x 2), F = [x1 - x0, x2 - x0] Dm^-1 (3 x 2),
//   G = (F^T F - I) / 2,  psi = mu |G|_F^2 + lambda_ps tr(G)^2 / 2,  mu = E / (2 (1 + nu)),  lambda_ps = E nu / (1 - nu^2),  energy = h A psi.
//   The gradient is exact.  The 9 x 9 Hessian is projected to PSD per triangle: it annihilates the rigid translations, so it is formed as a 6 x 6 matrix in
//   the Helmert basis of their complement (stencil_hessian_device.h), projected there by the register-resident Jacobi iteration (jacobi9_device.h) and
//   expanded to the six upper node-pair blocks -- the same matrix as the projection of the 9 x 9 one.  The energy is a polynomial, finite for every
//   configuration: like FCR and SNH it needs no inversion check and no step filter.
// Bending, per interior edge: a discrete hinge with nodes (x0, x1) on the edge and (x2, x3) opposite, theta = the signed dihedral angle
//   atan2((n1 x n2) . e / |e|, n1 . n2), e = x1 - x0, n1 = e x (x2 - x0), n2 = (x0 - x1) x (x3 - x1), thetaBar the same at rest (a curved rest shape is
//   stress-free), energy = bendScale k_b w_e (theta - thetaBar)^2 with w_e = 3 |eBar|^2 / (A1 + A2) and k_b = E h^3 / (24 (1 - nu^2)) (mean of the two
//   triangles).  The gradient is exact (closed form of grad theta); the Hessian is the Gauss-Newton term 2 bendScale k_b w_e grad theta grad theta^T,
//   rank one and PSD by construction.  theta - thetaBar is NOT unwrapped: a hinge folded through +-pi is a self-intersection of the surface, which
//   contact prevents; without contact such a fold jumps by 2 pi.
//
// One lane per triangle / per hinge.  Gradient entries and 3 x 3 blocks go into the nodal vector and the upper CSR by atomicAdd, the block found by the
// same row lookup as the contact stencils use (binary search of column 3 * max in row 3 * min); rows, columns and gradient entries of projected Dirichlet
// nodes are dropped (Energy.cpp:402-407), the diagonal identity stays with the node pass of the elastic assembly.
#pragma once
#include "codim_view.h"
#include <hip/hip_runtime.h>

namespace ipcgpu {

struct ShellFields {
    int nTri, nHinge;
    const int* tri; // 3 nTri
    const double* triConst; // SoA [6][nTri]: Dm^-1 (b00, b10, b01, b11), h A mu, h A lambda_ps (shell_plan.h)
    const int4* hinge; // nHinge: x0, x1 on the edge, x2, x3 opposite
    const double* hingeConst; // SoA [2][nHinge]: thetaBar, bendScale k_b w_e
};
struct ShellView : ShellFields, CodimBase {}; // (the shared fields behind the term's own: codim_view.h)

int shell_energy_blocks(const ShellView& v); // partial sums launch_shell_energy writes
// *out (device) = (accumulate ? *out : 0) + coef * (membrane + bending energy); partial: shell_energy_blocks(v) doubles.  Deterministic: fixed order.
void launch_shell_energy(const ShellView& v, double coef, double* partial, double* out, bool accumulate, hipStream_t s);
void launch_shell_energy_per_elem(const ShellView& v, double* perTri, double* perHinge, hipStream_t s);
// grad (nullable) += coef * gradient; a (nullable) += coef * PSD Hessian blocks.  *err |= 1 where the pattern lacks a block (device int).
void launch_shell_assemble(const ShellView& v, double coef, int projectDBC, double* grad, double* a, int* err, hipStream_t s);

} // namespace ipcgpu
