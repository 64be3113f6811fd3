// Elastic rods on segment components (gfx950, fp64): stretching and bending energy, their gradients and PSD Hessians.  A project extension: the
// reference has no rods.  The host side (validation, rest constants, bending triples, masses, neighbour pairs) is rod_plan.h.
//
// Stretching, per segment (a, b): rest length L, current length l, radius r, Young's modulus E, A = pi r^2, k_s = E A / L,  W_s = k_s (l - L)^2 / 2.
//   The gradient is exact.  With t = (x_b - x_a) / l the 3 x 3 block is B = k_s [t t^T + max(0, 1 - L / l) (I - t t^T)] and the 6 x 6 Hessian
//   [[B, -B], [-B, B]].  The clamp at 0 IS the eigenvalue projection of the full Hessian, whose spectrum is 2 k_s, 2 k_s (1 - L / l) twice and 0 three
//   times: no eigen-iteration.  A segment collapsed to a point (l = 0) has no direction: it contributes its energy, no force and no block.
// Bending, per interior node b (exactly two incident segments (a, b), (b, c)): e0 = x_b - x_a, e1 = x_c - x_b, the discrete curvature binormal
//   kb = 2 e0 x e1 / d,  d = |e0||e1| + e0 . e1,  W_b = bendScale k_b |kb|^2,  k_b = E_m I / (L0 + L1),  I = pi r_m^4 / 4  (means of the two segments):
//   the bending term of discrete elastic rods without twist (|kb| = 2 tan(theta / 2)), with a STRAIGHT rest state.  |kb|^2 is evaluated as
//   4 (|e0||e1| - e0 . e1) / d, |e0||e1| as sqrt(|e0|^2 |e1|^2).  The gradient 2 bendScale k_b J^T kb is exact, J = d kb / d (x_a, x_b, x_c) (3 x 9):
//     d kb / d e0 = (-2 [e1]_x - kb (|e1| t0 + e1)^T) / d,   d kb / d e1 = (2 [e0]_x - kb (|e0| t1 + e0)^T) / d,   columns -d e0, d e0 - d e1, d e1.
//   The Hessian is the Gauss-Newton term 2 bendScale k_b J^T J: rank <= 3, PSD by construction (the choice the shell's hinge made).
//   W_b grows without bound as the node folds flat (d -> 0): that keeps two adjacent segments, which share a node and form no contact pair, from folding
//   onto each other.  Where d <= 0 in floating point the energy of the node is +infinity (never NaN) and the node writes no gradient and no block: the
//   line search rejects such a trial point (hip_optimizer.cpp, lineSearch).
// Not modelled: twist and material frames, rest curvature, bending at junctions (three or more segments at a node: stretching only).
//
// One lane per segment / per bending triple, constants as SoA.  Gradient entries and 3 x 3 blocks go into the nodal vector and the upper CSR by fp64
// atomicAdd through the row lookup of csr_scatter_device.h (3 upper blocks per segment, 6 per triple); rows, columns and gradient entries of projected
// Dirichlet nodes are dropped (Energy.cpp:402-407), the diagonal identity stays with the node pass of the elastic assembly.
#pragma once
#include "codim_view.h"
#include <hip/hip_runtime.h>

namespace ipcgpu {

struct RodFields {
    int nSeg, nBend;
    const int2* seg; // nSeg: a, b
    const double* segConst; // SoA [2][nSeg]: L, k_s (rod_plan.h)
    const int* bend; // SoA [3][nBend]: a, b, c
    const double* bendConst; // nBend: bendScale k_b
};
struct RodView : RodFields, CodimBase {}; // (the shared fields behind the term's own: codim_view.h)

int rod_energy_blocks(const RodView& v); // partial sums launch_rod_energy writes
// *out (device) = (accumulate ? *out : 0) + coef * (stretching + bending energy); partial: rod_energy_blocks(v) doubles.  Deterministic: fixed order.
void launch_rod_energy(const RodView& v, double coef, double* partial, double* out, bool accumulate, hipStream_t s);
void launch_rod_energy_per_elem(const RodView& v, double* perSeg, double* perBend, hipStream_t s);
// grad (nullable) += coef * gradient; a (nullable) += coef * PSD Hessian blocks.  *err |= 1 where the pattern lacks a block (device int).
void launch_rod_assemble(const RodView& v, double coef, int projectDBC, double* grad, double* a, int* err, hipStream_t s);

} // namespace ipcgpu
