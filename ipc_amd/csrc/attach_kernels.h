// Attachments (gfx950, fp64): springs that tie a point A of the mesh to a point B -- stitches (rest length 0) and tethers (rest length > 0).  A project
// extension: the reference has none.  The host side (validation, merged stencils, neighbour pairs) is attach_plan.h.
//
// Each point is a fixed convex combination of one to three nodes (a node, a point on an edge, a point in a triangle) of ANY components: tetrahedral, shell,
// rod, scripted or obstacle nodes, the same component included.  The plan merges the two points into up to six distinct nodes with signed coefficients
// c_i = weight in A - weight in B (sum c_i = 0).  Per attachment, with stiffness k > 0 (a force per length, the caller's: no material scales it) and rest
// length L >= 0:
//     d = sum_i c_i x_i,  l = |d|,  W = k (l - L)^2 / 2,  grad_i = k (l - L) c_i t,  t = d / l,
//     H_ij = c_i c_j B,   B = k [t t^T + max(0, 1 - L / l) (I - t t^T)].
//   The full Hessian is (c c^T) (x) B_full, its eigenvalues |c|^2 times those of B_full: k, and k (1 - L / l) twice.  So the clamp at 0 IS the eigenvalue
//   projection in closed form (the argument of the rod's stretching term, rod_kernels.h): no eigen-iteration.
//   L == 0 (a stitch): W = k |d|^2 / 2, grad_i = k c_i d, B = k I -- evaluated without a square root or a division, well defined at d = 0.
//   L > 0 and l == 0: no direction.  The attachment contributes its energy k L^2 / 2, no force and no block (the rod's rule for a collapsed segment).
//   No state yields NaN.
// Contact is NOT changed: attached bodies still form contact pairs, so a zero-length stitch between two different surfaces settles at a gap below dHat with
// the barrier active.  That is legal; a caller who wants none of it masks the pair of bodies with the contact groups (ipcgpu_set_contact_groups) or gives
// the attachment a rest length.
//
// One lane per attachment, constants as SoA, the loops over the six slots unrolled at compile time (ids and coefficients stay in registers).  Gradient
// entries and 3 x 3 blocks go into the nodal vector and the upper CSR by fp64 atomicAdd through the row lookup of csr_scatter_device.h: at most 6 diagonal
// and 15 off-diagonal blocks; a slot with coefficient 0 (the padding) issues no load and no atomic.  Rows, columns and gradient entries of projected
// Dirichlet nodes are dropped (projected_dbc): an attachment to a scripted collider pulls the free side only.
#pragma once
#include "codim_view.h"
#include <hip/hip_runtime.h>

namespace ipcgpu {

struct AttachFields {
    int n;
    const int* node; // SoA [6][n]: distinct node ids, padding slots repeat slot 0 (attach_plan.h)
    const double* coef; // SoA [6][n]: signed coefficients, 0 in the padding slots
    const double* kL; // SoA [2][n]: k, L
};
struct AttachView : AttachFields, CodimBase {}; // (the shared fields behind the term's own: codim_view.h)

int attach_energy_blocks(const AttachView& v); // partial sums launch_attach_energy writes
// *out (device) = (accumulate ? *out : 0) + coef * (sum of W); partial: attach_energy_blocks(v) doubles.  Deterministic: fixed order.
void launch_attach_energy(const AttachView& v, double coef, double* partial, double* out, bool accumulate, hipStream_t s);
void launch_attach_energy_per_elem(const AttachView& v, double* perAttach, hipStream_t s);
// grad (nullable) += coef * gradient; a (nullable) += coef * PSD Hessian blocks.  *err |= 1 where the pattern lacks a block (device int).
void launch_attach_assemble(const AttachView& v, double coef, int projectDBC, double* grad, double* a, int* err, hipStream_t s);
// per attachment the current length l = |d| and the signed force k (l - L) (positive: pulling the points together); either may be null
void launch_attach_state(const AttachView& v, double* length, double* force, hipStream_t s);

} // namespace ipcgpu
