// Pressure chambers (gfx950, fp64): a constant gas pressure inside closed surfaces -- a balloon, a cushion, a hollow body under outside pressure.  A project
// extension: the reference has none.  The host side (validation, rest volume, rest reference point, neighbour pairs) is chamber_plan.h.
//
// A chamber is a closed, consistently oriented set of triangles (outward normals by the right-hand rule) over ANY nodes of the mesh: shell nodes, surface
// nodes of tetrahedral components, scripted nodes.  It may consist of several closed pieces.  Chamber c holds the constant gauge pressure p_c: positive
// pushes outward, negative is suction or an outside hydrostatic pressure.  With a reference point r_c that is constant during any one evaluation and
// y_i = x_i - r_c:
//     V_c = 1/6 sum_t y0 . (y1 x y2)            the enclosed volume, over the chamber's triangles
//     W_c = -p_c V_c,   per triangle  W_t = -(p_c / 6) y0 . (y1 x y2)
//     dW_t/dx0 = -(p/6) y1 x y2,   dW_t/dx1 = -(p/6) y2 x y0,   dW_t/dx2 = -(p/6) y0 x y1          (exact: the load follows the surface)
//     9 x 9 Hessian of a triangle: zero diagonal blocks,  H01 = (p/6) [y2]x,  H02 = -(p/6) [y1]x,  H12 = (p/6) [y0]x   ([v]x w = v x w)
//   The Hessian is indefinite (its trace is 0).  It is projected to PSD PER TRIANGLE by the cyclic Jacobi iteration of jacobi9_device.h on the full 9 x 9
//   block (the triple product is not invariant under a translation of one triangle, so there is no 6-dimensional complement to work in).
// Why r_c exists: for a closed surface V_c and its gradient do not depend on r_c in exact arithmetic, but the per-triangle Hessian does -- its entries grow
//   with |y|, and a per-triangle projection about the world origin would add a spurious stiffness proportional to the body's distance from the origin.
// The rule for r_c: the mean of the centroids of the chamber's triangles.  ipcgpu_set_chambers computes it at the rest positions (chamber_plan.h);
//   ipcgpu_opt_begin_timestep refreshes it on the device from the positions the step starts from (launch_chamber_state); it stays fixed through that step's
//   Newton iterations and line searches, so every energy comparison inside a step uses one r_c.  ipcgpu_set_positions does not move it.
// NOT modelled:
//   * a gas law (pressure as a function of the volume).  Its Hessian has a dense rank-one term per chamber, beta gradV gradV^T, that for real air on cloth
//     dominates every other stiffness: omitting it stalls Newton and lagging the pressure per step is unstable.  It needs a low-rank correction inside the
//     linear solve.  Until then ipcgpu_chamber_set_pressure and ipcgpu_chamber_state let a caller drive the pressure between time steps.
//   * open chambers closed by a plane;  * the mass of the enclosed gas;  * any change to contact.
// The term is no stiffness: it does not enter the lagged stiffness damping (HipOptimizer::assembleDampingMtr masks it out).
//
// One lane per triangle, ids and y in registers.  Gradient entries and the 3 diagonal + 3 off-diagonal projected blocks go into the nodal vector and the upper
// CSR by fp64 atomicAdd through the row lookup of csr_scatter_device.h.  Rows, columns and gradient entries of projected Dirichlet nodes are dropped
// (projected_dbc).  A triangle of a chamber with p_c == 0 issues no atomic.
#pragma once
#include "codim_view.h"
#include <hip/hip_runtime.h>

namespace ipcgpu {

struct ChamberFields {
    int nTri;
    int n; // chambers
    const int* tri; // SoA [3][nTri]
    const int* chamberOf; // nTri
    const int* triEnd; // n: chamber c owns the triangles [triEnd[c - 1], triEnd[c])
    const double* pressure; // n
    const double* ref; // 3 n: r_c
};
struct ChamberView : ChamberFields, CodimBase {}; // (the shared fields behind the term's own: codim_view.h)

int chamber_energy_blocks(const ChamberView& v); // partial sums launch_chamber_energy writes
// *out (device) = (accumulate ? *out : 0) + coef * (sum of W_t); partial: chamber_energy_blocks(v) doubles.  Deterministic: fixed order.
void launch_chamber_energy(const ChamberView& v, double coef, double* partial, double* out, bool accumulate, hipStream_t s);
void launch_chamber_energy_per_elem(const ChamberView& v, double* perTri, hipStream_t s);
// grad (nullable) += coef * gradient; a (nullable) += coef * PSD Hessian blocks.  *err |= 1 where the pattern lacks a block (device int).
void launch_chamber_assemble(const ChamberView& v, double coef, int projectDBC, double* grad, double* a, int* err, hipStream_t s);
// Per chamber, at v.x: refPoint[3 c ..] the mean of the triangle centroids, volume[c] and area[c] (the volume taken about THAT point, whatever v.ref holds).
// Any pointer may be null; refPoint may be the buffer behind v.ref (the kernel never reads v.ref): that is the stepper's refresh of r_c.
// A segmented reduction in a fixed order: one workgroup per chamber strides over its triangle range, then a tree in LDS.  Deterministic.
void launch_chamber_state(const ChamberView& v, double* volume, double* area, double* refPoint, hipStream_t s);

} // namespace ipcgpu
