// Wind and air drag on shells and body surfaces (gfx950, fp64): a load that depends on how a surface faces the air and how fast it moves through it -- a
// sheet that sinks instead of dropping, a flag, a parachute, a balloon that slows down.  A project extension: the reference has none.  The host side
// (validation, rest records, neighbour pairs) is aero_plan.h.
//
// An aerodynamic surface is a list of triangles over ANY nodes of the mesh: shell triangles, boundary faces of tetrahedral components; it need not be
// closed.  Surface s has a normal coefficient Cn >= 0, a tangential coefficient Ct >= 0 and a flag oneSided; globally there is a wind velocity w, uniform in
// space and settable between steps, and an air density rho_a > 0 (defaults: still air, 1.225).
// Per triangle t, LAGGED at the positions the time step starts from: the unit normal n (right-hand rule), the area A and the centroid c^n.
//   ipcgpu_set_aero computes them at the rest positions (aero_plan.h); ipcgpu_opt_begin_timestep refreshes them on the device (launch_aero_refresh) before
//   any scripted move; they stay fixed through that step's Newton iterations and line searches, so every energy comparison inside a step uses one record.
//   ipcgpu_set_positions does not move them (the rule of the chambers' r_c).
// At positions x, with the step size dt:
//     c   = ((x0 + x1) + x2) / 3
//     u   = (c - c^n) / dt - w                     the velocity of the triangle against the air, at the END of the step
//     u_n = u . n,   u_t = u - u_n n
//     s_n = u_n (two-sided),  max(0, u_n) (one-sided: only the face that pushes into the air is loaded)
//     D_t = dt (rho_a A / 6) (Cn |s_n|^3 + Ct |u_t|^3)                                      a convex dissipative potential (as the lagged friction's)
//     -dD_t/dc = -(rho_a A / 2) (Cn |s_n| s_n n + Ct |u_t| u_t)                             the force on the centroid; a third of it on each node
//     K = d2D_t/dc2 = (rho_a A / (2 dt)) (2 Cn |s_n| n n^T + Ct (|u_t| P + u_t u_t^T / |u_t|)),  P = I - n n^T
//   K is the exact Hessian and PSD as it stands: no clamp, no eigen-iteration.  Each of the nine 3 x 3 nodal blocks of the triangle's 9 x 9 Hessian is K / 9.
//   At |u_t| = 0 the tangential part is exactly zero, at s_n = 0 the normal part; a triangle whose lagged area is zero contributes nothing.  Where K (or the
//   force) vanishes altogether the kernels issue no atomic; no kernel produces NaN or Inf from finite input.  u = 0 is no edge case: it is the first
//   Newton iterate of every step in still air.
// D enters the stepper and the building blocks wherever the elastic codimensional terms do, with the same coefficient.  Under Newmark the velocity the term
//   sees is still (x - x^n) / dt (the lagged friction makes the same choice): the load is then first order in time.
// Rows, columns and gradient entries of projected Dirichlet nodes are dropped (projected_dbc); their motion still counts in c.
// The term is no stiffness: it does not enter the lagged stiffness damping (its bit is not in HipOptimizer::CODIM_STIFFNESS).  Contact is not changed.
// NOT modelled: lift other than the normal component of flat-plate drag;  shading of one surface by another;  wind that varies in space;  rods;  sharded
//   contexts (refused both ways round, as for shells).
//
// One lane per triangle, ids SoA, the lagged record eight doubles (n, A, c^n, pad) read as four aligned 16-byte loads.  The gradient (one 3-vector, the
// same for the three nodes) and the 3 diagonal + 3 upper off-diagonal blocks (all K / 9: six distinct entries) go into the nodal vector and the upper CSR
// by fp64 atomicAdd through csr_scatter_device.h: 9 + 45 adds per triangle, as a chamber triangle, behind a few dozen flops instead of a Jacobi iteration.
#pragma once
#include "codim_view.h"
#include <hip/hip_runtime.h>

namespace ipcgpu {

struct AeroFields {
    int nTri;
    int n; // surfaces
    const int* tri; // SoA [3][nTri]
    const int* surfOf; // nTri
    const double* coef; // 4 n: Cn, Ct, oneSided (0 or 1), pad of surface s at 4 s
    const double* lagged; // 8 nTri: n (3), A, c^n (3), pad of triangle t at 8 t; 16-byte aligned
    double wind[3];
    double density; // rho_a
    double dt;
};
struct AeroView : AeroFields, CodimBase {}; // (the shared fields behind the term's own: codim_view.h)

// lagged[8 t ..] (device, 8 v.nTri doubles, may be the buffer behind v.lagged: the kernel never reads v.lagged) = the record of triangle t at v.x
void launch_aero_refresh(const AeroView& v, double* lagged, hipStream_t s);
int aero_energy_blocks(const AeroView& v); // partial sums launch_aero_energy and launch_aero_state write per quantity
// *out (device) = (accumulate ? *out : 0) + coef * (sum of D_t); partial: aero_energy_blocks(v) doubles.  Deterministic: fixed order.
void launch_aero_energy(const AeroView& v, double coef, double* partial, double* out, bool accumulate, hipStream_t s);
void launch_aero_energy_per_elem(const AeroView& v, double* perTri, hipStream_t s); // the unscaled D_t
// grad (nullable) += coef * gradient; a (nullable) += coef * Hessian blocks.  *err |= 1 where the pattern lacks a block (device int).
void launch_aero_assemble(const AeroView& v, double coef, int projectDBC, double* grad, double* a, int* err, hipStream_t s);
// At v.x: force (nullable, 3 v.nTri) the force -dD_t/dc on every triangle; total5 (nullable) = total force (3), the dissipated power sum -f . u (>= 0), the
// loaded area (the lagged area of the triangles that carry a force).  partial: 5 aero_energy_blocks(v) doubles.  Two passes in a fixed order, no
// floating-point atomic, no host read-back: bit-reproducible.
void launch_aero_state(const AeroView& v, double* force, double* partial, double* total5, hipStream_t s);

} // namespace ipcgpu
