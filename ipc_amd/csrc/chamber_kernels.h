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
// The gas law (ipcgpu_chamber_set_gas).  A chamber is either CONSTANT (above, the default) or GAS: an ideal gas with the ambient absolute pressure p_amb >= 0,
//   the exponent gamma >= 1 (1 isothermal, 1.4 adiabatic air) and the fill volume V0 > 0 (default: the rest volume).  p_c then is the gauge pressure the gas
//   has at V0: P0 = p_amb + p_c > 0, and ipcgpu_chamber_set_pressure between steps pumps gas in or out.  With V the enclosed volume about r_c:
//     P(V) = P0 (V0 / V)^gamma,   gauge(V) = P(V) - p_amb
//     W = -P0 V0 ln(V / V0) + p_amb (V - V0)                                  gamma == 1
//     W =  P0 V0 / (gamma - 1) ((V0 / V)^(gamma - 1) - 1) + p_amb (V - V0)    gamma  > 1
//     W = +infinity for V <= 0   (the line search backs off, as for the rod's exact fold; gauge and beta are reported as 0 there)
//     dW/dx = -gauge(V) gradV,    d2W/dx2 = -gauge(V) d2V/dx2 + beta gradV gradV^T,   beta = gamma P(V) / V > 0
//   The first Hessian term is the constant chamber's per-triangle block with p = gauge(V) at the current positions, projected as above: the assemble kernel
//   reads an EFFECTIVE pressure per chamber -- p_c of a constant chamber, written when the pressure is set; gauge(V_c) of a gas chamber, written by the gas
//   update, which is enqueued ahead of every assembly at the same positions.  The second term is PSD, rank one and DENSE: it never enters the CSR.  The stepper
//   applies it as a rank-k correction around the factor (k gas chambers, k <= 8; Woodbury):
//     (A + coef sum_c beta_c u_c u_c^T) d = r,  u_c = gradV_c:   y = A^-1 r,  z_c = A^-1 u_c,  C = diag(1 / (coef beta_c)) + U^T Z,  C w = U^T y,  d = y - Z w
//   ipcgpu_chamber_hessian_add and ipcgpu_assemble_newton add the sparse part only.
// The gas update is two passes, deterministic, without a floating-point atomic and without the host: the host plan cuts every gas chamber's triangle range
//   into slices of at most 256 triangles of one chamber (chamber_plan.h); pass 1, one 256-lane workgroup per slice, sums the triple products (a wave-level
//   reduction, then LDS across the four waves) into one partial per slice; pass 2, one wave per gas chamber, sums that chamber's partials in index order and
//   writes V_c, gauge_c, beta_c and W_c, gauge_c into the effective pressure, and adds coef W_c into the energy slot in chamber order.
// NOT modelled: open chambers closed by a plane;  the mass, the temperature and any leakage of the enclosed gas;  the rank-k term inside the operator of the
//   iterative solver (a context with a gas chamber refuses that solver);  any change to contact.
// The term is no stiffness: it does not enter the lagged stiffness damping (HipOptimizer::assembleDampingMtr masks it out), neither as a constant chamber
// nor as a gas chamber (its sparse part and its rank-one part both stay out).
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
    const double* pressure; // n: the effective pressure (p_c; with gas chambers see above)
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

// ---- the gas law -------------------------------------------------------------------------------------------------------------------------
struct ChamberGasView {
    int nGas, nSlice;
    const int* sliceBegin; // nSlice
    const int* sliceEnd; // nSlice
    const int* sliceOff; // nGas + 1
    const int* gasChamber; // nGas
    const double* param; // 3 n: ambient, gamma, fill volume of chamber c at 3 c
    const double* basePressure; // n: p_c
    double* slicePartial; // nSlice (pass 1 -> pass 2)
    double* effPressure; // n: pass 2 writes gauge_c of the gas chambers
    double* state; // 4 n: V, gauge, beta, W of chamber c at 4 c (gas chambers only are written)
};
// The gas update at v.x (the value of v.pressure is not used).  out (nullable): *out = (accumulate ? *out : 0) + coef * (W of the gas chambers, in chamber order).
void launch_chamber_gas_update(const ChamberView& v, const ChamberGasView& g, double coef, double* out, bool accumulate, hipStream_t s);
// perTri[t] = W_c V_t / V_c for the triangles of the gas chambers (the others are not touched).  isGas: n ints, state: 4 n doubles as the last gas
// update left them (ChamberGasView::state), both on the device.
void launch_chamber_gas_energy_per_elem(const ChamberView& v, const int* isGas, const double* state, double* perTri, hipStream_t s);
// u (n3 = 3 nV doubles, zeroed here) = gradV of ONE chamber: the gradient kernel with unit pressure.  select: n doubles, 1 at that chamber and 0 elsewhere.
// Entries of projected Dirichlet nodes are dropped, as in the gradient.
void launch_chamber_volume_gradient(const ChamberView& v, const double* select, int projectDBC, double* u, size_t n3, hipStream_t s);
// The rank-k correction, k = g.nGas <= 8.  U, Z: k vectors of n3 doubles each, y: n3, dots: chamber_gas_dot_doubles(n3, k) doubles, w: 8 doubles.
//   y -= Z w,  (diag(1 / (coef beta_c)) + U^T Z) w = U^T y;  the k + k (k + 1) / 2 dot products in a fixed order in two passes, the k x k Cholesky in one wave.
//   A chamber with beta_c == 0 (V_c <= 0) gets w_c = 0.
size_t chamber_gas_dot_doubles(size_t n3, int k);
void launch_chamber_gas_woodbury(const ChamberGasView& g, double coef, size_t n3, const double* U, const double* Z, double* y, double* dots, double* w, hipStream_t s);

} // namespace ipcgpu
