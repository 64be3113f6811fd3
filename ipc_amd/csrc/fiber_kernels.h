// Fibre reinforcement and active contraction of tetrahedral bodies (gfx950, fp64): tendon, wood grain, a cord ply, tissue that stiffens with stretch, a
// muscle or soft actuator that contracts on command.  A project extension: the reference has none (every body of it is isotropic).  The host side
// (validation, merged ranges, the compact lists) is fiber_plan.h.
//
// Per fibred tetrahedron t with rest volume vol, unit rest direction a and A_t = restTriInv:
//     F a = Ds(x) (A_t a) = sum_i c_i x_i,   b = A_t a,   c = (-(b1 + b2 + b3), b1, b2, b3)     (sum c_i = 0)
//     d = sum_i c_i x_i,   l = |d|  (the fibre stretch, I4 = l^2),   t = d / l
//     W = vol psi(l),   grad_i = vol psi'(l) c_i t,
//     H_ij = c_i c_j B,   B = vol [max(0, psi''(l)) t t^T + max(0, psi'(l) / l) (I - t t^T)].
//   The full Hessian is (c c^T) (x) B_full with B_full = vol [psi'' t t^T + (psi' / l) (I - t t^T)]; its eigenvalues are |c|^2 times those of B_full: vol psi''
//   once (eigenvector t) and vol psi' / l twice (the plane normal to t); the other nine are zero.  So the two clamps at 0 ARE the eigenvalue projection in
//   closed form (the argument of the attachment spring, attach_kernels.h, and of the rod's stretching term): no eigen-iteration.
//   The kernels evaluate d as b1 (x1 - x0) + b2 (x2 - x0) + b3 (x3 - x0), which is the same sum and exact under a translation.
// Two laws, chosen per call of ipcgpu_set_fibers:
//   law 0, spring:  psi = k (l - l0)^2 / 2,  psi' = k (l - l0),  psi'' = k.  l0 = 1 - act(group) > 0 is the active rest stretch of the element's activation
//     group: act = 0 is passive, act = 0.3 a muscle that wants to be 30 % shorter.  k is a stress (Pa), the caller's: no material scales it.
//     tensiononly: psi = 0 for l <= l0 -- the fibres buckle; the law stays C1 at l0.
//   law 1, exp (the Holzapfel-Gasser-Ogden fibre family):  psi = k / (2 k2) (exp(k2 (l^2 - 1)^2) - 1),  k2 > 0, with I = l^2 - 1 and e = exp(k2 I^2):
//     psi' = 2 k l I e,  psi'' = k e (2 I + 4 l^2 + 8 k2 l^2 I^2).  Always tension only: psi = 0 for l <= 1 (C1 there: psi'' jumps from 0 to 4 k, as the
//     tension-only spring's jumps from 0 to k at l0).  No activation: a group with act != 0 is refused on law-1 elements (fiber_plan.h).
// A lane whose psi' and psi'' are both zero (a tension-only or exp fibre in compression) issues NO atomic: gradient and matrix keep their bits.
// Degenerate states:
//   l == 0: no direction.  The element contributes its energy vol psi(0), no force and no block (the attachment's rule for l == 0).
//   The exponent overflows (or vol psi reaches the end of the fp64 range any other way): the energy is +inf, which the line search never accepts; never NaN.
//   Where vol psi' or vol psi'' is not finite the assembly issues nothing for the element, so no finite state yields NaN in energy, gradient or blocks.
// NOT modelled:  dispersion (HGO's kappa) and two fibre families in one element;  fibres in shells and rods;  fibres on an element that is also plastic
//   -- its A_t would flow under b -- refused both ways round (ipcgpu_set_fibers on a plastic element, ipcgpu_set_plasticity on a fibred one);  sharded
//   contexts, refused both ways round as for aero and plasticity;  the fibre part of the Cauchy stress: ipcgpu_elastic_stress stays the isotropic part;
//   the fibre energy in the per-component system report: ipcgpu_fiber_state gives the total instead.
//
// One lane per FIBRED element through the compact ascending list fibTet[nF]: a mesh with few fibres costs few lanes.  Constants are SoA over nF (b, vol k,
// k2, a flag word, the group); l0 is a separate array of FIBER_MAX_GROUPS doubles, so a new activation uploads that and nothing per element.  Exact sqrt
// and exp.  Gradient entries and 3 x 3 blocks go into the nodal vector and the upper CSR by fp64 atomicAdd through scatter::add_diag and add_off of
// csr_scatter_device.h (the row lookup; NOT ElemView::edgeP0): 4 x 3 + 4 x 6 + 6 x 9 = 90 atomic adds per element at most -- a node with c_i == 0 issues
// none.  All six node pairs of a tetrahedron are in every pattern, so the term adds no neighbour pair.  Rows, columns and gradient entries of projected
// Dirichlet nodes are dropped (projected_dbc).
#pragma once
#include "codim_view.h"
#include "fiber_plan.h"
#include <hip/hip_runtime.h>

namespace ipcgpu {

struct FiberFields {
    int nF;
    const int* fibTet; // nF: the fibred elements, ascending
    const int4* tet; // the mesh's elements (nT)
    const double* b; // SoA [3][nF]: A_t a
    const double* volK; // nF: vol k
    const double* k2; // nF (law 1; 0 otherwise)
    const int* flags; // nF: FIBER_FLAG_*
    const int* groupOf; // nF
    const double* l0; // FIBER_MAX_GROUPS: 1 - act per group
};
struct FiberView : FiberFields, CodimBase {}; // (the shared fields behind the term's own: codim_view.h)

constexpr int FIBER_STATE_COLS = 5; // l, psi'(l), t

int fiber_energy_blocks(const FiberView& v); // partial sums launch_fiber_energy writes
// *out (device) = (accumulate ? *out : 0) + coef * (sum of W); partial: fiber_energy_blocks(v) doubles.  Deterministic: fixed order.
void launch_fiber_energy(const FiberView& v, double coef, double* partial, double* out, bool accumulate, hipStream_t s);
void launch_fiber_energy_per_elem(const FiberView& v, double* perFiber, hipStream_t s); // nF doubles
// grad (nullable) += coef * gradient; a (nullable) += coef * PSD Hessian blocks.  *err |= 1 where the pattern lacks a block (device int).
void launch_fiber_assemble(const FiberView& v, double coef, int projectDBC, double* grad, double* a, int* err, hipStream_t s);
// Read-only.  perFiber (nullable; SoA [FIBER_STATE_COLS][nF]): l, the tension psi'(l) (a stress: vol psi' over vol[fibTet], vol the mesh's nT rest
// volumes) and the current direction t (0 0 0 where l == 0).  totals3 (nullable; device): min l, max l, sum of W in a fixed order;
// partial: 3 fiber_energy_blocks(v) doubles.
void launch_fiber_state(const FiberView& v, const double* vol, double* perFiber, double* partial, double* totals3, hipStream_t s);

} // namespace ipcgpu
