// HipRoundCollider: analytic sphere / capsule obstacle, the second shape of HipVertexCollider (vertex_collider.h) beside HipHalfSpace.  A project
// extension: the reference has no such class, so tests/round_collider_mp.py (mpmath) is the reference.
//
// Shape (round_collider_plan.h): a segment [p0, p1], a radius R > 0, side = +1 (solid) or -1 (hollow sphere: the bodies live inside).
//
// Distance.  q(x) is the closest point of the segment to x: q = p0 + t a with t = clamp((x - p0) . a, 0, len), a the unit axis (t = 0 for a sphere).
//   r = |x - q|,  m = (x - q) / r,  s = side (r - R),  n = grad s = side m.
//   Region: "side" where 0 < (x - p0) . a < len strictly, "cap" otherwise (the end planes themselves, the axis extension, and every point of a sphere).
//   r = 0 (a vertex on the segment, s = -side R): m is taken as the zero vector, so nothing is NaN.  A hollow sphere has R^2 > dHat, so no ACTIVE
//   vertex has r = 0; on a solid collider r = 0 is an intersection, which the stepper refuses.
// Barrier.  kappa b(s^2, dHat) with cdev::barrier, evaluated as the half-space's kernels treat dist^2.
// Active set.  Surface vertices with dbc == 0 and s^2 < dHat, ascending surface-vertex order (HipVertexCollider::build).
// Gradient.  kappa b' 2 s n.
// Hessian.  kappa [ (4 b'' s^2 + 2 b') n n^T + 2 b' s side / r T ],  T = I - m m^T on a cap, T = I - m m^T - a a^T on the side.  n, a and the range of T
//   are mutually orthogonal eigen-directions, so clamping the two coefficients at 0 IS the PSD projection, in closed form.  b' < 0 inside dHat, so the
//   curvature term of a solid collider (side s > 0) is always dropped and that of a hollow sphere is kept.  Only the node's diagonal block is written.
// Step bound.  For every surface vertex with dbc == 0, the first t in (0, stepSize] with s(x + t p) = (1 - slackness) s(x): the ray against the
//   collider of radius R + side (1 - slackness) s(x).  Solid: the cylinder piece with its axial parameter in [0, len] and the two end spheres, the
//   smallest positive root; hollow sphere: the larger root of one quadratic.  A ray that never reaches the inflated surface does not bound the step.
// Intersection.  s <= 0 on any node with dbc == 0.
// Lagged friction.  lambda = -kappa b' 2 s per active vertex (the half-space's has sqrt(dist^2) for s), and the unit normal n of that vertex (the lagged tangent plane); energy,
//   gradient and Hessian are the half-space's with the per-entry lagged normal in place of the plane's.
// move(delta, slackness).  The collider is translated by the largest fraction <= 1 of delta that keeps `slackness` of every surface node's gap
//   (Dirichlet nodes included): the relative ray p = -delta through the step-bound routine.  Returns the fraction left, like HipHalfSpace::move.
// state.  Set size, the smallest s over the surface nodes, the total barrier force on the bodies, its torque about p0 and the total lagged friction
//   force, summed in a fixed order (block_sum, k_reduce_partials): two calls agree to the bit.
// The contact report (ipcgpu_contact_report) does not list round colliders: `state` serves that purpose.
//
// Kernels: the templates of vertex_collider.hip on RoundShape (k_vc_*<RoundShape>, and k_vc_fric_*<LaggedNormal> for the friction terms); k_vc_min_dist,
// k_rc_state and k_vc_fric_state serve `state` alone.  Resources (tools/kernel_resources.py, gfx950, 256 lanes, no scratch): see DESIGN.md section 4.
#pragma once
#include "vertex_collider.h"
#include "round_collider_plan.h"
#include <memory>

namespace ipcgpu {

class HipRoundCollider : public HipVertexCollider {
public:
    static std::unique_ptr<HipRoundCollider> create(hipStream_t s, const RoundShape& shape);
    RoundShape shape;
    // out10: smallest s over the surface nodes (+infinity without one), barrier force[3], its torque about p0[3], lagged friction force[3] (zero when
    // eps2 <= 0 or nothing is lagged); returns the set size
    int state(int nSVI, const int* svi_dev, const double* x_dev, const double* xt_dev, double dHat, double kappa, double eps2, double* out10);

protected:
    HipRoundCollider(hipStream_t s, const RoundShape& shape) : HipVertexCollider(s), shape(shape) {}
};

} // namespace ipcgpu
