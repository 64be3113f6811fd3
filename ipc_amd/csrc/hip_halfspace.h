// HipHalfSpace: analytic half-space obstacle of the hot path with its vertex constraint set in HBM.
//   HalfSpace::init                              src/CollisionObject/HalfSpace.cpp:41-85
//   CollisionObject::computeConstraintSet        src/CollisionObject/CollisionObject.h:323-351   -> build
//   evaluateConstraint + barrier energy          HalfSpace.cpp:106-111, Optimizer.cpp:3254-3267  -> energy
//   leftMultiplyConstraintJacobianT              HalfSpace.cpp:121-143                           -> gradientAdd
//   augmentIPHessian                             HalfSpace.cpp:169-214                           -> hessianAdd
//   largestFeasibleStepSize                      HalfSpace.cpp:242-269                           -> stepBound
//   CollisionObject::isIntersected               CollisionObject.h:386-401                       -> intersected
//   HalfSpace::move                              HalfSpace.cpp:389-416                           -> move
// The methods are HipVertexCollider's (vertex_collider.h); the kernels are the templates of vertex_collider.hip on hsdev::Plane (halfspace_device.h).
#pragma once
#include "vertex_collider.h"
#include <memory>

namespace ipcgpu {

class HipHalfSpace : public HipVertexCollider {
public:
    static std::unique_ptr<HipHalfSpace> create(hipStream_t s, const double* origin3, const double* normal3);
    double n[3], D, origin[3];

protected:
    HipHalfSpace(hipStream_t s, const double* origin3, const double* normal3);
};

} // namespace ipcgpu
