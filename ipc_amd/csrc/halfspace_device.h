// Device functions of the half-space obstacle that more than one translation unit uses: the kernels of vertex_collider.hip and the contact report of
// hip_contact.hip (both compiled with -ffp-contract=off, so the signed distance has the same bits in both).
#pragma once
#include <hip/hip_runtime.h>

namespace ipcgpu {
namespace hsdev {

struct Plane {
    double n0, n1, n2, D;
};
__device__ __forceinline__ double plane_dist(const Plane& h, const double* __restrict__ x, int v)
{
    return h.n0 * x[3 * (size_t)v] + h.n1 * x[3 * (size_t)v + 1] + h.n2 * x[3 * (size_t)v + 2] + h.D;
}

} // namespace hsdev
} // namespace ipcgpu
