// The signed dihedral angle of a shell hinge and (optionally) its gradient: THE device function of the bending energy (shell_kernels.hip) and of the
// hinge's plastic flow (shell_plastic_kernels.hip), defined once so that both read the same theta.  __forceinline__, and it takes the including unit's
// -ffp-contract setting.  For .hip files only.
#pragma once
#include "stencil_hessian_device.h"

namespace ipcgpu {

// theta and (optionally) its gradient g[4][3] with respect to x0 .. x3
template <bool GRAD>
__device__ __forceinline__ double hinge_angle(const double* x0, const double* x1, const double* x2, const double* x3, double (*g)[3])
{
    double e[3], a[3], b[3], c[3], n1[3], n2[3], nn[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        e[i] = x1[i] - x0[i];
        a[i] = x2[i] - x0[i];
        b[i] = x0[i] - x1[i];
        c[i] = x3[i] - x1[i];
    }
    sh::cross(e, a, n1);
    sh::cross(b, c, n2);
    sh::cross(n1, n2, nn);
    const double le = sqrt(sh::dot(e, e));
    const double theta = atan2(sh::dot(nn, e) / le, sh::dot(n1, n2));
    if constexpr (GRAD) {
        // grad theta (closed form): x2: -|e| n1 / |n1|^2, x3: -|e| n2 / |n2|^2,
        // x0: ((x1 - x2) . e / |e|) n1 / |n1|^2 + ((x1 - x3) . e / |e|) n2 / |n2|^2, x1: ((x2 - x0) . e / |e|) n1 / |n1|^2 + ((x3 - x0) . e / |e|) n2 / |n2|^2
        const double i1 = 1.0 / sh::dot(n1, n1), i2 = 1.0 / sh::dot(n2, n2), ile = 1.0 / le;
        double d12 = 0.0, d13 = 0.0, d20 = 0.0, d30 = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            d12 += (x1[i] - x2[i]) * e[i];
            d13 += (x1[i] - x3[i]) * e[i];
            d20 += a[i] * e[i];
            d30 += (x3[i] - x0[i]) * e[i];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double a1 = n1[i] * i1, a2 = n2[i] * i2;
            g[0][i] = (d12 * a1 + d13 * a2) * ile;
            g[1][i] = (d20 * a1 + d30 * a2) * ile;
            g[2][i] = -le * a1;
            g[3][i] = -le * a2;
        }
    }
    return theta;
}

} // namespace ipcgpu
