// The atomic scatter of 3 x 3 blocks into the upper CSR through the row lookup of the contact stencils, for the element-parallel kernels of the codimensional
// energies (shell_kernels, shell_limit_kernels, shell_rubber_kernels, rod_kernels, attach_kernels, chamber_kernels).  Those units take everything else they share
// -- the Dirichlet projection rule, the fixed-order reductions and their launch, nblk, block_row_off -- from device_prims.h through this header.  For .hip files only.
#pragma once
#include "device_prims.h"

namespace ipcgpu {
namespace scatter {

using prims::block_row_off;
using prims::block_sum;
using prims::launch_reduce_partials;
using prims::nblk;
using prims::projected_dbc;
using prims::store_block_sum;
using prims::wave_max;
using prims::wave_sum;

__device__ __forceinline__ void ld3(const double* __restrict__ x, int v, double* p)
{
    p[0] = x[3 * (size_t)v];
    p[1] = x[3 * (size_t)v + 1];
    p[2] = x[3 * (size_t)v + 2];
}

struct CsrSink {
    const int* rowBase;
    const int* rowLen;
    const int* ja;
    double* a;
    int* err;
};
// upper triangle of the diagonal block of node n; A[r + 3 c]
__device__ __forceinline__ void add_diag(const CsrSink& k, int n, const double* A)
{
    const int base = k.rowBase[n], Lr = k.rowLen[n];
    atomicAdd(&k.a[base + 0], A[0]);
    atomicAdd(&k.a[base + 1], A[3]);
    atomicAdd(&k.a[base + 2], A[6]);
    atomicAdd(&k.a[base + Lr + 0], A[4]);
    atomicAdd(&k.a[base + Lr + 1], A[7]);
    atomicAdd(&k.a[base + 2 * Lr - 1], A[8]);
}
// block with rows of node nk and columns of node nl (nk != nl); A[r + 3 c].  The upper CSR holds (min, max): transposed when nl comes first.
__device__ __forceinline__ void add_off(const CsrSink& k, int nk, int nl, const double* A)
{
    const bool swap = nk > nl;
    const int rn = swap ? nl : nk, cn = swap ? nk : nl;
    const int base = k.rowBase[rn], Lr = k.rowLen[rn];
    int lo = base + 3, hi = base + Lr; // neighbour blocks start behind the 3 diagonal-block entries
    const int end = hi, target = 3 * cn;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (k.ja[mid] < target) lo = mid + 1;
        else hi = mid;
    }
    if (!(lo < end && k.ja[lo] == target)) {
        atomicOr(k.err, 1); // the pattern lacks this pair: the energy must be set before the pattern is built
        return;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int p = lo + block_row_off(r, Lr);
#pragma unroll
        for (int c = 0; c < 3; ++c) atomicAdd(&k.a[p + c], swap ? A[c + 3 * r] : A[r + 3 * c]);
    }
}

} // namespace scatter
} // namespace ipcgpu
