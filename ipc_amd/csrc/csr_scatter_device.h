// What the element-parallel kernels of the codimensional energies (shell_kernels.hip, shell_limit_kernels.hip, rod_kernels.hip) share: the Dirichlet
// projection rule, the scatter of 3 x 3 blocks into the upper CSR through the row lookup of the contact stencils, the fixed-order block sum of the energy
// kernels and the launch of their reduction.  For .hip files only.
#pragma once
#include <hip/hip_runtime.h>

namespace ipcgpu {
namespace scatter {

inline int nblk(int n, int block) { return (n + block - 1) / block; }

__device__ __forceinline__ bool projected_dbc(int type, int projectDBC) { return type == 1 || (type == 2 && projectDBC); }

__device__ __forceinline__ void ld3(const double* __restrict__ x, int v, double* p)
{
    p[0] = x[3 * (size_t)v];
    p[1] = x[3 * (size_t)v + 1];
    p[2] = x[3 * (size_t)v + 2];
}

// ---- scatter into the upper CSR (block rows of LinSysSolver.hpp:63-111: row 3 v has rowLen entries, 3 v + 1 one less, 3 v + 2 two less) -----------------------
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
        const int p = lo + (r == 0 ? 0 : (r == 1 ? Lr - 1 : 2 * Lr - 3));
#pragma unroll
        for (int c = 0; c < 3; ++c) atomicAdd(&k.a[p + c], swap ? A[c + 3 * r] : A[r + 3 * c]);
    }
}

// sum over the workgroup of BLOCK lanes, valid in lane 0; fixed-order tree: deterministic.  sm: BLOCK / 64 doubles of LDS
template <int BLOCK>
__device__ __forceinline__ double block_sum(double x, double* sm)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) sm[wv] = x;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) {
        for (int i = 0; i < BLOCK / 64; ++i) r += sm[i];
    }
    return r;
}

// the tail of an energy kernel: partial[blockIdx.x] = the sum of e over the workgroup
template <int BLOCK>
__device__ __forceinline__ void store_block_sum(double e, double* __restrict__ partial)
{
    __shared__ double sm[BLOCK / 64];
    const double r = block_sum<BLOCK>(e, sm);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

// out[0] = (accumulate ? out[0] : 0) + sum of the n partial sums, one workgroup of BLOCK lanes, fixed order
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_reduce_partials(const double* __restrict__ partial, int n, int accumulate, double* __restrict__ out)
{
    __shared__ double sm[BLOCK / 64];
    double x = 0.0;
    for (int i = threadIdx.x; i < n; i += BLOCK) x += partial[i];
    const double r = block_sum<BLOCK>(x, sm);
    if (threadIdx.x == 0) out[0] = accumulate ? out[0] + r : r;
}

inline void launch_reduce_partials(const double* partial, int n, bool accumulate, double* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_reduce_partials<256>, dim3(1), dim3(256), 0, s, partial, n, accumulate ? 1 : 0, out);
}

} // namespace scatter
} // namespace ipcgpu
