// The small device idioms that every kernel unit outside the direct solver shares, each defined once: the fixed-order wave and workgroup reductions
// and the kernel that sums their partials, the kernel that publishes a small result to mapped host memory, the Dirichlet projection rule, the launch
// grid size, and where the rows of a 3 x 3 block lie in the upper CSR.  Bit-reproducible energies, gradients and CSR values rest on every unit running
// the SAME reduction tree, hence one definition.
// Everything is __forceinline__ and takes the including unit's -ffp-contract setting; nothing here multiplies and adds, so that setting cannot
// change a bit -- keep arithmetic beyond add / min / max out of the helpers.  For .hip files only.
//   nh_kernels, hip_contact, vertex_collider, pcg        include this header
//   shell*, rod, attach, chamber kernels                 get it through csr_scatter_device.h (the atomic block scatter)
//   mf_numeric, mf_sweeps                                include it for the publish kernel alone
#pragma once
#include <hip/hip_runtime.h>
#include <cstring>
#include "common.h"

namespace ipcgpu {
namespace prims {

// workgroups of `block` lanes that cover n items
inline int nblk(long long n, int block) { return (int)((n + block - 1) / block); }

__device__ __forceinline__ bool projected_dbc(int type, int projectDBC)
{
    return type == 1 || (type == 2 && projectDBC); // Mesh.hpp:135-144
}

// ---- wave reductions: x = op(x, lane + off's x) for off = 32, 16, ..., 1 -- a fixed tree, the result is valid in lane 0 --------------------------------------
template <class T>
__device__ __forceinline__ T wave_sum(T x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
    return x;
}
__device__ __forceinline__ double wave_min(double x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = fmin(x, __shfl_down(x, off, 64));
    return x;
}
__device__ __forceinline__ double wave_max(double x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = fmax(x, __shfl_down(x, off, 64));
    return x;
}
__device__ __forceinline__ int wave_min(int x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = min(x, __shfl_down(x, off, 64));
    return x;
}
__device__ __forceinline__ int wave_max(int x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = max(x, __shfl_down(x, off, 64));
    return x;
}
// the butterfly: the sum in every lane
template <class T>
__device__ __forceinline__ T wave_sum_all(T x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

// ---- workgroup sum -----------------------------------------------------------------------------------------------------------------------------------------
// sum over the workgroup of BLOCK lanes, valid in lane 0: the wave tree, then the waves in index order.  sm: BLOCK / 64 doubles of LDS
template <int BLOCK>
__device__ __forceinline__ double block_sum(double x, double* sm)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64); // wave_sum, written out (see below)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) sm[wv] = x;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) {
        for (int i = 0; i < BLOCK / 64; ++i) r += sm[i];
    }
    return r;
}
// (block_sum does not call wave_sum: against the parent commit's code objects the call moves one instruction in every energy kernel, and this change
// was held to identical instruction streams for every kernel it does not merge.)
// the tail of an energy kernel: partial[blockIdx.x] = the sum of e over the workgroup
template <int BLOCK>
__device__ __forceinline__ void store_block_sum(double e, double* __restrict__ partial)
{
    __shared__ double sm[BLOCK / 64];
    const double r = block_sum<BLOCK>(e, sm);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}
// out[0] = (accumulate ? out[0] : nothing) + scale * (sum of the n partial sums): one workgroup, lane l takes partials l, l + BLOCK, ... in index order,
// then block_sum.  Callers without a scale pass exactly 1.0 (1.0 * r is r, sign of zero included); a plain store adds nothing, so -0.0 stays -0.0
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_reduce_partials(const double* __restrict__ partial, int n, double scale, int accumulate, double* __restrict__ out)
{
    __shared__ double sm[BLOCK / 64];
    double x = 0.0;
    for (int i = threadIdx.x; i < n; i += BLOCK) x += partial[i];
    const double r = scale * block_sum<BLOCK>(x, sm);
    if (threadIdx.x == 0) out[0] = accumulate ? out[0] + r : r;
}
template <int BLOCK = 256> // (a template: a unit that never calls it gets no kernel)
inline void launch_reduce_partials(const double* partial, int n, double scale, bool accumulate, double* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_reduce_partials<BLOCK>, dim3(1), dim3(BLOCK), 0, s, partial, n, scale, accumulate ? 1 : 0, out);
}

// ---- minimum of doubles through atomicMin ---------------------------------------------------------------------------------------------------------------------
// order-preserving map double -> uint64, so that atomicMin works for either sign; the cell starts at ~0ull
__device__ __forceinline__ unsigned long long ordered_bits(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
inline double from_ordered_bits(unsigned long long k)
{
    const unsigned long long b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    double v;
    std::memcpy(&v, &b, sizeof(v));
    return v;
}
// the tail of a minimum kernel: the wave tree, then one atomic per wave
__device__ __forceinline__ void atomic_min_wave(double best, unsigned long long* __restrict__ out)
{
    best = wave_min(best);
    if ((threadIdx.x & 63) == 0) atomicMin(out, ordered_bits(best));
}

// ---- read-backs through mapped host memory------------------------------------------------------------------------------------------------------------------
// dst[i] = src[i] for the nWords <= 64 32-bit words of a small result, one lane each: THE kernel that carries flags, counters and scalars from device memory
// to their mapped place on the host.  (k_publish2, k_publish_narrow and the tail of k_reduce_scaled stay where they are: two sources, or a gather.)
template <int WAVE = 64> // (a template, like k_reduce_partials: a unit that never launches it gets no kernel)
__global__ __launch_bounds__(WAVE) void k_publish_words(const unsigned* __restrict__ src, unsigned* __restrict__ dst, int nWords)
{
    const int i = threadIdx.x;
    if (i < nWords) dst[i] = src[i];
}
// `count` elements of T (publish_words, common.h)
template <class T>
inline void launch_publish(const T* src, T* dst, int count, hipStream_t s)
{
    hipLaunchKernelGGL(k_publish_words<64>, dim3(1), dim3(64), 0, s, reinterpret_cast<const unsigned*>(src), reinterpret_cast<unsigned*>(dst), publish_words<T>(count));
}

// ---- 3 x 3 node blocks in the upper CSR (LinSysSolver.hpp:63-111) ----------------------------------------------------------------------------------------------
// The three rows of node v start with the upper triangle of its diagonal block, then hold one block per neighbour w > v in ascending order: row 3 v has
// L entries starting at base, row 3 v + 1 starts at base + L and has L - 1, row 3 v + 2 starts at base + 2 L - 1 and has L - 2.  The six entries of
// the diagonal block are base, base + 1, base + 2, base + L, base + L + 1, base + 2 L - 1; they stay written out at their sites, and so does the search in
// scatter::add_off: in the code-object diff against the parent commit every helper form tried for them changed the instruction stream of the kernels.
// (The vertex colliders, whose kernels write nothing but this block, do share the write.)
// a[the diagonal block of the node whose row starts at p0 with L entries] += h6, the upper triangle row by row: 00 01 02 11 12 22
__device__ __forceinline__ void add_diag_block(double* __restrict__ a, int p0, int L, const double* h6)
{
    a[p0] += h6[0];
    a[p0 + 1] += h6[1];
    a[p0 + 2] += h6[2];
    a[p0 + L] += h6[3];
    a[p0 + L + 1] += h6[4];
    a[p0 + 2 * L - 1] += h6[5];
}
// row r of an off-diagonal block whose first entry is at p0 starts at p0 + block_row_off(r, L)
__device__ __forceinline__ int block_row_off(int r, int L) { return r == 0 ? 0 : (r == 1 ? L - 1 : 2 * L - 3); }
// Binary search for the block of neighbour cn in ja[lo, hi): lo = base + 3 (behind the diagonal block's entries) and hi = base + L of the node row.
// The position of the block's first entry, -1 if the pattern lacks the pair.
__device__ __forceinline__ int find_block(const int* ja, int lo, int hi, int cn)
{
    const int end = hi, target = 3 * cn;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ja[mid] < target) lo = mid + 1;
        else hi = mid;
    }
    return (lo < end && ja[lo] == target) ? lo : -1;
}

} // namespace prims
} // namespace ipcgpu
