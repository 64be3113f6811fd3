// Kernels of the preconditioned conjugate-gradient solver (pcg.h).  A bandwidth- and launch-bound path: the matrix is read once per iteration
// (8 B value + 4 B column per stored entry; the lower half comes from the same storage through a per-pattern index), the vectors once per
// pass, the scalars never leave the device, and nothing is accumulated with atomics -- two runs give the same bits.
#include "pcg.h"
#include "pcg_coarse.h"
#include "device_prims.h"
#include <algorithm>

namespace ipcgpu {

namespace {
constexpr int BLOCK = 256;
constexpr int GROUP = 16; // lanes that share one node block row of the product
constexpr int NODES_PER_BLOCK = BLOCK / GROUP;
constexpr int MAX_VEC_BLOCKS = 1024; // grid of the vector passes (grid-stride): at most this many partial sums per scalar

using prims::block_sum; // fixed-order tree: deterministic
// gate: 0 always, 1 while the iteration runs, 2 once it has ended
__device__ __forceinline__ bool gated_out(const PcgState* st, int gate)
{
    if (gate == 0) return false;
    const int done = st->done;
    return gate == 1 ? done != 0 : done == 0;
}

// ---- product ------------------------------------------------------------------------------------------------------------------------
// Node block rows.  GROUP lanes walk the blocks of one node: its diagonal block, the blocks of its upper neighbours (contiguous in the three
// CSR rows of the node: adjacent lanes read adjacent 24-byte runs) and the transposed blocks of its lower neighbours (found through the
// pattern's index).  A lane loads the three x values of a neighbour once for the nine entries of the block.
template <bool FUSE>
__global__ __launch_bounds__(BLOCK) void k_pcg_symv_blocks(int nNodes, const int* __restrict__ rowBase, const int* __restrict__ rowLen,
    const int* __restrict__ ja, const double* __restrict__ a, const int* __restrict__ lowPtr, const int* __restrict__ lowNode,
    const int* __restrict__ lowSlot, const int* __restrict__ lowLen, const double* __restrict__ x, const double* __restrict__ pOld,
    double* __restrict__ pOut, int first, double* __restrict__ y, double* __restrict__ partial, const PcgState* __restrict__ st, int gate)
{
    __shared__ double sm[BLOCK / 64];
    if (gated_out(st, gate)) return;
    const int lane = threadIdx.x & (GROUP - 1);
    const int v = blockIdx.x * NODES_PER_BLOCK + (threadIdx.x / GROUP);
    const bool mix = FUSE && !first;
    const double beta = mix ? st->beta : 0.0;
    auto load3 = [&](int node, double& p0, double& p1, double& p2) {
        const size_t o = 3 * (size_t)node;
        p0 = x[o], p1 = x[o + 1], p2 = x[o + 2];
        if (mix) {
            p0 += beta * pOld[o];
            p1 += beta * pOld[o + 1];
            p2 += beta * pOld[o + 2];
        }
    };
    double y0 = 0.0, y1 = 0.0, y2 = 0.0, own0 = 0.0, own1 = 0.0, own2 = 0.0;
    if (v < nNodes) {
        const int base = rowBase[v], len = rowLen[v], cnt = (len - 3) / 3;
        const int lo0 = lowPtr[v], nItems = 1 + cnt + (lowPtr[v + 1] - lo0);
        for (int it = lane; it < nItems; it += GROUP) {
            double p0, p1, p2;
            if (it == 0) {
                load3(v, p0, p1, p2);
                own0 = p0, own1 = p1, own2 = p2;
                const double d00 = a[base], d01 = a[base + 1], d02 = a[base + 2];
                const double d11 = a[base + len], d12 = a[base + len + 1], d22 = a[base + 2 * len - 1];
                y0 += d00 * p0 + d01 * p1 + d02 * p2;
                y1 += d01 * p0 + d11 * p1 + d12 * p2;
                y2 += d02 * p0 + d12 * p1 + d22 * p2;
            }
            else if (it <= cnt) {
                const int s0 = base + 3 * it, s1 = s0 + len - 1, s2 = s0 + 2 * len - 3;
                load3(ja[s0] / 3, p0, p1, p2);
                y0 += a[s0] * p0 + a[s0 + 1] * p1 + a[s0 + 2] * p2;
                y1 += a[s1] * p0 + a[s1 + 1] * p1 + a[s1 + 2] * p2;
                y2 += a[s2] * p0 + a[s2 + 1] * p1 + a[s2 + 2] * p2;
            }
            else {
                const int k = lo0 + it - 1 - cnt;
                const int l = lowLen[k], s0 = lowSlot[k], s1 = s0 + l - 1, s2 = s0 + 2 * l - 3;
                load3(lowNode[k], p0, p1, p2);
                y0 += a[s0] * p0 + a[s1] * p1 + a[s2] * p2;
                y1 += a[s0 + 1] * p0 + a[s1 + 1] * p1 + a[s2 + 1] * p2;
                y2 += a[s0 + 2] * p0 + a[s1 + 2] * p1 + a[s2 + 2] * p2;
            }
        }
    }
#pragma unroll
    for (int off = GROUP / 2; off > 0; off >>= 1) {
        y0 += __shfl_xor(y0, off, GROUP);
        y1 += __shfl_xor(y1, off, GROUP);
        y2 += __shfl_xor(y2, off, GROUP);
    }
    double dot = 0.0;
    if (lane == 0 && v < nNodes) {
        const size_t o = 3 * (size_t)v;
        y[o] = y0, y[o + 1] = y1, y[o + 2] = y2;
        if (FUSE) {
            pOut[o] = own0, pOut[o + 1] = own1, pOut[o + 2] = own2;
            dot = own0 * y0 + own1 * y1 + own2 * y2;
        }
    }
    if (FUSE) {
        const double r = block_sum<BLOCK>(dot, sm);
        if (threadIdx.x == 0) partial[blockIdx.x] = r;
    }
}

// Scalar rows (set_pattern_csr patterns): one thread per row, upper entries from its own row, lower entries through the index.
template <bool FUSE>
__global__ __launch_bounds__(BLOCK) void k_pcg_symv_rows(int nRows, const int* __restrict__ ia, const int* __restrict__ ja, const double* __restrict__ a,
    const int* __restrict__ lowPtr, const int* __restrict__ lowRow, const int* __restrict__ lowSlot, const double* __restrict__ x,
    const double* __restrict__ pOld, double* __restrict__ pOut, int first, double* __restrict__ y, double* __restrict__ partial,
    const PcgState* __restrict__ st, int gate)
{
    __shared__ double sm[BLOCK / 64];
    if (gated_out(st, gate)) return;
    const int r = blockIdx.x * BLOCK + threadIdx.x;
    const bool mix = FUSE && !first;
    const double beta = mix ? st->beta : 0.0;
    double dot = 0.0;
    if (r < nRows) {
        double acc = 0.0;
        for (int k = ia[r]; k < ia[r + 1]; ++k) {
            const int c = ja[k];
            acc += a[k] * (mix ? x[c] + beta * pOld[c] : x[c]);
        }
        for (int k = lowPtr[r]; k < lowPtr[r + 1]; ++k) {
            const int c = lowRow[k];
            acc += a[lowSlot[k]] * (mix ? x[c] + beta * pOld[c] : x[c]);
        }
        y[r] = acc;
        if (FUSE) {
            const double own = mix ? x[r] + beta * pOld[r] : x[r];
            pOut[r] = own;
            dot = own * acc;
        }
    }
    if (FUSE) {
        const double s = block_sum<BLOCK>(dot, sm);
        if (threadIdx.x == 0) partial[blockIdx.x] = s;
    }
}

// ---- block Jacobi -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_pcg_invert_blocks(int nNodes, const int* __restrict__ diagSlot, const double* __restrict__ a,
    double* __restrict__ dinv, int* __restrict__ flag)
{
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= nNodes) return;
    double d[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int s = diagSlot[(size_t)i * nNodes + v];
        d[i] = s >= 0 ? a[s] : 0.0;
    }
    // (00, 01, 02, 11, 12, 22); positive definite <=> the three leading minors are positive
    const double c00 = d[3] * d[5] - d[4] * d[4], c01 = d[2] * d[4] - d[1] * d[5], c02 = d[1] * d[4] - d[2] * d[3];
    const double m2 = d[0] * d[3] - d[1] * d[1];
    const double det = d[0] * c00 + d[1] * c01 + d[2] * c02;
    if (!(d[0] > 0.0) || !(m2 > 0.0) || !(det > 0.0)) {
        atomicOr(flag, 1);
        return;
    }
    const double inv[6] = { c00 / det, c01 / det, c02 / det, (d[0] * d[5] - d[2] * d[2]) / det, (d[1] * d[2] - d[0] * d[4]) / det, m2 / det };
#pragma unroll
    for (int i = 0; i < 6; ++i) dinv[(size_t)i * nNodes + v] = inv[i];
}

__device__ __forceinline__ void apply_dinv(const double* __restrict__ dinv, int nNodes, int v, double r0, double r1, double r2, double& z0, double& z1,
    double& z2)
{
    const double m00 = dinv[v], m01 = dinv[(size_t)nNodes + v], m02 = dinv[2 * (size_t)nNodes + v];
    const double m11 = dinv[3 * (size_t)nNodes + v], m12 = dinv[4 * (size_t)nNodes + v], m22 = dinv[5 * (size_t)nNodes + v];
    z0 = m00 * r0 + m01 * r1 + m02 * r2;
    z1 = m01 * r0 + m11 * r1 + m12 * r2;
    z2 = m02 * r0 + m12 * r1 + m22 * r2;
}

// ---- vector passes ------------------------------------------------------------------------------------------------------------------
// partial layout: [0, cap) p.Ap of the product, [cap, 2 cap) r.z, [2 cap, 3 cap) r.r
// start of a solve (restart = 0: x = 0, r = b) or of a restart from the current x (restart = 1: r = b - y with y = A x)
__global__ __launch_bounds__(BLOCK) void k_pcg_begin(int nNodes, int jacobi, int restart, const double* __restrict__ b, const double* __restrict__ yAx,
    const double* __restrict__ dinv, double* __restrict__ x, double* __restrict__ r, double* __restrict__ z, double* __restrict__ pRz,
    double* __restrict__ pRr)
{
    __shared__ double smA[BLOCK / 64], smB[BLOCK / 64];
    double rz = 0.0, rr = 0.0;
    for (int v = blockIdx.x * BLOCK + threadIdx.x; v < nNodes; v += gridDim.x * BLOCK) {
        const size_t o = 3 * (size_t)v;
        double r0 = b[o], r1 = b[o + 1], r2 = b[o + 2];
        if (restart) r0 -= yAx[o], r1 -= yAx[o + 1], r2 -= yAx[o + 2];
        else x[o] = x[o + 1] = x[o + 2] = 0.0;
        r[o] = r0, r[o + 1] = r1, r[o + 2] = r2;
        rr += r0 * r0 + r1 * r1 + r2 * r2;
        if (jacobi) {
            double z0, z1, z2;
            apply_dinv(dinv, nNodes, v, r0, r1, r2, z0, z1, z2);
            z[o] = z0, z[o + 1] = z1, z[o + 2] = z2;
            rz += r0 * z0 + r1 * z1 + r2 * z2;
        }
    }
    const double sRz = block_sum<BLOCK>(rz, smA), sRr = block_sum<BLOCK>(rr, smB);
    if (threadIdx.x == 0) pRz[blockIdx.x] = sRz, pRr[blockIdx.x] = sRr;
}
__device__ __forceinline__ double reduce_partials(const double* __restrict__ partial, int n, double* sm)
{
    double x = 0.0;
    for (int i = threadIdx.x; i < n; i += BLOCK) x += partial[i];
    return block_sum<BLOCK>(x, sm);
}
__global__ __launch_bounds__(BLOCK) void k_pcg_begin_state(int n, int jacobi, int restart, const double* __restrict__ pRz, const double* __restrict__ pRr,
    double relTol, int maxIter, PcgState* __restrict__ st)
{
    __shared__ double smA[BLOCK / 64], smB[BLOCK / 64];
    const double rz = reduce_partials(pRz, n, smA), rr = reduce_partials(pRr, n, smB);
    if (threadIdx.x) return;
    if (!restart) {
        st->bb = rr;
        st->tol2 = relTol * relTol * rr;
        st->iter = 0;
        st->maxIter = maxIter;
        st->trueRes2 = rr;
    }
    st->rr = rr;
    st->rz = jacobi ? rz : 0.0;
    st->pAp = st->alpha = st->beta = 0.0;
    st->done = rr <= st->tol2 ? PCG_CONVERGED : (st->iter >= st->maxIter ? PCG_MAXITER : PCG_RUNNING);
}

__global__ __launch_bounds__(BLOCK) void k_pcg_alpha(int n, const double* __restrict__ pAp, PcgState* __restrict__ st)
{
    __shared__ double sm[BLOCK / 64];
    if (st->done) return;
    const double s = reduce_partials(pAp, n, sm);
    if (threadIdx.x) return;
    st->pAp = s;
    if (!(s > 0.0)) st->done = PCG_BREAKDOWN; // (a NaN lands here too)
    else st->alpha = st->rz / s;
}

__global__ __launch_bounds__(BLOCK) void k_pcg_update(int nNodes, int jacobi, const double* __restrict__ p, const double* __restrict__ Ap,
    const double* __restrict__ dinv, double* __restrict__ x, double* __restrict__ r, double* __restrict__ z, double* __restrict__ pRz,
    double* __restrict__ pRr, const PcgState* __restrict__ st)
{
    __shared__ double smA[BLOCK / 64], smB[BLOCK / 64];
    if (st->done) return;
    const double alpha = st->alpha;
    double rz = 0.0, rr = 0.0;
    for (int v = blockIdx.x * BLOCK + threadIdx.x; v < nNodes; v += gridDim.x * BLOCK) {
        const size_t o = 3 * (size_t)v;
        x[o] += alpha * p[o], x[o + 1] += alpha * p[o + 1], x[o + 2] += alpha * p[o + 2];
        const double r0 = r[o] - alpha * Ap[o], r1 = r[o + 1] - alpha * Ap[o + 1], r2 = r[o + 2] - alpha * Ap[o + 2];
        r[o] = r0, r[o + 1] = r1, r[o + 2] = r2;
        rr += r0 * r0 + r1 * r1 + r2 * r2;
        if (jacobi) {
            double z0, z1, z2;
            apply_dinv(dinv, nNodes, v, r0, r1, r2, z0, z1, z2);
            z[o] = z0, z[o + 1] = z1, z[o + 2] = z2;
            rz += r0 * z0 + r1 * z1 + r2 * z2;
        }
    }
    const double sRz = block_sum<BLOCK>(rz, smA), sRr = block_sum<BLOCK>(rr, smB);
    if (threadIdx.x == 0) pRz[blockIdx.x] = sRz, pRr[blockIdx.x] = sRr;
}
__global__ __launch_bounds__(BLOCK) void k_pcg_update_state(int n, int jacobi, const double* __restrict__ pRz, const double* __restrict__ pRr,
    PcgState* __restrict__ st)
{
    __shared__ double smA[BLOCK / 64], smB[BLOCK / 64];
    if (st->done) return;
    const double rz = reduce_partials(pRz, n, smA), rr = reduce_partials(pRr, n, smB);
    if (threadIdx.x) return;
    st->rr = rr;
    st->iter += 1;
    if (jacobi) {
        st->beta = rz / st->rz;
        st->rz = rz;
    }
    if (rr <= st->tol2) st->done = PCG_CONVERGED;
    else if (st->iter >= st->maxIter) st->done = PCG_MAXITER;
}

// r.z for a z that another solver produced (lagged factor)
__global__ __launch_bounds__(BLOCK) void k_pcg_dot(int n, const double* __restrict__ u, const double* __restrict__ w, double* __restrict__ partial,
    const PcgState* __restrict__ st)
{
    __shared__ double sm[BLOCK / 64];
    if (st->done) return;
    double s = 0.0;
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) s += u[i] * w[i];
    const double t = block_sum<BLOCK>(s, sm);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}
__global__ __launch_bounds__(BLOCK) void k_pcg_rz_state(int n, int first, const double* __restrict__ pRz, PcgState* __restrict__ st)
{
    __shared__ double sm[BLOCK / 64];
    if (st->done) return;
    const double rz = reduce_partials(pRz, n, sm);
    if (threadIdx.x) return;
    if (!first) st->beta = rz / st->rz;
    st->rz = rz;
}

// |b - y|^2, once the iteration has ended
__global__ __launch_bounds__(BLOCK) void k_pcg_res(int n, const double* __restrict__ b, const double* __restrict__ y, double* __restrict__ partial,
    const PcgState* __restrict__ st)
{
    __shared__ double sm[BLOCK / 64];
    if (!st->done) return;
    double s = 0.0;
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        const double d = b[i] - y[i];
        s += d * d;
    }
    const double t = block_sum<BLOCK>(s, sm);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}
__global__ __launch_bounds__(BLOCK) void k_pcg_res_state(int n, const double* __restrict__ partial, PcgState* __restrict__ st)
{
    __shared__ double sm[BLOCK / 64];
    if (!st->done) return;
    const double s = reduce_partials(partial, n, sm);
    if (threadIdx.x == 0) st->trueRes2 = s;
}
__global__ void k_pcg_publish(const unsigned* __restrict__ src, unsigned* __restrict__ dst, int n)
{
    const int i = threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// ---- two-level preconditioner -------------------------------------------------------------------------------------------------------------------
// GROUP lanes share one aggregate (geometry, restriction) or one aggregate pair (Galerkin product): the lanes stride over the item's list, the sums are
// combined by the xor butterfly below -- a fixed order, the same bits on every run -- and lane 0 writes.
__device__ __forceinline__ double group_sum(double x)
{
#pragma unroll
    for (int off = GROUP / 2; off > 0; off >>= 1) x += __shfl_xor(x, off, GROUP);
    return x;
}
// out = M S(d) and out = S(d)^T M for row-major 3x3 M, S(d) w = d x w
__device__ __forceinline__ void times_S(const double* M, double dx, double dy, double dz, double* out)
{
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        out[3 * r + 0] = M[3 * r + 1] * dz - M[3 * r + 2] * dy;
        out[3 * r + 1] = M[3 * r + 2] * dx - M[3 * r + 0] * dz;
        out[3 * r + 2] = M[3 * r + 0] * dy - M[3 * r + 1] * dx;
    }
}
__device__ __forceinline__ void St_times(const double* M, double dx, double dy, double dz, double* out)
{
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        out[0 + c] = dz * M[3 + c] - dy * M[6 + c];
        out[3 + c] = dx * M[6 + c] - dz * M[0 + c];
        out[6 + c] = dy * M[0 + c] - dx * M[3 + c];
    }
}

__global__ __launch_bounds__(BLOCK) void k_pcg_coarse_geometry(int nAgg, int nNodes, const int* __restrict__ aggPtr, const int* __restrict__ aggNodes,
    const double* __restrict__ x, const int* __restrict__ dbcType, double* __restrict__ geo, int* __restrict__ aggFlags)
{
    const int lane = threadIdx.x & (GROUP - 1);
    const int I = blockIdx.x * NODES_PER_BLOCK + (threadIdx.x / GROUP);
    const int b = I < nAgg ? aggPtr[I] : 0, e = I < nAgg ? aggPtr[I + 1] : 0;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, cnt = 0.0;
    for (int k = b + lane; k < e; k += GROUP) {
        const int v = aggNodes[k];
        if (dbcType[v] == 0) {
            const size_t o = 3 * (size_t)v;
            s0 += x[o], s1 += x[o + 1], s2 += x[o + 2];
            cnt += 1.0;
        }
    }
    s0 = group_sum(s0), s1 = group_sum(s1), s2 = group_sum(s2), cnt = group_sum(cnt);
    if (I >= nAgg) return;
    const bool rot = cnt >= 4.0;
    const double inv = cnt > 0.0 ? 1.0 / cnt : 0.0;
    const double c0 = s0 * inv, c1 = s1 * inv, c2 = s2 * inv;
    for (int k = b + lane; k < e; k += GROUP) {
        const int v = aggNodes[k];
        const bool free_ = dbcType[v] == 0;
        const size_t o = 3 * (size_t)v;
        const bool arm = rot && free_;
        geo[v] = arm ? x[o] - c0 : 0.0;
        geo[(size_t)nNodes + v] = arm ? x[o + 1] - c1 : 0.0;
        geo[2 * (size_t)nNodes + v] = arm ? x[o + 2] - c2 : 0.0;
        geo[3 * (size_t)nNodes + v] = free_ ? 1.0 : 0.0;
    }
    if (lane == 0) aggFlags[I] = (cnt >= 1.0 ? 1 : 0) | (rot ? 2 : 0);
}

// One lane group per aggregate pair (I <= J).  For an entry (i in I, j in J) with fine block B the pair receives P_i^T B P_j =
// [ B, B S_j ; S_i^T B, S_i^T B S_j ]; an off-diagonal fine block inside one aggregate stands for its mirror image too (M + M^T).
__global__ __launch_bounds__(BLOCK) void k_pcg_galerkin(int nPairs, int nNodes, const int* __restrict__ pairIJ, const int* __restrict__ pairPtr,
    const int* __restrict__ pairSlot, const int4* __restrict__ ent, const int* __restrict__ rowLen, const int* __restrict__ cRowLen,
    const double* __restrict__ geo, const int* __restrict__ aggFlags, const double* __restrict__ a, double* __restrict__ ca)
{
    const int lane = threadIdx.x & (GROUP - 1);
    const int p = blockIdx.x * NODES_PER_BLOCK + (threadIdx.x / GROUP);
    const bool live = p < nPairs;
    const int I = live ? pairIJ[2 * p] : 0, J = live ? pairIJ[2 * p + 1] : 0;
    const int b = live ? pairPtr[p] : 0, e = live ? pairPtr[p + 1] : 0;
    double TT[9], TR[9], RT[9], RR[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) TT[q] = TR[q] = RT[q] = RR[q] = 0.0;
    for (int k = b + lane; k < e; k += GROUP) {
        const int4 en = ent[k]; // slot, row node u, column node w, transposed
        const int u = en.y, w = en.z;
        if (geo[3 * (size_t)nNodes + u] * geo[3 * (size_t)nNodes + w] == 0.0) continue; // a fixed node has no entries in P
        const int len = rowLen[u], s0 = en.x;
        double B[9];
        if (u == w) {
            B[0] = a[s0], B[1] = B[3] = a[s0 + 1], B[2] = B[6] = a[s0 + 2];
            B[4] = a[s0 + len], B[5] = B[7] = a[s0 + len + 1], B[8] = a[s0 + 2 * len - 1];
        }
        else {
            const int s1 = s0 + len - 1, s2 = s0 + 2 * len - 3;
            if (en.w) {
                B[0] = a[s0], B[3] = a[s0 + 1], B[6] = a[s0 + 2];
                B[1] = a[s1], B[4] = a[s1 + 1], B[7] = a[s1 + 2];
                B[2] = a[s2], B[5] = a[s2 + 1], B[8] = a[s2 + 2];
            }
            else {
                B[0] = a[s0], B[1] = a[s0 + 1], B[2] = a[s0 + 2];
                B[3] = a[s1], B[4] = a[s1 + 1], B[5] = a[s1 + 2];
                B[6] = a[s2], B[7] = a[s2 + 1], B[8] = a[s2 + 2];
            }
        }
        const int i = en.w ? w : u, j = en.w ? u : w;
        const double ix = geo[i], iy = geo[(size_t)nNodes + i], iz = geo[2 * (size_t)nNodes + i];
        const double jx = geo[j], jy = geo[(size_t)nNodes + j], jz = geo[2 * (size_t)nNodes + j];
        double tr[9], rt[9], rr[9];
        times_S(B, jx, jy, jz, tr);
        St_times(B, ix, iy, iz, rt);
        St_times(tr, ix, iy, iz, rr);
        if (I == J && u != w) {
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    TT[3 * r + c] += B[3 * r + c] + B[3 * c + r];
                    TR[3 * r + c] += tr[3 * r + c] + rt[3 * c + r];
                    RR[3 * r + c] += rr[3 * r + c] + rr[3 * c + r];
                }
        }
        else {
#pragma unroll
            for (int q = 0; q < 9; ++q) TT[q] += B[q], TR[q] += tr[q], RT[q] += rt[q], RR[q] += rr[q];
        }
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) TT[q] = group_sum(TT[q]), TR[q] = group_sum(TR[q]), RT[q] = group_sum(RT[q]), RR[q] = group_sum(RR[q]);
    if (!live || lane) return;
    const int lt = cRowLen[2 * I], lr = cRowLen[2 * I + 1];
    const int sTT = pairSlot[4 * p], sTR = pairSlot[4 * p + 1], sRT = pairSlot[4 * p + 2], sRR = pairSlot[4 * p + 3];
    auto full = [&](const double* M, int s, int len) {
#pragma unroll
        for (int c = 0; c < 3; ++c) ca[s + c] = M[c], ca[s + len - 1 + c] = M[3 + c], ca[s + 2 * len - 3 + c] = M[6 + c];
    };
    auto diag = [&](const double* M, int s, int len, bool identity) {
        ca[s] = identity ? 1.0 : M[0], ca[s + 1] = identity ? 0.0 : M[1], ca[s + 2] = identity ? 0.0 : M[2];
        ca[s + len] = identity ? 1.0 : M[4], ca[s + len + 1] = identity ? 0.0 : M[5], ca[s + 2 * len - 1] = identity ? 1.0 : M[8];
    };
    if (I == J) {
        const int f = aggFlags[I];
        diag(TT, sTT, lt, !(f & 1));
        full(TR, sTR, lt);
        diag(RR, sRR, lr, !(f & 2));
    }
    else {
        full(TT, sTT, lt);
        full(TR, sTR, lt);
        full(RT, sRT, lr);
        full(RR, sRR, lr);
    }
}

__global__ __launch_bounds__(BLOCK) void k_pcg_restrict(int nAgg, int nNodes, const int* __restrict__ aggPtr, const int* __restrict__ aggNodes,
    const double* __restrict__ geo, const double* __restrict__ r, double* __restrict__ rc, const PcgState* __restrict__ st, int gate)
{
    if (gated_out(st, gate)) return;
    const int lane = threadIdx.x & (GROUP - 1);
    const int I = blockIdx.x * NODES_PER_BLOCK + (threadIdx.x / GROUP);
    const int b = I < nAgg ? aggPtr[I] : 0, e = I < nAgg ? aggPtr[I + 1] : 0;
    double t0 = 0.0, t1 = 0.0, t2 = 0.0, q0 = 0.0, q1 = 0.0, q2 = 0.0;
    for (int k = b + lane; k < e; k += GROUP) {
        const int v = aggNodes[k];
        const size_t o = 3 * (size_t)v;
        const double w = geo[3 * (size_t)nNodes + v];
        const double dx = geo[v], dy = geo[(size_t)nNodes + v], dz = geo[2 * (size_t)nNodes + v]; // (zero for a fixed node)
        const double r0 = r[o], r1 = r[o + 1], r2 = r[o + 2];
        t0 += w * r0, t1 += w * r1, t2 += w * r2;
        q0 += r1 * dz - r2 * dy, q1 += r2 * dx - r0 * dz, q2 += r0 * dy - r1 * dx; // S(d)^T r = r x d
    }
    t0 = group_sum(t0), t1 = group_sum(t1), t2 = group_sum(t2), q0 = group_sum(q0), q1 = group_sum(q1), q2 = group_sum(q2);
    if (I < nAgg && lane == 0) {
        double* o = rc + 6 * (size_t)I;
        o[0] = t0, o[1] = t1, o[2] = t2, o[3] = q0, o[4] = q1, o[5] = q2;
    }
}

__global__ __launch_bounds__(BLOCK) void k_pcg_prolong(int nNodes, const int* __restrict__ aggOf, const double* __restrict__ geo, const double* __restrict__ dinv,
    const double* __restrict__ r, const double* __restrict__ xc, double* __restrict__ z, double* __restrict__ pRz, const PcgState* __restrict__ st, int gate)
{
    __shared__ double sm[BLOCK / 64];
    if (gated_out(st, gate)) return;
    double rz = 0.0;
    for (int v = blockIdx.x * BLOCK + threadIdx.x; v < nNodes; v += gridDim.x * BLOCK) {
        const size_t o = 3 * (size_t)v;
        const double r0 = r[o], r1 = r[o + 1], r2 = r[o + 2];
        double z0, z1, z2;
        apply_dinv(dinv, nNodes, v, r0, r1, r2, z0, z1, z2);
        const double* c = xc + 6 * (size_t)aggOf[v];
        const double w = geo[3 * (size_t)nNodes + v];
        const double dx = geo[v], dy = geo[(size_t)nNodes + v], dz = geo[2 * (size_t)nNodes + v];
        z0 += w * c[0] + (dy * c[5] - dz * c[4]); // S(d) w = d x w
        z1 += w * c[1] + (dz * c[3] - dx * c[5]);
        z2 += w * c[2] + (dx * c[4] - dy * c[3]);
        z[o] = z0, z[o + 1] = z1, z[o + 2] = z2;
        rz += r0 * z0 + r1 * z1 + r2 * z2;
    }
    const double s = block_sum<BLOCK>(rz, sm);
    if (threadIdx.x == 0) pRz[blockIdx.x] = s;
}

inline int vec_grid(long long n) { return (int)std::max<long long>(1, std::min<long long>(MAX_VEC_BLOCKS, (n + BLOCK - 1) / BLOCK)); }
} // namespace

// ---- host ---------------------------------------------------------------------------------------------------------------------------
void PcgPattern::build(int nRows_, const std::vector<int>& ia, const std::vector<int>& ja, const std::vector<int>& rowBase, const std::vector<int>& rowLen,
    hipStream_t s)
{
    nRows = nRows_;
    nNodes = nRows / 3;
    nnz = ia[nRows];
    blocks = (int)rowBase.size() == nNodes && nNodes > 0;
    std::vector<int> ptr, node, slot, len, dslot(6 * (size_t)nNodes, -1);
    if (blocks) {
        // one counting pass and one fill pass over the node blocks, like the transpose of the rocSOLVER back end but a ninth of its size
        ptr.assign(nNodes + 1, 0);
        for (int u = 0; u < nNodes; ++u)
            for (int k = rowBase[u] + 3; k < rowBase[u] + rowLen[u]; k += 3) ptr[ja[k] / 3 + 1]++;
        for (int v = 0; v < nNodes; ++v) ptr[v + 1] += ptr[v];
        node.resize(ptr[nNodes]);
        slot.resize(ptr[nNodes]);
        len.resize(ptr[nNodes]);
        std::vector<int> pos(ptr.begin(), ptr.end() - 1);
        for (int u = 0; u < nNodes; ++u)
            for (int k = rowBase[u] + 3; k < rowBase[u] + rowLen[u]; k += 3) {
                const int q = pos[ja[k] / 3]++;
                node[q] = u;
                slot[q] = k;
                len[q] = rowLen[u];
            }
        for (int v = 0; v < nNodes; ++v) {
            const int b = rowBase[v], l = rowLen[v];
            const int d[6] = { b, b + 1, b + 2, b + l, b + l + 1, b + 2 * l - 1 };
            for (int i = 0; i < 6; ++i) dslot[(size_t)i * nNodes + v] = d[i];
        }
    }
    else {
        ptr.assign(nRows + 1, 0);
        for (int r = 0; r < nRows; ++r)
            for (int k = ia[r] + 1; k < ia[r + 1]; ++k) ptr[ja[k] + 1]++;
        for (int r = 0; r < nRows; ++r) ptr[r + 1] += ptr[r];
        node.resize(ptr[nRows]);
        slot.resize(ptr[nRows]);
        std::vector<int> pos(ptr.begin(), ptr.end() - 1);
        for (int r = 0; r < nRows; ++r)
            for (int k = ia[r] + 1; k < ia[r + 1]; ++k) {
                const int q = pos[ja[k]]++;
                node[q] = r;
                slot[q] = k;
            }
        static const int dr[6] = { 0, 0, 0, 1, 1, 2 }, dc[6] = { 0, 1, 2, 1, 2, 2 };
        for (int v = 0; v < nNodes; ++v)
            for (int i = 0; i < 6; ++i) {
                const int r = 3 * v + dr[i], c = 3 * v + dc[i];
                const int* b = ja.data() + ia[r];
                const int* e = ja.data() + ia[r + 1];
                const int* it = std::lower_bound(b, e, c);
                if (it != e && *it == c) dslot[(size_t)i * nNodes + v] = int(it - ja.data());
            }
    }
    if (node.empty()) node.push_back(0), slot.push_back(0); // (a diagonal matrix: keep the pointers valid)
    if (len.empty()) len.push_back(0);
    lowPtr.uploadGrow(ptr, s);
    lowNode.uploadGrow(node, s);
    lowSlot.uploadGrow(slot, s);
    lowLen.uploadGrow(len, s);
    diagSlot.uploadGrow(dslot, s);
    dinv.ensure(6 * (size_t)nNodes);
    HIP_CHECK(hipStreamSynchronize(s)); // the host vectors go out of scope
}

int pcg_symv_grid(const PcgPattern& P) { return P.blocks ? (P.nNodes + NODES_PER_BLOCK - 1) / NODES_PER_BLOCK : (P.nRows + BLOCK - 1) / BLOCK; }

void PcgWork::ensure(int nRows)
{
    const size_t n = (size_t)nRows;
    r.ensure(n), z.ensure(n), p0.ensure(n), p1.ensure(n), Ap.ensure(n);
    // the product's grid is at most nRows / 3 / NODES_PER_BLOCK + 1 (blocks) or nRows / BLOCK + 1 (rows)
    const int cap = std::max(MAX_VEC_BLOCKS, nRows / 3 / NODES_PER_BLOCK + 2);
    if (cap > nPartial || !partial.p) {
        partial.alloc(3 * (size_t)cap);
        nPartial = cap;
    }
    if (!state.p) state.alloc(1);
    if (!flag.p) flag.alloc(1);
    if (!hState.p) hState.alloc(1);
}

void launch_pcg_symv(const PcgPattern& P, const int* ia, const int* ja, const int* rowBase, const int* rowLen, const double* a, const double* x,
    const double* pOld, double* pOut, int first, double* y, double* partial, const PcgState* st, int gate, hipStream_t s)
{
    const bool fuse = pOut != nullptr;
    const dim3 grid(pcg_symv_grid(P)), block(BLOCK);
    if (P.blocks) {
        if (fuse)
            hipLaunchKernelGGL(k_pcg_symv_blocks<true>, grid, block, 0, s, P.nNodes, rowBase, rowLen, ja, a, P.lowPtr.p, P.lowNode.p, P.lowSlot.p, P.lowLen.p, x,
                pOld, pOut, first, y, partial, st, gate);
        else
            hipLaunchKernelGGL(k_pcg_symv_blocks<false>, grid, block, 0, s, P.nNodes, rowBase, rowLen, ja, a, P.lowPtr.p, P.lowNode.p, P.lowSlot.p, P.lowLen.p, x,
                pOld, pOut, first, y, partial, st, gate);
    }
    else {
        if (fuse)
            hipLaunchKernelGGL(k_pcg_symv_rows<true>, grid, block, 0, s, P.nRows, ia, ja, a, P.lowPtr.p, P.lowNode.p, P.lowSlot.p, x, pOld, pOut, first, y, partial,
                st, gate);
        else
            hipLaunchKernelGGL(k_pcg_symv_rows<false>, grid, block, 0, s, P.nRows, ia, ja, a, P.lowPtr.p, P.lowNode.p, P.lowSlot.p, x, pOld, pOut, first, y, partial,
                st, gate);
    }
}

void launch_pcg_invert_blocks(PcgPattern& P, const double* a, int* flag, hipStream_t s)
{
    hipLaunchKernelGGL(k_pcg_invert_blocks, dim3((P.nNodes + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, P.nNodes, P.diagSlot.p, a, P.dinv.p, flag);
}

void launch_pcg_begin(const PcgPattern& P, bool jacobi, bool restart, const double* b, const double* yAx, double* x, PcgWork& W, double relTol, int maxIter,
    hipStream_t s)
{
    const int g = vec_grid(P.nNodes);
    double* pRz = W.partial.p + W.nPartial;
    double* pRr = W.partial.p + 2 * (size_t)W.nPartial;
    hipLaunchKernelGGL(k_pcg_begin, dim3(g), dim3(BLOCK), 0, s, P.nNodes, (int)jacobi, (int)restart, b, yAx, P.dinv.p, x, W.r.p, W.z.p, pRz, pRr);
    hipLaunchKernelGGL(k_pcg_begin_state, dim3(1), dim3(BLOCK), 0, s, g, (int)jacobi, (int)restart, pRz, pRr, relTol, maxIter, W.state.p);
}

void launch_pcg_rz(int n, const double* r, const double* z, PcgWork& W, int first, hipStream_t s)
{
    const int g = vec_grid(n);
    double* pRz = W.partial.p + W.nPartial;
    hipLaunchKernelGGL(k_pcg_dot, dim3(g), dim3(BLOCK), 0, s, n, r, z, pRz, W.state.p);
    hipLaunchKernelGGL(k_pcg_rz_state, dim3(1), dim3(BLOCK), 0, s, g, first, pRz, W.state.p);
}

void launch_pcg_alpha(PcgWork& W, int nPartialAp, hipStream_t s)
{
    hipLaunchKernelGGL(k_pcg_alpha, dim3(1), dim3(BLOCK), 0, s, nPartialAp, W.partial.p, W.state.p);
}

void launch_pcg_update(const PcgPattern& P, bool jacobi, const double* p, const double* Ap, double* x, PcgWork& W, hipStream_t s)
{
    const int g = vec_grid(P.nNodes);
    double* pRz = W.partial.p + W.nPartial;
    double* pRr = W.partial.p + 2 * (size_t)W.nPartial;
    hipLaunchKernelGGL(k_pcg_update, dim3(g), dim3(BLOCK), 0, s, P.nNodes, (int)jacobi, p, Ap, P.dinv.p, x, W.r.p, W.z.p, pRz, pRr, W.state.p);
    hipLaunchKernelGGL(k_pcg_update_state, dim3(1), dim3(BLOCK), 0, s, g, (int)jacobi, pRz, pRr, W.state.p);
}

void PcgCoarseDev::upload(const PcgCoarse& C, hipStream_t s)
{
    nNodes = C.nNodes, nAgg = C.nAgg, nPairs = (int)C.pairI.size();
    std::vector<int> ij(2 * (size_t)nPairs), e4(4 * C.entSlot.size());
    for (int p = 0; p < nPairs; ++p) ij[2 * p] = C.pairI[p], ij[2 * p + 1] = C.pairJ[p];
    for (size_t k = 0; k < C.entSlot.size(); ++k) e4[4 * k] = C.entSlot[k], e4[4 * k + 1] = C.entRow[k], e4[4 * k + 2] = C.entCol[k], e4[4 * k + 3] = C.entTrans[k];
    aggOf.uploadGrow(C.aggOf, s), aggPtr.uploadGrow(C.aggPtr, s), aggNodes.uploadGrow(C.aggNodes, s);
    pairIJ.uploadGrow(ij, s), pairPtr.uploadGrow(C.pairPtr, s), pairSlot.uploadGrow(C.pairSlot, s), cRowLen.uploadGrow(C.cRowLen, s);
    ent.uploadGrow(e4, s);
    geo.ensure(4 * (size_t)nNodes), aggFlags.ensure(nAgg), rc.ensure(6 * (size_t)nAgg), xc.ensure(6 * (size_t)nAgg);
    HIP_CHECK(hipStreamSynchronize(s)); // the host vectors go out of scope
}

void launch_pcg_coarse_geometry(PcgCoarseDev& C, const double* x, const int* dbcType, hipStream_t s)
{
    hipLaunchKernelGGL(k_pcg_coarse_geometry, dim3((C.nAgg + NODES_PER_BLOCK - 1) / NODES_PER_BLOCK), dim3(BLOCK), 0, s, C.nAgg, C.nNodes, C.aggPtr.p, C.aggNodes.p, x,
        dbcType, C.geo.p, C.aggFlags.p);
}

void launch_pcg_galerkin(const PcgCoarseDev& C, const int* rowLen, const double* a, double* ca, hipStream_t s)
{
    hipLaunchKernelGGL(k_pcg_galerkin, dim3((C.nPairs + NODES_PER_BLOCK - 1) / NODES_PER_BLOCK), dim3(BLOCK), 0, s, C.nPairs, C.nNodes, C.pairIJ.p, C.pairPtr.p,
        C.pairSlot.p, (const int4*)C.ent.p, rowLen, C.cRowLen.p, C.geo.p, C.aggFlags.p, a, ca);
}

void launch_pcg_restrict(const PcgCoarseDev& C, const double* r, double* rc, const PcgState* st, int gate, hipStream_t s)
{
    hipLaunchKernelGGL(k_pcg_restrict, dim3((C.nAgg + NODES_PER_BLOCK - 1) / NODES_PER_BLOCK), dim3(BLOCK), 0, s, C.nAgg, C.nNodes, C.aggPtr.p, C.aggNodes.p, C.geo.p, r,
        rc, st, gate);
}

void launch_pcg_prolong(const PcgPattern& P, const PcgCoarseDev& C, const double* xc, PcgWork& W, int first, int gate, hipStream_t s)
{
    const int g = vec_grid(P.nNodes);
    double* pRz = W.partial.p + W.nPartial;
    hipLaunchKernelGGL(k_pcg_prolong, dim3(g), dim3(BLOCK), 0, s, P.nNodes, C.aggOf.p, C.geo.p, P.dinv.p, W.r.p, xc, W.z.p, pRz, W.state.p, gate);
    hipLaunchKernelGGL(k_pcg_rz_state, dim3(1), dim3(BLOCK), 0, s, g, first, pRz, W.state.p);
}

void launch_pcg_residual(int n, const double* b, const double* y, PcgWork& W, hipStream_t s)
{
    const int g = vec_grid(n);
    hipLaunchKernelGGL(k_pcg_res, dim3(g), dim3(BLOCK), 0, s, n, b, y, W.partial.p, W.state.p);
    hipLaunchKernelGGL(k_pcg_res_state, dim3(1), dim3(BLOCK), 0, s, g, W.partial.p, W.state.p);
}

void launch_pcg_publish(PcgWork& W, hipStream_t s)
{
    hipLaunchKernelGGL(k_pcg_publish, dim3(1), dim3(64), 0, s, (const unsigned*)W.state.p, (unsigned*)W.hState.dev, PCG_STATE_WORDS);
}

} // namespace ipcgpu
