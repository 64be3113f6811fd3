// Elastic rods: kernels (see rod_kernels.h for the energies).
//   k_rod_energy               one lane per segment or bending triple, one partial sum per block, reduced in a fixed order
//   k_rod_stretch<withHessian> one lane per segment: 6-vector + three upper 3 x 3 blocks (the clamp is closed form: no eigen-iteration)
//   k_rod_bend<withHessian>    one lane per triple: 9-vector + six upper 3 x 3 blocks (Gauss-Newton, rank <= 3: no eigen-iteration)
// All of them are small (no iterate to carry) and run 256 wide; register figures: DESIGN.md.
#include "rod_kernels.h"
#include "csr_scatter_device.h"
#include "stencil_hessian_device.h"
#include <algorithm>

namespace ipcgpu {

namespace {

using namespace scatter; // projected_dbc, ld3, CsrSink, add_diag, add_off, store_block_sum, nblk, launch_reduce_partials (csr_scatter_device.h)

constexpr int ROD_BLOCK = 256;

__device__ __forceinline__ double stretch_energy(const RodView& v, int s)
{
    const int2 n = v.seg[s];
    double xa[3], xb[3];
    ld3(v.x, n.x, xa);
    ld3(v.x, n.y, xb);
    const double e[3] = { xb[0] - xa[0], xb[1] - xa[1], xb[2] - xa[2] };
    const double dl = sqrt(sh::dot(e, e)) - v.segConst[s];
    return 0.5 * v.segConst[(size_t)v.nSeg + s] * dl * dl;
}

// the edges of a triple and d = |e0||e1| + e0 . e1; returns |kb|^2 = 4 (|e0||e1| - e0 . e1) / d, +infinity where d <= 0
struct Bend {
    double e0[3], e1[3];
    double s0, s1, d;
};
__device__ __forceinline__ double bend_state(const RodView& v, int i, int* node, Bend& b)
{
    const size_t n = (size_t)v.nBend;
    node[0] = v.bend[i];
    node[1] = v.bend[n + i];
    node[2] = v.bend[2 * n + i];
    double xa[3], xb[3], xc[3];
    ld3(v.x, node[0], xa);
    ld3(v.x, node[1], xb);
    ld3(v.x, node[2], xc);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        b.e0[k] = xb[k] - xa[k];
        b.e1[k] = xc[k] - xb[k];
    }
    b.s0 = sh::dot(b.e0, b.e0);
    b.s1 = sh::dot(b.e1, b.e1);
    const double p = sqrt(b.s0 * b.s1), q = sh::dot(b.e0, b.e1);
    b.d = p + q;
    if (!(b.d > 0.0)) return __builtin_inf();
    return 4.0 * fmax(p - q, 0.0) / b.d; // (Cauchy-Schwarz: p >= q; the clamp only removes a rounding of a straight node)
}
__device__ __forceinline__ double bend_energy(const RodView& v, int i)
{
    int node[3];
    Bend b;
    const double k2 = bend_state(v, i, node, b);
    return v.bendConst[i] * k2;
}

__global__ __launch_bounds__(ROD_BLOCK) void k_rod_energy(RodView v, double coef, double* __restrict__ partial)
{
    const int gid = blockIdx.x * ROD_BLOCK + threadIdx.x;
    double e = 0.0;
    if (gid < v.nSeg) e = coef * stretch_energy(v, gid);
    else if (gid - v.nSeg < v.nBend) e = coef * bend_energy(v, gid - v.nSeg);
    store_block_sum<ROD_BLOCK>(e, partial);
}
__global__ __launch_bounds__(ROD_BLOCK) void k_rod_energy_per_elem(RodView v, double* __restrict__ perSeg, double* __restrict__ perBend)
{
    const int gid = blockIdx.x * ROD_BLOCK + threadIdx.x;
    if (gid < v.nSeg) {
        if (perSeg) perSeg[gid] = stretch_energy(v, gid);
    }
    else if (gid - v.nSeg < v.nBend) {
        if (perBend) perBend[gid - v.nSeg] = bend_energy(v, gid - v.nSeg);
    }
}

template <bool HESS>
__global__ __launch_bounds__(ROD_BLOCK) void k_rod_stretch(RodView v, double coef, int projectDBC, double* __restrict__ grad, double* __restrict__ a,
    int* __restrict__ err)
{
    const int s = blockIdx.x * ROD_BLOCK + threadIdx.x;
    if (s >= v.nSeg) return;
    const int2 n = v.seg[s];
    const bool pa = projected_dbc(v.dbc[n.x], projectDBC), pb = projected_dbc(v.dbc[n.y], projectDBC);
    double xa[3], xb[3];
    ld3(v.x, n.x, xa);
    ld3(v.x, n.y, xb);
    const double e[3] = { xb[0] - xa[0], xb[1] - xa[1], xb[2] - xa[2] };
    const double L = v.segConst[s], ks = coef * v.segConst[(size_t)v.nSeg + s];
    const double l = sqrt(sh::dot(e, e));
    if (!(l > 0.0)) return; // collapsed to a point: no direction, hence no force and no block
    const double il = 1.0 / l;
    const double t[3] = { e[0] * il, e[1] * il, e[2] * il };
    if (grad) {
        const double f = ks * (l - L);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (!pa) atomicAdd(&grad[3 * (size_t)n.x + i], -f * t[i]);
            if (!pb) atomicAdd(&grad[3 * (size_t)n.y + i], f * t[i]);
        }
    }
    if constexpr (HESS) {
        // B = k_s [(1 - c) t t^T + c I], c = max(0, 1 - L / l): the eigenvalue clamp in closed form
        const double c = fmax(0.0, 1.0 - L * il);
        const double kt = ks * (1.0 - c), kc = ks * c;
        double B[9], Bm[9];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                B[r + 3 * q] = kt * t[r] * t[q] + (r == q ? kc : 0.0);
                Bm[r + 3 * q] = -B[r + 3 * q];
            }
        const CsrSink k{ v.rowBase, v.rowLen, v.ja, a, err };
        if (!pa) add_diag(k, n.x, B);
        if (!pb) add_diag(k, n.y, B);
        if (!pa && !pb) add_off(k, n.x, n.y, Bm);
    }
}

template <bool HESS>
__global__ __launch_bounds__(ROD_BLOCK) void k_rod_bend(RodView v, double coef, int projectDBC, double* __restrict__ grad, double* __restrict__ a,
    int* __restrict__ err)
{
    const int i = blockIdx.x * ROD_BLOCK + threadIdx.x;
    if (i >= v.nBend) return;
    int node[3];
    Bend b;
    bend_state(v, i, node, b);
    if (!(b.d > 0.0)) return; // folded flat: the energy is +infinity there, no derivative exists
    bool proj[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) proj[k] = projected_dbc(v.dbc[node[k]], projectDBC);
    const double id = 1.0 / b.d, ck2 = 2.0 * coef * v.bendConst[i];
    double kb[3];
    sh::cross(b.e0, b.e1, kb);
#pragma unroll
    for (int k = 0; k < 3; ++k) kb[k] *= 2.0 * id;
    // w0 = |e1| t0 + e1, w1 = |e0| t1 + e0 (the derivatives of d)
    const double r10 = sqrt(b.s1 / b.s0), r01 = sqrt(b.s0 / b.s1);
    double w0[3], w1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        w0[k] = r10 * b.e0[k] + b.e1[k];
        w1[k] = r01 * b.e1[k] + b.e0[k];
    }
    // J[n][m][c] = d kb_m / d x_n,c:  D0 = (-2 [e1]_x - kb w0^T) / d,  D1 = (2 [e0]_x - kb w1^T) / d;  a: -D0, b: D0 - D1, c: D1
    double J[3][3][3];
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            // [u]_x[m][c] = -eps(m, c, k) u_k: the entry is +-u_k for the k that differs from both m and c
            double x0 = 0.0, x1 = 0.0;
            if (m != c) {
                const int k = 3 - m - c;
                const double sgn = ((c - m + 3) % 3 == 1) ? -1.0 : 1.0; // [u]_x[0][1] = -u_2, [u]_x[1][2] = -u_0, [u]_x[2][0] = -u_1
                x0 = sgn * b.e0[k];
                x1 = sgn * b.e1[k];
            }
            const double D0 = (-2.0 * x1 - kb[m] * w0[c]) * id, D1 = (2.0 * x0 - kb[m] * w1[c]) * id;
            J[0][m][c] = -D0;
            J[1][m][c] = D0 - D1;
            J[2][m][c] = D1;
        }
    if (grad) {
#pragma unroll
        for (int n = 0; n < 3; ++n)
            if (!proj[n]) {
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    atomicAdd(&grad[3 * (size_t)node[n] + c], ck2 * (J[n][0][c] * kb[0] + J[n][1][c] * kb[1] + J[n][2][c] * kb[2]));
            }
    }
    if constexpr (HESS) {
        const CsrSink sink{ v.rowBase, v.rowLen, v.ja, a, err };
#pragma unroll
        for (int l = 0; l < 3; ++l)
#pragma unroll
            for (int k = 0; k <= l; ++k) {
                if (proj[k] || proj[l]) continue;
                double A[9];
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) A[r + 3 * c] = ck2 * (J[k][0][r] * J[l][0][c] + J[k][1][r] * J[l][1][c] + J[k][2][r] * J[l][2][c]);
                if (k == l) add_diag(sink, node[k], A);
                else add_off(sink, node[k], node[l], A);
            }
    }
}

} // namespace

int rod_energy_blocks(const RodView& v) { return std::max(1, nblk(v.nSeg + v.nBend, ROD_BLOCK)); }

void launch_rod_energy(const RodView& v, double coef, double* partial, double* out, bool accumulate, hipStream_t s)
{
    const int nb = rod_energy_blocks(v);
    hipLaunchKernelGGL(k_rod_energy, dim3(nb), dim3(ROD_BLOCK), 0, s, v, coef, partial);
    launch_reduce_partials(partial, nb, 1.0, accumulate, out, s);
}
void launch_rod_energy_per_elem(const RodView& v, double* perSeg, double* perBend, hipStream_t s)
{
    if (v.nSeg + v.nBend <= 0) return;
    hipLaunchKernelGGL(k_rod_energy_per_elem, dim3(nblk(v.nSeg + v.nBend, ROD_BLOCK)), dim3(ROD_BLOCK), 0, s, v, perSeg, perBend);
}
void launch_rod_assemble(const RodView& v, double coef, int projectDBC, double* grad, double* a, int* err, hipStream_t s)
{
    if (v.nSeg > 0) {
        if (a) hipLaunchKernelGGL(k_rod_stretch<true>, dim3(nblk(v.nSeg, ROD_BLOCK)), dim3(ROD_BLOCK), 0, s, v, coef, projectDBC, grad, a, err);
        else hipLaunchKernelGGL(k_rod_stretch<false>, dim3(nblk(v.nSeg, ROD_BLOCK)), dim3(ROD_BLOCK), 0, s, v, coef, projectDBC, grad, a, err);
    }
    if (v.nBend > 0) {
        if (a) hipLaunchKernelGGL(k_rod_bend<true>, dim3(nblk(v.nBend, ROD_BLOCK)), dim3(ROD_BLOCK), 0, s, v, coef, projectDBC, grad, a, err);
        else hipLaunchKernelGGL(k_rod_bend<false>, dim3(nblk(v.nBend, ROD_BLOCK)), dim3(ROD_BLOCK), 0, s, v, coef, projectDBC, grad, a, err);
    }
}

} // namespace ipcgpu
