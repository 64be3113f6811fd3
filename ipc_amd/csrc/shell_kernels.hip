// Elastic shells: kernels (see shell_kernels.h for the energies).
//   k_shell_energy                one lane per triangle or hinge, one partial sum per block, reduced in a fixed order
//   k_shell_membrane<withHessian> one lane per triangle: 9-vector + six upper 3 x 3 blocks; carries the 6 x 6 Jacobi iterate (21 + 36 doubles) in registers
//   k_shell_hinge<withHessian>    one lane per hinge: 12-vector + ten upper 3 x 3 blocks (rank one: no eigen-iteration)
// Launch bounds differ on purpose: the membrane kernel with Hessian needs 137 VGPRs for the iterate and its rotations (64-lane workgroups so that the
// compiler may take them: three waves per SIMD, no scratch); the other two are small (63 .. 92 VGPRs) and run 256 wide.  Figures: DESIGN.md.
#include "shell_kernels.h"
#include "csr_scatter_device.h"
#include "shell_hinge_device.h"
#include "stencil_hessian_device.h"
#include <algorithm>

namespace ipcgpu {

namespace {

constexpr int ENERGY_BLOCK = 256;
constexpr int MEMBRANE_BLOCK = 64;
constexpr int HINGE_BLOCK = 256;

using namespace scatter; // projected_dbc, ld3, CsrSink, add_diag, add_off, store_block_sum, nblk, launch_reduce_partials (csr_scatter_device.h)

// ---- membrane ----------------------------------------------------------------------------------------------------------------------------
struct Membrane {
    double f1[3], f2[3]; // columns of F
    double b00, b10, b01, b11;
    double cm, cl; // coef h A mu, coef h A lambda_ps
    double S11, S12, S22; // second Piola-Kirchhoff stress times coef h A
    double energy;
};
__device__ __forceinline__ void membrane_state(const ShellView& v, int t, double coef, const double* x0, const double* x1, const double* x2, Membrane& m)
{
    const size_t n = (size_t)v.nTri;
    m.b00 = v.triConst[t];
    m.b10 = v.triConst[n + t];
    m.b01 = v.triConst[2 * n + t];
    m.b11 = v.triConst[3 * n + t];
    m.cm = coef * v.triConst[4 * n + t];
    m.cl = coef * v.triConst[5 * n + t];
    double c11 = 0.0, c12 = 0.0, c22 = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double e1 = x1[i] - x0[i], e2 = x2[i] - x0[i];
        m.f1[i] = e1 * m.b00 + e2 * m.b10;
        m.f2[i] = e1 * m.b01 + e2 * m.b11;
        c11 += m.f1[i] * m.f1[i];
        c12 += m.f1[i] * m.f2[i];
        c22 += m.f2[i] * m.f2[i];
    }
    const double G11 = 0.5 * (c11 - 1.0), G22 = 0.5 * (c22 - 1.0), G12 = 0.5 * c12, tr = G11 + G22;
    m.S11 = 2.0 * m.cm * G11 + m.cl * tr;
    m.S22 = 2.0 * m.cm * G22 + m.cl * tr;
    m.S12 = 2.0 * m.cm * G12;
    m.energy = m.cm * (G11 * G11 + 2.0 * G12 * G12 + G22 * G22) + 0.5 * m.cl * tr * tr;
}

// ---- hinge -------------------------------------------------------------------------------------------------------------------------------
// theta and (optionally) its gradient: hinge_angle<GRAD> of shell_hinge_device.h (shared with the hinges' plastic flow, shell_plastic_kernels.hip)

template <int K, int L>
__device__ __forceinline__ void emit_membrane_pair(const CsrSink& k, const double* C, const int* node, const bool* proj)
{
    if (proj[K] || proj[L]) return;
    double A[9];
    sh::pair_block<2, K, L, 6>(C, A);
    if constexpr (K == L) add_diag(k, node[K], A);
    else add_off(k, node[K], node[L], A);
}

__device__ __forceinline__ double triangle_energy(const ShellView& v, int t)
{
    double x0[3], x1[3], x2[3];
    ld3(v.x, v.tri[3 * (size_t)t], x0);
    ld3(v.x, v.tri[3 * (size_t)t + 1], x1);
    ld3(v.x, v.tri[3 * (size_t)t + 2], x2);
    Membrane m;
    membrane_state(v, t, 1.0, x0, x1, x2, m);
    return m.energy;
}
__device__ __forceinline__ double hinge_energy(const ShellView& v, int h)
{
    const int4 n = v.hinge[h];
    double x0[3], x1[3], x2[3], x3[3];
    ld3(v.x, n.x, x0);
    ld3(v.x, n.y, x1);
    ld3(v.x, n.z, x2);
    ld3(v.x, n.w, x3);
    const double d = hinge_angle<false>(x0, x1, x2, x3, nullptr) - v.hingeConst[h];
    return v.hingeConst[(size_t)v.nHinge + h] * d * d;
}

__global__ __launch_bounds__(ENERGY_BLOCK) void k_shell_energy(ShellView v, double coef, double* __restrict__ partial)
{
    const int gid = blockIdx.x * ENERGY_BLOCK + threadIdx.x;
    double e = 0.0;
    if (gid < v.nTri) e = coef * triangle_energy(v, gid);
    else if (gid - v.nTri < v.nHinge) e = coef * hinge_energy(v, gid - v.nTri);
    store_block_sum<ENERGY_BLOCK>(e, partial);
}
__global__ __launch_bounds__(ENERGY_BLOCK) void k_shell_energy_per_elem(ShellView v, double* __restrict__ perTri, double* __restrict__ perHinge)
{
    const int gid = blockIdx.x * ENERGY_BLOCK + threadIdx.x;
    if (gid < v.nTri) {
        if (perTri) perTri[gid] = triangle_energy(v, gid);
    }
    else if (gid - v.nTri < v.nHinge) {
        if (perHinge) perHinge[gid - v.nTri] = hinge_energy(v, gid - v.nTri);
    }
}

template <bool HESS>
__global__ __launch_bounds__(MEMBRANE_BLOCK) void k_shell_membrane(ShellView v, double coef, int projectDBC, double* __restrict__ grad, double* __restrict__ a,
    int* __restrict__ err)
{
    const int t = blockIdx.x * MEMBRANE_BLOCK + threadIdx.x;
    if (t >= v.nTri) return;
    const int node[3] = { v.tri[3 * (size_t)t], v.tri[3 * (size_t)t + 1], v.tri[3 * (size_t)t + 2] };
    bool proj[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) proj[k] = projected_dbc(v.dbc[node[k]], projectDBC);
    double x0[3], x1[3], x2[3];
    ld3(v.x, node[0], x0);
    ld3(v.x, node[1], x1);
    ld3(v.x, node[2], x2);
    Membrane m;
    membrane_state(v, t, coef, x0, x1, x2, m);
    if (grad) {
        // dW/dF = F S; with F = [e1, e2] Dm^-1 the forces on the two edge vectors are its columns times Dm^-T, node 0 takes minus their sum
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double p1 = m.S11 * m.f1[i] + m.S12 * m.f2[i], p2 = m.S12 * m.f1[i] + m.S22 * m.f2[i];
            const double g1 = p1 * m.b00 + p2 * m.b01, g2 = p1 * m.b10 + p2 * m.b11;
            if (!proj[0]) atomicAdd(&grad[3 * (size_t)node[0] + i], -g1 - g2);
            if (!proj[1]) atomicAdd(&grad[3 * (size_t)node[1] + i], g1);
            if (!proj[2]) atomicAdd(&grad[3 * (size_t)node[2] + i], g2);
        }
    }
    if constexpr (HESS) {
        // d2W / d(f1, f2)^2:  H11 = S11 I + (2 cm + cl) f1 f1^T + cm f2 f2^T,  H22 = S22 I + (2 cm + cl) f2 f2^T + cm f1 f1^T,
        //                     H12 = S12 I + cl f1 f2^T + cm f2 f1^T,  H21 = H12^T
        // in the Helmert coordinates z of the translation complement f_alpha = sum_a T[alpha][a] z_a, T from Dm^-1 and the Helmert rows of three nodes
        constexpr double R2 = 2.0 * sh::S2, R6 = 3.0 * sh::S6;
        const double T[2][2] = { { -R2 * m.b00 - sh::S2 * m.b10, -R6 * m.b10 }, { -R2 * m.b01 - sh::S2 * m.b11, -R6 * m.b11 } };
        const double c2 = 2.0 * m.cm + m.cl;
        double C[36];
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int p = 0; p <= q; ++p) {
                const double w11 = T[0][p] * T[0][q], w22 = T[1][p] * T[1][q], w12 = T[0][p] * T[1][q], w21 = T[1][p] * T[0][q];
                const double cI = w11 * m.S11 + w22 * m.S22 + (w12 + w21) * m.S12;
                const double k11 = w11 * c2 + w22 * m.cm, k22 = w22 * c2 + w11 * m.cm;
                const double k12 = w12 * m.cl + w21 * m.cm, k21 = w12 * m.cm + w21 * m.cl; // coefficients of f1 f2^T and f2 f1^T
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        if (p == q && j < i) continue;
                        double h = k11 * m.f1[i] * m.f1[j] + k22 * m.f2[i] * m.f2[j] + k12 * m.f1[i] * m.f2[j] + k21 * m.f2[i] * m.f1[j];
                        if (i == j) h += cI;
                        C[sh::su<6>(3 * p + i, 3 * q + j)] = h;
                    }
            }
        sh::project_psd<6>(C);
        const CsrSink k{ v.rowBase, v.rowLen, v.ja, a, err };
        emit_membrane_pair<0, 0>(k, C, node, proj);
        emit_membrane_pair<0, 1>(k, C, node, proj);
        emit_membrane_pair<1, 1>(k, C, node, proj);
        emit_membrane_pair<0, 2>(k, C, node, proj);
        emit_membrane_pair<1, 2>(k, C, node, proj);
        emit_membrane_pair<2, 2>(k, C, node, proj);
    }
}

template <bool HESS>
__global__ __launch_bounds__(HINGE_BLOCK) void k_shell_hinge(ShellView v, double coef, int projectDBC, double* __restrict__ grad, double* __restrict__ a,
    int* __restrict__ err)
{
    const int h = blockIdx.x * HINGE_BLOCK + threadIdx.x;
    if (h >= v.nHinge) return;
    const int4 n4 = v.hinge[h];
    const int node[4] = { n4.x, n4.y, n4.z, n4.w };
    bool proj[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) proj[k] = projected_dbc(v.dbc[node[k]], projectDBC);
    double x[4][3], g[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) ld3(v.x, node[k], x[k]);
    const double theta = hinge_angle<true>(x[0], x[1], x[2], x[3], g);
    const double kw2 = 2.0 * coef * v.hingeConst[(size_t)v.nHinge + h];
    if (grad) {
        const double s = kw2 * (theta - v.hingeConst[h]);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (!proj[k]) {
#pragma unroll
                for (int i = 0; i < 3; ++i) atomicAdd(&grad[3 * (size_t)node[k] + i], s * g[k][i]);
            }
    }
    if constexpr (HESS) {
        const CsrSink sink{ v.rowBase, v.rowLen, v.ja, a, err };
#pragma unroll
        for (int l = 0; l < 4; ++l)
#pragma unroll
            for (int k = 0; k <= l; ++k) {
                if (proj[k] || proj[l]) continue;
                double A[9];
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) A[r + 3 * c] = kw2 * g[k][r] * g[l][c];
                if (k == l) add_diag(sink, node[k], A);
                else add_off(sink, node[k], node[l], A);
            }
    }
}

} // namespace

int shell_energy_blocks(const ShellView& v) { return std::max(1, nblk(v.nTri + v.nHinge, ENERGY_BLOCK)); }

void launch_shell_energy(const ShellView& v, double coef, double* partial, double* out, bool accumulate, hipStream_t s)
{
    const int nb = shell_energy_blocks(v);
    hipLaunchKernelGGL(k_shell_energy, dim3(nb), dim3(ENERGY_BLOCK), 0, s, v, coef, partial);
    launch_reduce_partials(partial, nb, 1.0, accumulate, out, s);
}
void launch_shell_energy_per_elem(const ShellView& v, double* perTri, double* perHinge, hipStream_t s)
{
    if (v.nTri + v.nHinge <= 0) return;
    hipLaunchKernelGGL(k_shell_energy_per_elem, dim3(nblk(v.nTri + v.nHinge, ENERGY_BLOCK)), dim3(ENERGY_BLOCK), 0, s, v, perTri, perHinge);
}
void launch_shell_assemble(const ShellView& v, double coef, int projectDBC, double* grad, double* a, int* err, hipStream_t s)
{
    if (v.nTri > 0) {
        if (a) hipLaunchKernelGGL(k_shell_membrane<true>, dim3(nblk(v.nTri, MEMBRANE_BLOCK)), dim3(MEMBRANE_BLOCK), 0, s, v, coef, projectDBC, grad, a, err);
        else hipLaunchKernelGGL(k_shell_membrane<false>, dim3(nblk(v.nTri, MEMBRANE_BLOCK)), dim3(MEMBRANE_BLOCK), 0, s, v, coef, projectDBC, grad, a, err);
    }
    if (v.nHinge > 0) {
        if (a) hipLaunchKernelGGL(k_shell_hinge<true>, dim3(nblk(v.nHinge, HINGE_BLOCK)), dim3(HINGE_BLOCK), 0, s, v, coef, projectDBC, grad, a, err);
        else hipLaunchKernelGGL(k_shell_hinge<false>, dim3(nblk(v.nHinge, HINGE_BLOCK)), dim3(HINGE_BLOCK), 0, s, v, coef, projectDBC, grad, a, err);
    }
}

} // namespace ipcgpu
