// Woven cloth of the elastic shells: kernels (see shell_weave_kernels.h for the energy).
//   k_shell_weave_energy          one lane per woven triangle, one partial sum per block, reduced in a fixed order
//   k_shell_weave_energy_per_elem one lane per woven triangle, scattered to the shell's triangle index
//   k_shell_weave<withHessian>    one lane per woven triangle: 9-vector + six upper 3 x 3 blocks; carries the 6 x 6 Jacobi iterate in registers
//   k_shell_weave_state           one lane per woven triangle: six plain stores to the shell's triangle index
// The assemble kernel runs 64 wide for the same reason k_shell_membrane does (the iterate and its rotations); the others 256 wide.  Figures: DESIGN.md.
#include "shell_weave_kernels.h"
#include "csr_scatter_device.h"
#include "stencil_hessian_device.h"
#include <algorithm>
#include <cmath>

namespace ipcgpu {

namespace {

constexpr int ENERGY_BLOCK = 256;
constexpr int WEAVE_BLOCK = 64;

using namespace scatter; // projected_dbc, ld3, CsrSink, add_diag, add_off, store_block_sum, nblk, launch_reduce_partials (csr_scatter_device.h)

// the membrane's per-lane state (shell_kernels.hip) in the yarn frame: two columns, Dm^-1 R, the stress -- and four moduli where it has two
struct Weave {
    int node[3];
    double g1[3], g2[3]; // F a, F b
    double b00, b10, b01, b11; // Dm^-1 R, R = [a, b]
    double k11, k12, k22, kg; // coef h A (C11, C12, C22, G12)
    double S11, S12, S22; // s_ww, s_wf, s_ff times coef h A
    double Eww, Eff, Ewf;
    double energy; // times coef
};
__device__ __forceinline__ void weave_state(const ShellWeaveView& v, int i, double coef, Weave& m)
{
    const int t = v.wovTri[i];
    const size_t n = (size_t)v.nTri, nw = (size_t)v.nWoven;
    double x0[3], x1[3], x2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) m.node[k] = v.tri[3 * (size_t)t + k];
    ld3(v.x, m.node[0], x0);
    ld3(v.x, m.node[1], x1);
    ld3(v.x, m.node[2], x2);
    const double d00 = v.triConst[t], d10 = v.triConst[n + t], d01 = v.triConst[2 * n + t], d11 = v.triConst[3 * n + t];
    const double ax = v.wovConst[i], ay = v.wovConst[nw + i];
    m.b00 = d00 * ax + d01 * ay;
    m.b10 = d10 * ax + d11 * ay;
    m.b01 = d01 * ax - d00 * ay;
    m.b11 = d11 * ax - d10 * ay;
    m.k11 = coef * v.wovConst[2 * nw + i];
    m.k12 = coef * v.wovConst[3 * nw + i];
    m.k22 = coef * v.wovConst[4 * nw + i];
    m.kg = coef * v.wovConst[5 * nw + i];
    double c11 = 0.0, c12 = 0.0, c22 = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double e1 = x1[c] - x0[c], e2 = x2[c] - x0[c];
        m.g1[c] = e1 * m.b00 + e2 * m.b10;
        m.g2[c] = e1 * m.b01 + e2 * m.b11;
        c11 += m.g1[c] * m.g1[c];
        c12 += m.g1[c] * m.g2[c];
        c22 += m.g2[c] * m.g2[c];
    }
    m.Eww = 0.5 * (c11 - 1.0);
    m.Eff = 0.5 * (c22 - 1.0);
    m.Ewf = 0.5 * c12;
    m.S11 = m.k11 * m.Eww + m.k12 * m.Eff;
    m.S22 = m.k12 * m.Eww + m.k22 * m.Eff;
    m.S12 = 2.0 * m.kg * m.Ewf;
    m.energy = 0.5 * (m.k11 * m.Eww * m.Eww + m.k22 * m.Eff * m.Eff) + m.k12 * m.Eww * m.Eff + 2.0 * m.kg * m.Ewf * m.Ewf;
}

template <int K, int L>
__device__ __forceinline__ void emit_pair(const CsrSink& k, const double* C, const int* node, const bool* proj)
{
    if (proj[K] || proj[L]) return;
    double A[9];
    sh::pair_block<2, K, L, 6>(C, A);
    if constexpr (K == L) add_diag(k, node[K], A);
    else add_off(k, node[K], node[L], A);
}

__global__ __launch_bounds__(ENERGY_BLOCK) void k_shell_weave_energy(ShellWeaveView v, double coef, double* __restrict__ partial)
{
    const int i = blockIdx.x * ENERGY_BLOCK + threadIdx.x;
    double e = 0.0;
    if (i < v.nWoven) {
        Weave m;
        weave_state(v, i, 1.0, m);
        e = coef * m.energy;
    }
    store_block_sum<ENERGY_BLOCK>(e, partial);
}
__global__ __launch_bounds__(ENERGY_BLOCK) void k_shell_weave_energy_per_elem(ShellWeaveView v, double* __restrict__ perTri)
{
    const int i = blockIdx.x * ENERGY_BLOCK + threadIdx.x;
    if (i >= v.nWoven) return;
    Weave m;
    weave_state(v, i, 1.0, m);
    perTri[v.wovTri[i]] = m.energy;
}
__global__ __launch_bounds__(ENERGY_BLOCK) void k_shell_weave_state(ShellWeaveView v, double* __restrict__ state)
{
    const int i = blockIdx.x * ENERGY_BLOCK + threadIdx.x;
    if (i >= v.nWoven) return;
    Weave m;
    weave_state(v, i, 1.0, m);
    const size_t n = (size_t)v.nTri, t = (size_t)v.wovTri[i];
    const double l1 = sqrt(m.g1[0] * m.g1[0] + m.g1[1] * m.g1[1] + m.g1[2] * m.g1[2]), l2 = sqrt(m.g2[0] * m.g2[0] + m.g2[1] * m.g2[1] + m.g2[2] * m.g2[2]);
    const double s = (m.g1[0] * m.g2[0] + m.g1[1] * m.g2[1] + m.g1[2] * m.g2[2]) / (l1 * l2);
    state[t] = m.Eww;
    state[n + t] = m.Eff;
    state[2 * n + t] = asin(fmin(1.0, fmax(-1.0, s))); // (fmin / fmax would drop a NaN: put it back below)
    if (!(l1 > 0.0) || !(l2 > 0.0)) state[2 * n + t] = NAN;
#pragma unroll
    for (int c = 0; c < 3; ++c) state[(3 + c) * n + t] = l1 > 0.0 ? m.g1[c] / l1 : NAN;
}

template <bool HESS>
__global__ __launch_bounds__(WEAVE_BLOCK) void k_shell_weave(ShellWeaveView v, double coef, int projectDBC, double* __restrict__ grad, double* __restrict__ a,
    int* __restrict__ err)
{
    const int i = blockIdx.x * WEAVE_BLOCK + threadIdx.x;
    if (i >= v.nWoven) return;
    Weave m;
    weave_state(v, i, coef, m);
    bool proj[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) proj[k] = projected_dbc(v.dbc[m.node[k]], projectDBC);
    if (grad) {
        // dW/d(F R) = (F R) S; with F R = [e1, e2] (Dm^-1 R) the forces on the two edge vectors are its columns times (Dm^-1 R)^T, node 0 takes minus their sum
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double p1 = m.S11 * m.g1[c] + m.S12 * m.g2[c], p2 = m.S12 * m.g1[c] + m.S22 * m.g2[c];
            const double q1 = p1 * m.b00 + p2 * m.b01, q2 = p1 * m.b10 + p2 * m.b11;
            if (!proj[0]) atomicAdd(&grad[3 * (size_t)m.node[0] + c], -q1 - q2);
            if (!proj[1]) atomicAdd(&grad[3 * (size_t)m.node[1] + c], q1);
            if (!proj[2]) atomicAdd(&grad[3 * (size_t)m.node[2] + c], q2);
        }
    }
    if constexpr (HESS) {
        // d2W / d(g1, g2)^2:  H11 = S11 I + k11 g1 g1^T + kg g2 g2^T,  H22 = S22 I + k22 g2 g2^T + kg g1 g1^T,
        //                     H12 = S12 I + k12 g1 g2^T + kg g2 g1^T,  H21 = H12^T
        // in the Helmert coordinates z of the translation complement g_alpha = sum_a T[alpha][a] z_a, T from Dm^-1 R and the Helmert rows of three nodes
        constexpr double R2 = 2.0 * sh::S2, R6 = 3.0 * sh::S6;
        const double T[2][2] = { { -R2 * m.b00 - sh::S2 * m.b10, -R6 * m.b10 }, { -R2 * m.b01 - sh::S2 * m.b11, -R6 * m.b11 } };
        double C[36];
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int p = 0; p <= q; ++p) {
                const double w11 = T[0][p] * T[0][q], w22 = T[1][p] * T[1][q], w12 = T[0][p] * T[1][q], w21 = T[1][p] * T[0][q];
                const double cI = w11 * m.S11 + w22 * m.S22 + (w12 + w21) * m.S12;
                const double k11 = w11 * m.k11 + w22 * m.kg, k22 = w22 * m.k22 + w11 * m.kg;
                const double k12 = w12 * m.k12 + w21 * m.kg, k21 = w12 * m.kg + w21 * m.k12; // coefficients of g1 g2^T and g2 g1^T
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        if (p == q && c < r) continue;
                        double h = k11 * m.g1[r] * m.g1[c] + k22 * m.g2[r] * m.g2[c] + k12 * m.g1[r] * m.g2[c] + k21 * m.g2[r] * m.g1[c];
                        if (r == c) h += cI;
                        C[sh::su<6>(3 * p + r, 3 * q + c)] = h;
                    }
            }
        sh::project_psd<6>(C);
        const CsrSink k{ v.rowBase, v.rowLen, v.ja, a, err };
        emit_pair<0, 0>(k, C, m.node, proj);
        emit_pair<0, 1>(k, C, m.node, proj);
        emit_pair<1, 1>(k, C, m.node, proj);
        emit_pair<0, 2>(k, C, m.node, proj);
        emit_pair<1, 2>(k, C, m.node, proj);
        emit_pair<2, 2>(k, C, m.node, proj);
    }
}

} // namespace

int shell_weave_energy_blocks(const ShellWeaveView& v) { return std::max(1, nblk(v.nWoven, ENERGY_BLOCK)); }

void launch_shell_weave_energy(const ShellWeaveView& v, double coef, double* partial, double* out, bool accumulate, hipStream_t s)
{
    const int nb = shell_weave_energy_blocks(v);
    hipLaunchKernelGGL(k_shell_weave_energy, dim3(nb), dim3(ENERGY_BLOCK), 0, s, v, coef, partial);
    launch_reduce_partials(partial, nb, 1.0, accumulate, out, s);
}
void launch_shell_weave_energy_per_elem(const ShellWeaveView& v, double* perTri, hipStream_t s)
{
    if (v.nTri <= 0) return;
    (void)hipMemsetAsync(perTri, 0, sizeof(double) * (size_t)v.nTri, s);
    if (v.nWoven > 0) hipLaunchKernelGGL(k_shell_weave_energy_per_elem, dim3(nblk(v.nWoven, ENERGY_BLOCK)), dim3(ENERGY_BLOCK), 0, s, v, perTri);
}
void launch_shell_weave_assemble(const ShellWeaveView& v, double coef, int projectDBC, double* grad, double* a, int* err, hipStream_t s)
{
    if (v.nWoven <= 0) return;
    if (a) hipLaunchKernelGGL(k_shell_weave<true>, dim3(nblk(v.nWoven, WEAVE_BLOCK)), dim3(WEAVE_BLOCK), 0, s, v, coef, projectDBC, grad, a, err);
    else hipLaunchKernelGGL(k_shell_weave<false>, dim3(nblk(v.nWoven, WEAVE_BLOCK)), dim3(WEAVE_BLOCK), 0, s, v, coef, projectDBC, grad, a, err);
}
void launch_shell_weave_state(const ShellWeaveView& v, double* state, hipStream_t s)
{
    if (v.nTri <= 0) return;
    (void)hipMemsetAsync(state, 0, sizeof(double) * 6 * (size_t)v.nTri, s);
    if (v.nWoven > 0) hipLaunchKernelGGL(k_shell_weave_state, dim3(nblk(v.nWoven, ENERGY_BLOCK)), dim3(ENERGY_BLOCK), 0, s, v, state);
}

} // namespace ipcgpu
