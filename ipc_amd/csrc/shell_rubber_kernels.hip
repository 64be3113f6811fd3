// Rubber membrane of the elastic shells: kernels (see shell_rubber_kernels.h for the energy).
//   k_shell_rubber_energy          one lane per rubber triangle, one partial sum per block, reduced in a fixed order
//   k_shell_rubber_energy_per_elem one lane per rubber triangle, scattered to the shell's triangle index
//   k_shell_rubber<withHessian>    one lane per rubber triangle: 9-vector + six upper 3 x 3 blocks; carries the 6 x 6 Jacobi iterate in registers
//   k_shell_rubber_degenerate      one lane per rubber triangle: 1 where the energy is +infinity, summed like the energy
// The assemble kernel runs 64 wide for the same reason k_shell_membrane does (the iterate and its rotations); the others 256 wide.  Figures: DESIGN.md.
#include "shell_rubber_kernels.h"
#include "csr_scatter_device.h"
#include "stencil_hessian_device.h"
#include <algorithm>
#include <cmath>

namespace ipcgpu {

namespace {

constexpr int ENERGY_BLOCK = 256;
constexpr int RUBBER_BLOCK = 64;

using namespace scatter; // projected_dbc, ld3, CsrSink, add_diag, add_off, store_block_sum, nblk, launch_reduce_partials (csr_scatter_device.h)

struct Rubber {
    int node[3];
    double f1[3], f2[3]; // columns of F
    double b00, b10, b01, b11;
    double c11, c12, c22, J; // C and det C = |f1 x f2|^2
    double a, b, p, q; // S = a I + b adj C; coefficients of j t^T + t j^T and of j j^T
    double energy; // without coef; +infinity where !ok
    bool ok; // J > 0 and everything finite
};
// k1, k2 enter scaled by coef
__device__ __forceinline__ void rubber_state(const ShellRubberView& v, int i, double coef, Rubber& m)
{
    const int t = v.rubTri[i];
    const size_t n = (size_t)v.nTri, nr = (size_t)v.nRubber;
    double x0[3], x1[3], x2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) m.node[k] = v.tri[3 * (size_t)t + k];
    ld3(v.x, m.node[0], x0);
    ld3(v.x, m.node[1], x1);
    ld3(v.x, m.node[2], x2);
    m.b00 = v.triConst[t];
    m.b10 = v.triConst[n + t];
    m.b01 = v.triConst[2 * n + t];
    m.b11 = v.triConst[3 * n + t];
    const double k1 = v.rubConst[i], k2 = v.rubConst[nr + i];
    double c11 = 0.0, c12 = 0.0, c22 = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double e1 = x1[c] - x0[c], e2 = x2[c] - x0[c];
        m.f1[c] = e1 * m.b00 + e2 * m.b10;
        m.f2[c] = e1 * m.b01 + e2 * m.b11;
        c11 += m.f1[c] * m.f1[c];
        c12 += m.f1[c] * m.f2[c];
        c22 += m.f2[c] * m.f2[c];
    }
    const double n0 = m.f1[1] * m.f2[2] - m.f1[2] * m.f2[1], n1 = m.f1[2] * m.f2[0] - m.f1[0] * m.f2[2], n2 = m.f1[0] * m.f2[1] - m.f1[1] * m.f2[0];
    const double J = n0 * n0 + n1 * n1 + n2 * n2, tr = c11 + c22;
    m.c11 = c11;
    m.c12 = c12;
    m.c22 = c22;
    m.J = J;
    const double iJ = 1.0 / J, s = (k1 + k2 * tr) * (iJ * iJ);
    const double a = 2.0 * (k1 + k2 * iJ), b = 2.0 * (k2 - s), p = -k2 * (iJ * iJ), q = 2.0 * s * iJ;
    const double w = k1 * ((tr + iJ) - 3.0) + k2 * ((tr * iJ + J) - 3.0);
    // decided on the unscaled coefficients, so that every kernel calls the same triangles degenerate whatever its coef (a NaN compares false)
    m.ok = J > 0.0 && J < INFINITY && isfinite(a) && isfinite(b) && isfinite(q) && w < INFINITY;
    m.a = coef * a;
    m.b = coef * b;
    m.p = coef * p;
    m.q = coef * q;
    m.energy = m.ok ? w : INFINITY;
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

__global__ __launch_bounds__(ENERGY_BLOCK) void k_shell_rubber_energy(ShellRubberView v, double coef, double* __restrict__ partial)
{
    const int i = blockIdx.x * ENERGY_BLOCK + threadIdx.x;
    double e = 0.0;
    if (i < v.nRubber) {
        Rubber m;
        rubber_state(v, i, 1.0, m);
        e = coef * m.energy; // (coef > 0: an infinite term stays +infinity)
    }
    store_block_sum<ENERGY_BLOCK>(e, partial);
}
__global__ __launch_bounds__(ENERGY_BLOCK) void k_shell_rubber_energy_per_elem(ShellRubberView v, double* __restrict__ perTri)
{
    const int i = blockIdx.x * ENERGY_BLOCK + threadIdx.x;
    if (i >= v.nRubber) return;
    Rubber m;
    rubber_state(v, i, 1.0, m);
    perTri[v.rubTri[i]] = m.energy;
}
__global__ __launch_bounds__(ENERGY_BLOCK) void k_shell_rubber_degenerate(ShellRubberView v, double* __restrict__ partial)
{
    const int i = blockIdx.x * ENERGY_BLOCK + threadIdx.x;
    double e = 0.0;
    if (i < v.nRubber) {
        Rubber m;
        rubber_state(v, i, 1.0, m);
        e = m.ok ? 0.0 : 1.0;
    }
    store_block_sum<ENERGY_BLOCK>(e, partial);
}

template <bool HESS>
__global__ __launch_bounds__(RUBBER_BLOCK) void k_shell_rubber(ShellRubberView v, double coef, int projectDBC, double* __restrict__ grad, double* __restrict__ a,
    int* __restrict__ err)
{
    const int i = blockIdx.x * RUBBER_BLOCK + threadIdx.x;
    if (i >= v.nRubber) return;
    Rubber m;
    rubber_state(v, i, coef, m);
    if (!m.ok) return; // degenerate: energy +infinity, no derivative
    bool proj[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) proj[k] = projected_dbc(v.dbc[m.node[k]], projectDBC);
    const double S11 = m.a + m.b * m.c22, S22 = m.a + m.b * m.c11, S12 = -m.b * m.c12;
    if (grad) {
        // dW/dF = F S; with F = [e1, e2] Dm^-1 the forces on the two edge vectors are its columns times Dm^-T, node 0 takes minus their sum
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double p1 = S11 * m.f1[c] + S12 * m.f2[c], p2 = S12 * m.f1[c] + S22 * m.f2[c];
            const double g1 = p1 * m.b00 + p2 * m.b01, g2 = p1 * m.b10 + p2 * m.b11;
            if (!proj[0]) atomicAdd(&grad[3 * (size_t)m.node[0] + c], -g1 - g2);
            if (!proj[1]) atomicAdd(&grad[3 * (size_t)m.node[1] + c], g1);
            if (!proj[2]) atomicAdd(&grad[3 * (size_t)m.node[2] + c], g2);
        }
    }
    if constexpr (HESS) {
        // d2W / d(f_al, f_be) = S[al][be] I + sum over mu, nu of M[2 al + mu][2 be + nu] f_mu f_nu^T,  M (4 x 4, symmetric) from the 6-vectors of the header
        // written by their coefficients on (f1, f2):  t = (2, 0, 0, 2),  j = 2 (C22, -C12, -C12, C11),  u1 = (2, 0, 0, 0),  u2 = (0, 0, 0, 2),  u12 = (0, 1, 1, 0)
        const double jt[4] = { 2.0 * m.c22, -2.0 * m.c12, -2.0 * m.c12, 2.0 * m.c11 };
        constexpr double tt[4] = { 2.0, 0.0, 0.0, 2.0 }, u1[4] = { 2.0, 0.0, 0.0, 0.0 }, u2[4] = { 0.0, 0.0, 0.0, 2.0 }, u12[4] = { 0.0, 1.0, 1.0, 0.0 };
        const double hb = 0.5 * m.b;
        double M[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int s = 0; s < 4; ++s)
                M[r][s] = m.p * (jt[r] * tt[s] + tt[r] * jt[s]) + m.q * jt[r] * jt[s] + hb * (u1[r] * u2[s] + u2[r] * u1[s] - 2.0 * u12[r] * u12[s]);
        // in the Helmert coordinates z of the translation complement f_alpha = sum_a T[alpha][a] z_a, T from Dm^-1 and the Helmert rows of three nodes
        constexpr double R2 = 2.0 * sh::S2, R6 = 3.0 * sh::S6;
        const double T[2][2] = { { -R2 * m.b00 - sh::S2 * m.b10, -R6 * m.b10 }, { -R2 * m.b01 - sh::S2 * m.b11, -R6 * m.b11 } };
        double C[36];
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int p = 0; p <= q; ++p) {
                const double w[2][2] = { { T[0][p] * T[0][q], T[0][p] * T[1][q] }, { T[1][p] * T[0][q], T[1][p] * T[1][q] } }; // w[al][be]
                const double cI = w[0][0] * S11 + w[1][1] * S22 + (w[0][1] + w[1][0]) * S12;
                double K[2][2]; // coefficient of f_mu f_nu^T
#pragma unroll
                for (int mu = 0; mu < 2; ++mu)
#pragma unroll
                    for (int nu = 0; nu < 2; ++nu)
                        K[mu][nu] = w[0][0] * M[mu][nu] + w[0][1] * M[mu][2 + nu] + w[1][0] * M[2 + mu][nu] + w[1][1] * M[2 + mu][2 + nu];
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        if (p == q && c < r) continue;
                        double h = K[0][0] * m.f1[r] * m.f1[c] + K[1][1] * m.f2[r] * m.f2[c] + K[0][1] * m.f1[r] * m.f2[c] + K[1][0] * m.f2[r] * m.f1[c];
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

int shell_rubber_energy_blocks(const ShellRubberView& v) { return std::max(1, nblk(v.nRubber, ENERGY_BLOCK)); }

void launch_shell_rubber_energy(const ShellRubberView& v, double coef, double* partial, double* out, bool accumulate, hipStream_t s)
{
    const int nb = shell_rubber_energy_blocks(v);
    hipLaunchKernelGGL(k_shell_rubber_energy, dim3(nb), dim3(ENERGY_BLOCK), 0, s, v, coef, partial);
    launch_reduce_partials(partial, nb, 1.0, accumulate, out, s);
}
void launch_shell_rubber_energy_per_elem(const ShellRubberView& v, double* perTri, hipStream_t s)
{
    if (v.nTri <= 0) return;
    (void)hipMemsetAsync(perTri, 0, sizeof(double) * (size_t)v.nTri, s);
    if (v.nRubber > 0) hipLaunchKernelGGL(k_shell_rubber_energy_per_elem, dim3(nblk(v.nRubber, ENERGY_BLOCK)), dim3(ENERGY_BLOCK), 0, s, v, perTri);
}
void launch_shell_rubber_assemble(const ShellRubberView& v, double coef, int projectDBC, double* grad, double* a, int* err, hipStream_t s)
{
    if (v.nRubber <= 0) return;
    if (a) hipLaunchKernelGGL(k_shell_rubber<true>, dim3(nblk(v.nRubber, RUBBER_BLOCK)), dim3(RUBBER_BLOCK), 0, s, v, coef, projectDBC, grad, a, err);
    else hipLaunchKernelGGL(k_shell_rubber<false>, dim3(nblk(v.nRubber, RUBBER_BLOCK)), dim3(RUBBER_BLOCK), 0, s, v, coef, projectDBC, grad, a, err);
}
void launch_shell_rubber_degenerate(const ShellRubberView& v, double* partial, double* out, hipStream_t s)
{
    const int nb = shell_rubber_energy_blocks(v);
    hipLaunchKernelGGL(k_shell_rubber_degenerate, dim3(nb), dim3(ENERGY_BLOCK), 0, s, v, partial);
    launch_reduce_partials(partial, nb, 1.0, false, out, s);
}

} // namespace ipcgpu
