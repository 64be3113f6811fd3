// Strain limiting of the elastic shells: kernels (see shell_limit_kernels.h for the energy).
//   k_shell_limit_energy       one lane per limited triangle, one partial sum per block, reduced in a fixed order
//   k_shell_limit<withHessian> one lane per limited triangle: 9-vector + six upper 3 x 3 blocks (closed-form eigenpairs: no eigen-iteration)
//   k_shell_stretch            one lane per triangle of the shell: sigma1, sigma2, and per block the maximum of sigma1 / limit and the count at or over it
// All 256 wide, no scratch.  Figures: DESIGN.md.
#include "shell_limit_kernels.h"
#include "csr_scatter_device.h"
#include <algorithm>
#include <cmath>

namespace ipcgpu {

namespace {

constexpr int BLOCK = 256;

using namespace scatter; // projected_dbc, ld3, CsrSink, add_diag, add_off, block_sum, store_block_sum, nblk, launch_reduce_partials (csr_scatter_device.h)

struct Stretch {
    double f1[3], f2[3]; // columns of F
    double g[3][2]; // F = sum_k x_k g[k]^T: rows of Dm^-1 for nodes 1 and 2, minus their sum for node 0
    double c12, d, r; // C12, (C11 - C22) / 2, sqrt(d^2 + C12^2)
    double n[3], nn; // f1 x f2 and its length = sigma1 sigma2
    double s1, s2;
};
__device__ __forceinline__ void stretch_state(const ShellLimitView& v, int t, Stretch& m)
{
    double x0[3], x1[3], x2[3];
    ld3(v.x, v.tri[3 * (size_t)t], x0);
    ld3(v.x, v.tri[3 * (size_t)t + 1], x1);
    ld3(v.x, v.tri[3 * (size_t)t + 2], x2);
    const size_t n = (size_t)v.nTri;
    const double b00 = v.triConst[t], b10 = v.triConst[n + t], b01 = v.triConst[2 * n + t], b11 = v.triConst[3 * n + t];
    m.g[1][0] = b00;
    m.g[1][1] = b01;
    m.g[2][0] = b10;
    m.g[2][1] = b11;
    m.g[0][0] = -b00 - b10;
    m.g[0][1] = -b01 - b11;
    double c11 = 0.0, c12 = 0.0, c22 = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double e1 = x1[i] - x0[i], e2 = x2[i] - x0[i];
        m.f1[i] = e1 * b00 + e2 * b10;
        m.f2[i] = e1 * b01 + e2 * b11;
        c11 += m.f1[i] * m.f1[i];
        c12 += m.f1[i] * m.f2[i];
        c22 += m.f2[i] * m.f2[i];
    }
    m.c12 = c12;
    m.d = 0.5 * (c11 - c22);
    m.r = sqrt(m.d * m.d + c12 * c12);
    m.n[0] = m.f1[1] * m.f2[2] - m.f1[2] * m.f2[1];
    m.n[1] = m.f1[2] * m.f2[0] - m.f1[0] * m.f2[2];
    m.n[2] = m.f1[0] * m.f2[1] - m.f1[1] * m.f2[0];
    m.nn = sqrt(m.n[0] * m.n[0] + m.n[1] * m.n[1] + m.n[2] * m.n[2]);
    m.s1 = sqrt(0.5 * (c11 + c22) + m.r);
    m.s2 = m.s1 > 0.0 ? fmin(m.nn / m.s1, m.s1) : 0.0; // (the clamp only removes a rounding of sigma1 = sigma2)
}

// b, b' and b'' at sigma < lim (zeros at or below the onset)
struct Barrier {
    double y, z, L; // (sigma - on) / (lim - on), (lim - sigma) / (lim - on), ln z
    double b, d1, d2;
};
__device__ __forceinline__ void barrier(double sigma, double on, double lim, Barrier& q)
{
    q.y = q.b = q.d1 = q.d2 = q.L = 0.0;
    q.z = 1.0;
    if (!(sigma > on)) return;
    const double w = lim - on, iw = 1.0 / w;
    q.y = (sigma - on) * iw;
    q.z = (lim - sigma) * iw;
    q.L = q.y < 0.5 ? log1p(-q.y) : log(q.z);
    const double yz = q.y / q.z;
    q.b = -q.y * q.y * q.L;
    q.d1 = fmax(0.0, (-2.0 * q.y * q.L + q.y * yz) * iw);
    q.d2 = fmax(0.0, (-2.0 * q.L + 4.0 * yz + yz * yz) * (iw * iw));
}

// energy of limited triangle i (index into the compact list) without k; +infinity at or over the limit or where sigma1 does not compare
__device__ __forceinline__ double limit_energy(const ShellLimitView& v, int i)
{
    const size_t nl = (size_t)v.nLimited;
    const double on = v.limConst[i], lim = v.limConst[nl + i];
    Stretch m;
    stretch_state(v, v.limTri[i], m);
    if (!(m.s1 < lim)) return INFINITY;
    if (!(m.s1 > on)) return 0.0;
    Barrier b1, b2;
    barrier(m.s1, on, lim, b1);
    barrier(m.s2, on, lim, b2);
    return v.limConst[2 * nl + i] * (b1.b + b2.b);
}

__global__ __launch_bounds__(BLOCK) void k_shell_limit_energy(ShellLimitView v, double coef, double* __restrict__ partial)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    double e = 0.0;
    if (i < v.nLimited) {
        e = limit_energy(v, i);
        if (e != 0.0) e *= coef; // (coef > 0: an infinite term stays +infinity)
    }
    store_block_sum<BLOCK>(e, partial);
}
__global__ __launch_bounds__(BLOCK) void k_shell_limit_energy_per_elem(ShellLimitView v, double* __restrict__ perTri)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < v.nLimited) perTri[v.limTri[i]] = limit_energy(v, i);
}

template <bool HESS>
__global__ __launch_bounds__(BLOCK) void k_shell_limit(ShellLimitView v, double coef, int projectDBC, double* __restrict__ grad, double* __restrict__ a,
    int* __restrict__ err)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= v.nLimited) return;
    const size_t nl = (size_t)v.nLimited;
    const int t = v.limTri[i];
    const double on = v.limConst[i], lim = v.limConst[nl + i], kk = coef * v.limConst[2 * nl + i];
    Stretch m;
    stretch_state(v, t, m);
    if (!(m.s1 < lim) || !(m.s1 > on)) return; // over the limit: energy +infinity, no derivative; below the onset: exact zeros
    const int node[3] = { v.tri[3 * (size_t)t], v.tri[3 * (size_t)t + 1], v.tri[3 * (size_t)t + 2] };
    bool proj[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) proj[k] = projected_dbc(v.dbc[node[k]], projectDBC);
    Barrier b1, b2;
    barrier(m.s1, on, lim, b1);
    barrier(m.s2, on, lim, b2);
    const bool both = m.s2 > on;
    // v1: the eigenvector of C for sigma1^2, a column of C - sigma2^2 I = [[r + d, C12], [C12, r - d]] (the longer one); v2 = (-v1y, v1x)
    double vx = 1.0, vy = 0.0;
    if (m.r > 0.0) {
        vx = m.d >= 0.0 ? m.r + m.d : m.c12;
        vy = m.d >= 0.0 ? m.c12 : m.r - m.d;
        const double il = 1.0 / sqrt(vx * vx + vy * vy);
        vx *= il;
        vy *= il;
    }
    double u1[3], w[3], sk[3], tk[3]; // u1 = F v1 / sigma1, w = F v2 = sigma2 u2; s_k = v1 . g_k, t_k = v2 . g_k
    const double is1 = 1.0 / m.s1;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        u1[c] = (m.f1[c] * vx + m.f2[c] * vy) * is1;
        w[c] = m.f2[c] * vx - m.f1[c] * vy;
        sk[c] = m.g[c][0] * vx + m.g[c][1] * vy;
        tk[c] = m.g[c][1] * vx - m.g[c][0] * vy;
    }
    const double is2 = both ? 1.0 / m.s2 : 0.0; // (sigma2 > onset >= 1 where it is used)
    if (grad) {
        const double p1 = kk * b1.d1, p2 = kk * b2.d1 * is2;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (!proj[k]) {
#pragma unroll
                for (int c = 0; c < 3; ++c) atomicAdd(&grad[3 * (size_t)node[k] + c], p1 * sk[k] * u1[c] + p2 * tk[k] * w[c]);
            }
    }
    if constexpr (HESS) {
        // block (k, l) = s_k s_l S + t_k t_l T + t_k s_l X + s_k t_l X^T
        double S[9], T[9], X[9];
        if (both) {
            const double iw = 1.0 / (lim - on), iw2 = iw * iw;
            // y1 - y2 from sigma1 - sigma2 = 2 r / (sigma1 + sigma2): a few ulps apart, the difference of the two rounded stretches is noise.  q in [0, 1):
            // 1 - q = z1 / z2; away from 0 the logarithms themselves are used (log1p(-q) has a pole at 1, and L1 - L2 does not cancel there)
            const double q = 2.0 * m.r / (m.s1 + m.s2) * iw / b2.z;
            const double lq = q > 0.25 ? (b1.L - b2.L) / q : (q > 0.0 ? log1p(-q) / q : -1.0);
            const double flip = fmax(0.0, ((b1.y + b2.y - b1.y * b2.y) / (b1.z * b2.z) - 2.0 * (b1.L + b2.y * lq / b2.z)) * iw2);
            const double twist = (b1.d1 + b2.d1) / (m.s1 + m.s2);
            const double al = kk * 0.5 * (twist + flip), be = kk * 0.5 * (flip - twist);
            const double inn = 1.0 / m.nn;
            const double n1 = kk * b1.d1 * is1, n2 = kk * b2.d1 * is2, h1 = kk * b1.d2, h2 = kk * b2.d2;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double u11 = u1[r] * u1[c], u22 = (w[r] * is2) * (w[c] * is2), u33 = (m.n[r] * inn) * (m.n[c] * inn);
                    S[r + 3 * c] = h1 * u11 + al * u22 + n1 * u33;
                    T[r + 3 * c] = h2 * u22 + al * u11 + n2 * u33;
                    X[r + 3 * c] = be * u1[r] * (w[c] * is2);
                }
        }
        else {
            const double den = fmax(2.0 * m.r, (m.s1 - m.s2) * (m.s1 + m.s2)); // sigma1^2 - sigma2^2 > 0: sigma1 > onset >= sigma2
            const double de = kk * b1.d1 / den, al = de * m.s1, ga = de * is1, n1 = kk * b1.d1 * is1, h1 = kk * b1.d2;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const double u11 = u1[r] * u1[c];
                    S[r + 3 * c] = (h1 - n1) * u11 + (r == c ? n1 : 0.0) + ga * w[r] * w[c];
                    T[r + 3 * c] = al * u11;
                    X[r + 3 * c] = de * u1[r] * w[c];
                }
        }
        const CsrSink sink{ v.rowBase, v.rowLen, v.ja, a, err };
#pragma unroll
        for (int l = 0; l < 3; ++l)
#pragma unroll
            for (int k = 0; k <= l; ++k) {
                if (proj[k] || proj[l]) continue;
                const double ss = sk[k] * sk[l], tt = tk[k] * tk[l], ts = tk[k] * sk[l], st = sk[k] * tk[l];
                double A[9];
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) A[r + 3 * c] = ss * S[r + 3 * c] + tt * T[r + 3 * c] + ts * X[r + 3 * c] + st * X[c + 3 * r];
                if (k == l) add_diag(sink, node[k], A);
                else add_off(sink, node[k], node[l], A);
            }
    }
}

// maximum over the workgroup, valid in lane 0 (fixed-order tree; sm: BLOCK / 64 doubles)
__device__ __forceinline__ double block_max(double x, double* sm)
{
    x = wave_max(x);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __syncthreads(); // (sm may still be read by a reduction before this one)
    if (lane == 0) sm[wv] = x;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) {
        for (int i = 0; i < BLOCK / 64; ++i) r = fmax(r, sm[i]);
    }
    return r;
}

__global__ __launch_bounds__(BLOCK) void k_shell_stretch(ShellLimitView v, double* __restrict__ sigma, double* __restrict__ partial)
{
    __shared__ double sm[BLOCK / 64];
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    double ratio = 0.0, over = 0.0;
    if (t < v.nTri) {
        Stretch m;
        stretch_state(v, t, m);
        if (sigma) {
            sigma[2 * (size_t)t] = m.s1;
            sigma[2 * (size_t)t + 1] = m.s2;
        }
        const double lim = v.triLimit ? v.triLimit[t] : 0.0;
        if (lim > 0.0) {
            ratio = m.s1 / lim;
            if (ratio != ratio) ratio = INFINITY;
            over = m.s1 < lim ? 0.0 : 1.0;
        }
    }
    const double rm = block_max(ratio, sm);
    __syncthreads();
    const double rc = block_sum<BLOCK>(over, sm);
    if (threadIdx.x == 0) {
        partial[2 * (size_t)blockIdx.x] = rm;
        partial[2 * (size_t)blockIdx.x + 1] = rc;
    }
}
__global__ __launch_bounds__(BLOCK) void k_shell_stretch_reduce(const double* __restrict__ partial, int n, double* __restrict__ out2)
{
    __shared__ double sm[BLOCK / 64];
    double mx = 0.0, cnt = 0.0;
    for (int i = threadIdx.x; i < n; i += BLOCK) {
        mx = fmax(mx, partial[2 * (size_t)i]);
        cnt += partial[2 * (size_t)i + 1];
    }
    const double rm = block_max(mx, sm);
    __syncthreads();
    const double rc = block_sum<BLOCK>(cnt, sm);
    if (threadIdx.x == 0) {
        out2[0] = rm;
        out2[1] = rc;
    }
}

} // namespace

int shell_limit_energy_blocks(const ShellLimitView& v) { return std::max(1, nblk(v.nLimited, BLOCK)); }
int shell_stretch_blocks(const ShellLimitView& v) { return std::max(1, nblk(v.nTri, BLOCK)); }

void launch_shell_limit_energy(const ShellLimitView& v, double coef, double* partial, double* out, bool accumulate, hipStream_t s)
{
    const int nb = shell_limit_energy_blocks(v);
    hipLaunchKernelGGL(k_shell_limit_energy, dim3(nb), dim3(BLOCK), 0, s, v, coef, partial);
    launch_reduce_partials(partial, nb, 1.0, accumulate, out, s);
}
void launch_shell_limit_energy_per_elem(const ShellLimitView& v, double* perTri, hipStream_t s)
{
    if (v.nTri <= 0) return;
    (void)hipMemsetAsync(perTri, 0, sizeof(double) * (size_t)v.nTri, s);
    if (v.nLimited > 0) hipLaunchKernelGGL(k_shell_limit_energy_per_elem, dim3(nblk(v.nLimited, BLOCK)), dim3(BLOCK), 0, s, v, perTri);
}
void launch_shell_limit_assemble(const ShellLimitView& v, double coef, int projectDBC, double* grad, double* a, int* err, hipStream_t s)
{
    if (v.nLimited <= 0) return;
    if (a) hipLaunchKernelGGL(k_shell_limit<true>, dim3(nblk(v.nLimited, BLOCK)), dim3(BLOCK), 0, s, v, coef, projectDBC, grad, a, err);
    else hipLaunchKernelGGL(k_shell_limit<false>, dim3(nblk(v.nLimited, BLOCK)), dim3(BLOCK), 0, s, v, coef, projectDBC, grad, a, err);
}
void launch_shell_stretch(const ShellLimitView& v, double* sigma, double* partial, double* out2, hipStream_t s)
{
    const int nb = shell_stretch_blocks(v);
    hipLaunchKernelGGL(k_shell_stretch, dim3(nb), dim3(BLOCK), 0, s, v, sigma, partial);
    hipLaunchKernelGGL(k_shell_stretch_reduce, dim3(1), dim3(BLOCK), 0, s, partial, nb, out2);
}

} // namespace ipcgpu
