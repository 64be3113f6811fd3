// Plastic flow of the elastic shells: kernels (see shell_plastic_kernels.h for the model).
//   k_shell_plastic_flow_tri     one lane per triangle: B <- B G and alpha += Delta where the membrane yields, two integer counters
//   k_shell_plastic_flow_hinge   one lane per hinge: thetaBar += sign(k) Delta / g and alphaB += Delta where the hinge yields, two integer counters
//   k_shell_plastic_state        one lane per triangle or hinge, read-only: the per-record state; per workgroup max alpha, max alphaB, sum h A alpha
//   k_shell_plastic_totals       one workgroup: the partials of k_shell_plastic_state in index order
// Compiled without contraction into fused multiply-adds (build.py): tests/shell_plastic_mp.py restates the arithmetic in plain doubles.
#include "shell_plastic_kernels.h"
#include "csr_scatter_device.h"
#include "scalar_slots.h"
#include "shell_hinge_device.h"
#include <algorithm>

namespace ipcgpu {

namespace {

using scatter::block_sum;
using scatter::ld3;
using scatter::nblk;
using scatter::wave_max;

constexpr int SP_BLOCK = 256;

// the elastic strain measure of triangle t at v.x
struct TriStrain {
    double b00, b10, b01, b11; // B
    double vx, vy; // the unit eigenvector of l1; the one of l2 is (-vy, vx)
    double e1, e2; // ln(l_i) / 2
    double n; // the deviatoric Hencky norm of (e1, e2, e3)
};
// false: l2 <= 0 or something is not finite -- the triangle has no logarithmic strain
__device__ __forceinline__ bool tri_strain(const ShellPlasticView& v, int t, TriStrain& s)
{
    const size_t nTri = (size_t)v.nTri;
    s.b00 = v.triConst[t];
    s.b10 = v.triConst[nTri + t];
    s.b01 = v.triConst[2 * nTri + t];
    s.b11 = v.triConst[3 * nTri + t];
    const double hAmu = v.triConst[4 * nTri + t], hAlam = v.triConst[5 * nTri + t];
    double x0[3], x1[3], x2[3], u1[3], u2[3], w[3];
    ld3(v.x, v.tri[3 * (size_t)t], x0);
    ld3(v.x, v.tri[3 * (size_t)t + 1], x1);
    ld3(v.x, v.tri[3 * (size_t)t + 2], x2);
    double a = 0.0, b = 0.0, c = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        u1[i] = x1[i] - x0[i];
        u2[i] = x2[i] - x0[i];
        const double f1 = u1[i] * s.b00 + u2[i] * s.b10, f2 = u1[i] * s.b01 + u2[i] * s.b11;
        a += f1 * f1;
        b += f1 * f2;
        c += f2 * f2;
    }
    // C = [a b; b c].  l1 = mean + radius has no cancellation; l2 = det C / l1 with det C = |u1 x u2|^2 (det B)^2, exactly zero for edges that are
    // parallel in their doubles
    sh::cross(u1, u2, w);
    const double detB = s.b00 * s.b11 - s.b01 * s.b10;
    const double detC = sh::dot(w, w) * (detB * detB);
    double l1, l2;
    if (b == 0.0) { // diagonal already (l1 == l2 with b == 0 included: V = I serves, G is then a multiple of I)
        const bool first = a >= c;
        l1 = first ? a : c;
        l2 = first ? c : a;
        s.vx = first ? 1.0 : 0.0;
        s.vy = first ? 0.0 : 1.0;
    }
    else {
        const double h = 0.5 * (a - c), rad = sqrt(h * h + b * b); // rad >= |b| > 0: l1 > l2 here
        l1 = 0.5 * (a + c) + rad;
        l2 = detC / l1;
        // (C - l2 I) maps onto the eigenvector of l1: its better-conditioned column
        const double px = h >= 0.0 ? h + rad : b, py = h >= 0.0 ? b : rad - h;
        const double inv = 1.0 / sqrt(px * px + py * py);
        s.vx = px * inv;
        s.vy = py * inv;
    }
    if (!(l2 > 0.0) || !(l1 < INFINITY)) return false;
    s.e1 = 0.5 * log(l1);
    s.e2 = 0.5 * log(l2);
    const double cc = hAlam / (2.0 * hAmu);
    const double e3 = -cc * (s.e1 + s.e2);
    const double m = ((s.e1 + s.e2) + e3) / 3.0;
    const double d1 = s.e1 - m, d2 = s.e2 - m, d3 = e3 - m;
    s.n = sqrt((d1 * d1 + d2 * d2) + d3 * d3);
    return s.n < INFINITY; // (false for NaN as well)
}

// what one lane of a flow kernel did with its record
enum { FLOW_NONE = 0, FLOW_YIELDED = 1, FLOW_SKIPPED = 2 };

__device__ __forceinline__ int flow_triangle(const ShellPlasticView& v, int t)
{
    const double y0 = v.yield[t];
    if (!(y0 < INFINITY)) return FLOW_NONE; // membrane flow off
    const double creep = v.creep[t], K = v.harden[t], al = v.alpha[t];
    TriStrain s;
    if (!tri_strain(v, t, s)) return FLOW_SKIPPED;
    const double y = y0 + K * al;
    if (!(s.n > y)) return FLOW_NONE; // elastic (n = 0 included, whatever y is): not a bit is written
    const double r = -expm1(-creep * v.dt); // 1 at creep = +inf
    const double Delta = r * (s.n - y) / (1.0 + K);
    const double f = -Delta / s.n;
    const double g1 = exp(f * s.e1), g2 = exp(f * s.e2);
    // G = V diag(g1, g2) V^T, V = [vx -vy; vy vx]
    const double G11 = g1 * s.vx * s.vx + g2 * s.vy * s.vy;
    const double G12 = (g1 - g2) * s.vx * s.vy;
    const double G22 = g1 * s.vy * s.vy + g2 * s.vx * s.vx;
    const size_t nTri = (size_t)v.nTri;
    v.triConst[t] = s.b00 * G11 + s.b01 * G12;
    v.triConst[nTri + t] = s.b10 * G11 + s.b11 * G12;
    v.triConst[2 * nTri + t] = s.b00 * G12 + s.b01 * G22;
    v.triConst[3 * nTri + t] = s.b10 * G12 + s.b11 * G22;
    v.alpha[t] = al + Delta;
    return FLOW_YIELDED;
}

// theta of hinge i at v.x; false: a zero-length n1, n2 or e, or something not finite
__device__ __forceinline__ bool hinge_theta(const ShellPlasticView& v, int i, double& theta)
{
    const int4 nd = v.hinge[i];
    double x0[3], x1[3], x2[3], x3[3], e[3], a[3], b[3], c[3], n1[3], n2[3];
    ld3(v.x, nd.x, x0);
    ld3(v.x, nd.y, x1);
    ld3(v.x, nd.z, x2);
    ld3(v.x, nd.w, x3);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        e[k] = x1[k] - x0[k];
        a[k] = x2[k] - x0[k];
        b[k] = x0[k] - x1[k];
        c[k] = x3[k] - x1[k];
    }
    sh::cross(e, a, n1);
    sh::cross(b, c, n2);
    const double ee = sh::dot(e, e), n11 = sh::dot(n1, n1), n22 = sh::dot(n2, n2);
    if (!(ee > 0.0 && n11 > 0.0 && n22 > 0.0) || !(ee < INFINITY && n11 < INFINITY && n22 < INFINITY)) return false;
    theta = hinge_angle<false>(x0, x1, x2, x3, nullptr);
    return fabs(theta) < INFINITY;
}

__device__ __forceinline__ int flow_hinge(const ShellPlasticView& v, int i)
{
    const double y0 = v.hYield[i];
    if (!(y0 < INFINITY)) return FLOW_NONE; // one of its triangles has no bendYield
    const double creep = v.hCreep[i], K = v.hHarden[i], g = v.hG[i], al = v.alphaB[i], thetaBar = v.hingeConst[i];
    double theta;
    if (!hinge_theta(v, i, theta)) return FLOW_SKIPPED;
    const double k = theta - thetaBar;
    const double eps = g * fabs(k);
    const double y = y0 + K * al;
    if (!(eps > y)) return FLOW_NONE;
    const double r = -expm1(-creep * v.dt);
    const double Delta = r * (eps - y) / (1.0 + K);
    v.hingeConst[i] = thetaBar + copysign(Delta / g, k);
    v.alphaB[i] = al + Delta;
    return FLOW_YIELDED;
}

// the two counters of a flow kernel, at counts[first] and counts[first + 1]: a ballot per wave, the waves of the workgroup in LDS, one add per workgroup
__device__ __forceinline__ void count_flow(int what, int* __restrict__ counts, int first)
{
    __shared__ int sm[2];
    if (threadIdx.x < 2) sm[threadIdx.x] = 0;
    __syncthreads();
    const unsigned long long my = __ballot(what == FLOW_YIELDED), ms = __ballot(what == FLOW_SKIPPED);
    if ((threadIdx.x & 63) == 0) {
        if (my) atomicAdd(&sm[0], __popcll(my));
        if (ms) atomicAdd(&sm[1], __popcll(ms));
    }
    __syncthreads();
    if (threadIdx.x < 2 && sm[threadIdx.x]) atomicAdd(&counts[first + threadIdx.x], sm[threadIdx.x]);
}

__global__ __launch_bounds__(SP_BLOCK) void k_shell_plastic_flow_tri(ShellPlasticView v, int* __restrict__ counts)
{
    const int t = blockIdx.x * SP_BLOCK + threadIdx.x;
    count_flow(t < v.nTri ? flow_triangle(v, t) : FLOW_NONE, counts, SPC_TRI_YIELDED);
}
__global__ __launch_bounds__(SP_BLOCK) void k_shell_plastic_flow_hinge(ShellPlasticView v, int* __restrict__ counts)
{
    const int i = blockIdx.x * SP_BLOCK + threadIdx.x;
    count_flow(i < v.nHinge ? flow_hinge(v, i) : FLOW_NONE, counts, SPC_HINGE_YIELDED);
}

// lanes [0, nTri) take the triangles, lanes [nTri, nTri + nHinge) the hinges; partial: [SPT_COUNT][gridDim.x]
__global__ __launch_bounds__(SP_BLOCK) void k_shell_plastic_state(ShellPlasticView v, double* __restrict__ perTri, double* __restrict__ perHinge, double* __restrict__ partial)
{
    __shared__ double smSum[SP_BLOCK / 64], smMaxA[SP_BLOCK / 64], smMaxB[SP_BLOCK / 64];
    const int gid = blockIdx.x * SP_BLOCK + threadIdx.x;
    double al = 0.0, alB = 0.0, va = 0.0;
    if (gid < v.nTri) {
        const int t = gid;
        al = v.alpha[t];
        va = v.hA[t] * al;
        if (perTri) {
            const size_t nTri = (size_t)v.nTri;
            TriStrain s;
            if (!tri_strain(v, t, s)) s.n = NAN;
            perTri[t] = s.n;
            perTri[nTri + t] = v.yield[t] + v.harden[t] * al;
            perTri[2 * nTri + t] = al;
            const double det0 = v.B0[t] * v.B0[3 * nTri + t] - v.B0[2 * nTri + t] * v.B0[nTri + t];
            perTri[3 * nTri + t] = det0 / (s.b00 * s.b11 - s.b01 * s.b10);
        }
    }
    else if (gid - v.nTri < v.nHinge) {
        const int i = gid - v.nTri;
        alB = v.alphaB[i];
        if (perHinge) {
            const size_t nH = (size_t)v.nHinge;
            const double thetaBar = v.hingeConst[i];
            double theta;
            perHinge[i] = hinge_theta(v, i, theta) ? v.hG[i] * fabs(theta - thetaBar) : NAN;
            perHinge[nH + i] = v.hYield[i] + v.hHarden[i] * alB;
            perHinge[2 * nH + i] = alB;
            perHinge[3 * nH + i] = thetaBar - v.thetaBar0[i];
        }
    }
    if (!partial) return;
    const double mxA = wave_max(al), mxB = wave_max(alB);
    if ((threadIdx.x & 63) == 0) {
        smMaxA[threadIdx.x >> 6] = mxA;
        smMaxB[threadIdx.x >> 6] = mxB;
    }
    const double sum = block_sum<SP_BLOCK>(va, smSum); // (its barrier also publishes the two maxima)
    if (threadIdx.x == 0) {
        double ra = smMaxA[0], rb = smMaxB[0];
        for (int w = 1; w < SP_BLOCK / 64; ++w) {
            ra = fmax(ra, smMaxA[w]);
            rb = fmax(rb, smMaxB[w]);
        }
        partial[(size_t)SPT_MAX_ALPHA * gridDim.x + blockIdx.x] = ra;
        partial[(size_t)SPT_MAX_ALPHA_B * gridDim.x + blockIdx.x] = rb;
        partial[(size_t)SPT_HA_ALPHA * gridDim.x + blockIdx.x] = sum;
    }
}
// the nb partials per quantity: lane l takes l, l + BLOCK, ... in index order, then the workgroup tree
__global__ __launch_bounds__(SP_BLOCK) void k_shell_plastic_totals(const double* __restrict__ partial, int nb, double* __restrict__ totals)
{
    __shared__ double smSum[SP_BLOCK / 64], smMaxA[SP_BLOCK / 64], smMaxB[SP_BLOCK / 64];
    double ma = 0.0, mb = 0.0, x = 0.0;
    for (int i = threadIdx.x; i < nb; i += SP_BLOCK) {
        ma = fmax(ma, partial[(size_t)SPT_MAX_ALPHA * nb + i]);
        mb = fmax(mb, partial[(size_t)SPT_MAX_ALPHA_B * nb + i]);
        x += partial[(size_t)SPT_HA_ALPHA * nb + i];
    }
    ma = wave_max(ma);
    mb = wave_max(mb);
    if ((threadIdx.x & 63) == 0) {
        smMaxA[threadIdx.x >> 6] = ma;
        smMaxB[threadIdx.x >> 6] = mb;
    }
    const double sum = block_sum<SP_BLOCK>(x, smSum);
    if (threadIdx.x == 0) {
        double ra = smMaxA[0], rb = smMaxB[0];
        for (int w = 1; w < SP_BLOCK / 64; ++w) {
            ra = fmax(ra, smMaxA[w]);
            rb = fmax(rb, smMaxB[w]);
        }
        totals[SPT_MAX_ALPHA] = ra;
        totals[SPT_MAX_ALPHA_B] = rb;
        totals[SPT_HA_ALPHA] = sum;
    }
}

} // namespace

void launch_shell_plastic_flow(const ShellPlasticView& v, bool tris, bool hinges, int* counts, hipStream_t s)
{
    if (tris && v.nTri > 0) hipLaunchKernelGGL(k_shell_plastic_flow_tri, dim3(nblk(v.nTri, SP_BLOCK)), dim3(SP_BLOCK), 0, s, v, counts);
    if (hinges && v.nHinge > 0) hipLaunchKernelGGL(k_shell_plastic_flow_hinge, dim3(nblk(v.nHinge, SP_BLOCK)), dim3(SP_BLOCK), 0, s, v, counts);
}
int shell_plastic_state_blocks(const ShellPlasticView& v) { return std::max(1, nblk((long long)v.nTri + v.nHinge, SP_BLOCK)); }
void launch_shell_plastic_state(const ShellPlasticView& v, double* perTri, double* perHinge, double* partial, double* totals3, hipStream_t s)
{
    if (v.nTri <= 0 || (!perTri && !perHinge && !totals3)) return;
    const int nb = shell_plastic_state_blocks(v);
    hipLaunchKernelGGL(k_shell_plastic_state, dim3(nb), dim3(SP_BLOCK), 0, s, v, perTri, perHinge, totals3 ? partial : nullptr);
    if (totals3) hipLaunchKernelGGL(k_shell_plastic_totals, dim3(1), dim3(SP_BLOCK), 0, s, partial, nb, totals3);
}

} // namespace ipcgpu
