// Plastic flow of tetrahedral bodies: kernels (see plastic_kernels.h for the model).
//   k_plastic_flow      one lane per tetrahedron of [tetBegin, tetEnd): A_t <- A_t G and alpha_t += Delta where the element yields, two integer counters
//   k_plastic_state     one lane per tetrahedron, read-only: n, y, alpha; per workgroup max alpha and sum vol alpha
//   k_plastic_totals    one workgroup: the partials of k_plastic_state in index order
// Compiled without contraction into fused multiply-adds (build.py): tests/plastic_mp.py restates the arithmetic in plain doubles.
#include "plastic_kernels.h"
#include "nh_device.h"
#include "scalar_slots.h"
#include <algorithm>

namespace ipcgpu {

namespace {

using prims::block_sum;
using prims::nblk;
using prims::wave_max;

constexpr int PLASTIC_BLOCK = 256;

// the elastic strain measure of element t at v.x: A_t, V of F = U diag(s) V^T, the deviatoric logarithmic stretches d and their norm n.
// false: s2 <= 0 (or not a number) -- the element has no logarithmic strain
__device__ __forceinline__ bool hencky(const PlasticView& v, int t, double A[9], double V[9], double d[3], double& n)
{
    const size_t nT = (size_t)v.nT;
#pragma unroll
    for (int k = 0; k < 9; ++k) A[k] = v.A[k * nT + t];
    const int4 tv = v.tet[t];
    double F[9], U[9], s[3];
    dev::deformation_gradient(dev::ld3(v.x, tv.x), dev::ld3(v.x, tv.y), dev::ld3(v.x, tv.z), dev::ld3(v.x, tv.w), A, F);
    dev::svd3(F, U, s, V);
    if (!(s[2] > 0.0)) return false;
    const double e0 = log(s[0]), e1 = log(s[1]), e2 = log(s[2]);
    const double m = ((e0 + e1) + e2) / 3.0;
    d[0] = e0 - m;
    d[1] = e1 - m;
    d[2] = e2 - m;
    n = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    return true;
}

// what one lane of k_plastic_flow did with its element
enum { FLOW_NONE = 0, FLOW_YIELDED = 1, FLOW_SKIPPED = 2 };

__device__ __forceinline__ int flow_element(const PlasticView& v, int t)
{
    const double y0 = v.yield[t];
    if (!(y0 < INFINITY)) return FLOW_NONE; // plasticity off
    const double creep = v.creep[t], K = v.harden[t], al = v.alpha[t];
    double A[9], V[9], d[3], n;
    if (!hencky(v, t, A, V, d, n)) return FLOW_SKIPPED;
    const double y = y0 + K * al;
    if (!(n > y)) return FLOW_NONE; // elastic (n = 0 included, whatever y is): not a bit is written
    const double r = -expm1(-creep * v.dt); // 1 at creep = +inf
    const double Delta = r * (n - y) / (1.0 + K);
    const double q = -Delta / n;
    const double g[3] = { exp(q * d[0]), exp(q * d[1]), exp(q * d[2]) };
    // G = V diag(g) V^T (column j of V is V[3 j ..]), symmetric: six entries
    double G[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) G[a + 3 * b] = G[b + 3 * a] = (V[a] * g[0] * V[b] + V[3 + a] * g[1] * V[3 + b]) + V[6 + a] * g[2] * V[6 + b];
    const size_t nT = (size_t)v.nT;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i) v.A[(size_t)(i + 3 * j) * nT + t] = (A[i] * G[3 * j] + A[i + 3] * G[1 + 3 * j]) + A[i + 6] * G[2 + 3 * j];
    v.alpha[t] = al + Delta;
    return FLOW_YIELDED;
}

// The counters: every lane atomically adding to ONE address serialises (1.5 ms for 133 206 yielding elements); so each wave counts its lanes by ballot,
// the workgroup adds its four waves in LDS, and one lane per workgroup adds to device memory -- and only a number that is not zero.
__global__ __launch_bounds__(PLASTIC_BLOCK) void k_plastic_flow(PlasticView v, int* __restrict__ counts)
{
    __shared__ int sm[PC_COUNT];
    if (threadIdx.x < PC_COUNT) sm[threadIdx.x] = 0;
    __syncthreads();
    const int t = v.tetBegin + blockIdx.x * PLASTIC_BLOCK + threadIdx.x;
    const int what = t < v.tetEnd ? flow_element(v, t) : FLOW_NONE;
    const unsigned long long my = __ballot(what == FLOW_YIELDED), ms = __ballot(what == FLOW_SKIPPED);
    if ((threadIdx.x & 63) == 0) {
        if (my) atomicAdd(&sm[PC_YIELDED], __popcll(my));
        if (ms) atomicAdd(&sm[PC_SKIPPED], __popcll(ms));
    }
    __syncthreads();
    if (threadIdx.x < PC_COUNT && sm[threadIdx.x]) atomicAdd(&counts[threadIdx.x], sm[threadIdx.x]);
}

__global__ __launch_bounds__(PLASTIC_BLOCK) void k_plastic_state(PlasticView v, double* __restrict__ perElem, double* __restrict__ partial)
{
    __shared__ double smSum[PLASTIC_BLOCK / 64], smMax[PLASTIC_BLOCK / 64];
    const int t = blockIdx.x * PLASTIC_BLOCK + threadIdx.x;
    double al = 0.0, va = 0.0;
    if (t < v.nT) {
        al = v.alpha[t];
        va = v.vol[t] * al;
        if (perElem) {
            double A[9], V[9], d[3], n;
            if (!hencky(v, t, A, V, d, n)) n = NAN;
            const size_t nT = (size_t)v.nT;
            perElem[t] = n;
            perElem[nT + t] = v.yield[t] + v.harden[t] * al;
            perElem[2 * nT + t] = al;
        }
    }
    if (!partial) return;
    const double mx = wave_max(al);
    if ((threadIdx.x & 63) == 0) smMax[threadIdx.x >> 6] = mx;
    const double sum = block_sum<PLASTIC_BLOCK>(va, smSum); // (its barrier also publishes smMax)
    if (threadIdx.x == 0) {
        double r = smMax[0];
        for (int i = 1; i < PLASTIC_BLOCK / 64; ++i) r = fmax(r, smMax[i]);
        partial[blockIdx.x] = r;
        partial[gridDim.x + blockIdx.x] = sum;
    }
}
// totals[PT_MAX_ALPHA] = max, totals[PT_VOL_ALPHA] = sum of the nb partials: lane l takes l, l + BLOCK, ... in index order, then the workgroup tree
__global__ __launch_bounds__(PLASTIC_BLOCK) void k_plastic_totals(const double* __restrict__ partial, int nb, double* __restrict__ totals)
{
    __shared__ double smSum[PLASTIC_BLOCK / 64], smMax[PLASTIC_BLOCK / 64];
    double mx = 0.0, x = 0.0;
    for (int i = threadIdx.x; i < nb; i += PLASTIC_BLOCK) {
        mx = fmax(mx, partial[i]);
        x += partial[nb + i];
    }
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) smMax[threadIdx.x >> 6] = mx;
    const double sum = block_sum<PLASTIC_BLOCK>(x, smSum);
    if (threadIdx.x == 0) {
        double r = smMax[0];
        for (int i = 1; i < PLASTIC_BLOCK / 64; ++i) r = fmax(r, smMax[i]);
        totals[PT_MAX_ALPHA] = r;
        totals[PT_VOL_ALPHA] = sum;
    }
}

} // namespace

void launch_plastic_flow(const PlasticView& v, int* counts, hipStream_t s)
{
    if (v.tetEnd <= v.tetBegin) return;
    hipLaunchKernelGGL(k_plastic_flow, dim3(nblk(v.tetEnd - v.tetBegin, PLASTIC_BLOCK)), dim3(PLASTIC_BLOCK), 0, s, v, counts);
}
int plastic_state_blocks(const PlasticView& v) { return std::max(1, nblk(v.nT, PLASTIC_BLOCK)); }
void launch_plastic_state(const PlasticView& v, double* perElem, double* partial, double* totals2, hipStream_t s)
{
    if (v.nT <= 0 || (!perElem && !totals2)) return;
    const int nb = plastic_state_blocks(v);
    hipLaunchKernelGGL(k_plastic_state, dim3(nb), dim3(PLASTIC_BLOCK), 0, s, v, perElem, totals2 ? partial : nullptr);
    if (totals2) hipLaunchKernelGGL(k_plastic_totals, dim3(1), dim3(PLASTIC_BLOCK), 0, s, partial, nb, totals2);
}

} // namespace ipcgpu
