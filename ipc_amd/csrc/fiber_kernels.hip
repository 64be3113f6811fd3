// Fibre reinforcement of tetrahedral elements: kernels (see fiber_kernels.h for the energy).
//   k_fiber_energy             one lane per fibred element, one partial sum per block, reduced in a fixed order
//   k_fiber_energy_per_elem    one lane per fibred element
//   k_fiber_assemble<HESS>     one lane per fibred element: 4 gradient 3-vectors + 10 upper 3 x 3 blocks (the clamp is closed form: no eigen-iteration)
//   k_fiber_state              one lane per fibred element: l, tension, t; min l / max l / sum W per block, then one workgroup over the blocks
// All of them run 256 wide; the node loops are unrolled at compile time.  Timings: DESIGN.md section 0 (tools/bench_fiber.py).
#include "fiber_kernels.h"
#include "csr_scatter_device.h"
#include <algorithm>
#include <cmath>

namespace ipcgpu {

namespace {

using namespace scatter; // projected_dbc, ld3, CsrSink, add_diag, add_off, store_block_sum, nblk, launch_reduce_partials (csr_scatter_device.h)

constexpr int FIBER_BLOCK = 256;

// element i of the compact list: its nodes, c and d = sum c_s x_s
struct Stencil {
    int node[4];
    double c[4];
    double d[3];
    double vk, k2, l0;
    int flags;
};
__device__ __forceinline__ void load_stencil(const FiberView& v, int i, Stencil& st)
{
    const size_t n = (size_t)v.nF;
    const int4 tt = v.tet[v.fibTet[i]];
    st.node[0] = tt.x;
    st.node[1] = tt.y;
    st.node[2] = tt.z;
    st.node[3] = tt.w;
    st.c[1] = v.b[i];
    st.c[2] = v.b[n + i];
    st.c[3] = v.b[2 * n + i];
    st.c[0] = -(st.c[1] + st.c[2] + st.c[3]);
    st.vk = v.volK[i];
    st.k2 = v.k2[i];
    st.flags = v.flags[i];
    st.l0 = v.l0[v.groupOf[i]];
    double x0[3];
    ld3(v.x, st.node[0], x0);
    st.d[0] = st.d[1] = st.d[2] = 0.0;
#pragma unroll
    for (int s = 1; s < 4; ++s) {
        double x[3];
        ld3(v.x, st.node[s], x);
#pragma unroll
        for (int a = 0; a < 3; ++a) st.d[a] += st.c[s] * (x[a] - x0[a]); // (translation drops out exactly)
    }
}
__device__ __forceinline__ double stretch(const Stencil& st) { return sqrt(st.d[0] * st.d[0] + st.d[1] * st.d[1] + st.d[2] * st.d[2]); }

// W = vol psi(l), d1 = vol psi'(l), d2 = vol psi''(l).  All three are 0 where the law is switched off (compression of a tension-only or exp fibre).
template <bool DERIV>
__device__ __forceinline__ void fiber_law(const Stencil& st, double l, double& W, double& d1, double& d2)
{
    W = d1 = d2 = 0.0;
    if (st.flags & FIBER_FLAG_EXP) {
        if (!(l > 1.0)) return;
        const double I = l * l - 1.0, q = st.k2 * I * I;
        W = st.vk / (2.0 * st.k2) * expm1(q); // +inf where q overflows
        if constexpr (DERIV) {
            const double e = exp(q);
            d1 = st.vk * (2.0 * l * I) * e;
            d2 = st.vk * e * (2.0 * I + 4.0 * l * l + 8.0 * q * l * l);
        }
    }
    else {
        const double dl = l - st.l0;
        if ((st.flags & FIBER_FLAG_TENSION_ONLY) && !(dl > 0.0)) return;
        W = 0.5 * st.vk * dl * dl;
        if constexpr (DERIV) {
            d1 = st.vk * dl;
            d2 = st.vk;
        }
    }
}

__global__ __launch_bounds__(FIBER_BLOCK) void k_fiber_energy(FiberView v, double coef, double* __restrict__ partial)
{
    const int i = blockIdx.x * FIBER_BLOCK + threadIdx.x;
    double e = 0.0;
    if (i < v.nF) {
        Stencil st;
        load_stencil(v, i, st);
        double W, d1, d2;
        fiber_law<false>(st, stretch(st), W, d1, d2);
        e = coef * W;
    }
    store_block_sum<FIBER_BLOCK>(e, partial);
}
__global__ __launch_bounds__(FIBER_BLOCK) void k_fiber_energy_per_elem(FiberView v, double* __restrict__ perFiber)
{
    const int i = blockIdx.x * FIBER_BLOCK + threadIdx.x;
    if (i >= v.nF) return;
    Stencil st;
    load_stencil(v, i, st);
    double W, d1, d2;
    fiber_law<false>(st, stretch(st), W, d1, d2);
    perFiber[i] = W;
}

template <bool HESS>
__global__ __launch_bounds__(FIBER_BLOCK) void k_fiber_assemble(FiberView v, double coef, int projectDBC, double* __restrict__ grad, double* __restrict__ a,
    int* __restrict__ err)
{
    const int i = blockIdx.x * FIBER_BLOCK + threadIdx.x;
    if (i >= v.nF) return;
    Stencil st;
    load_stencil(v, i, st);
    const double l = stretch(st);
    if (!(l > 0.0)) return; // no direction: no force and no block
    double W, d1, d2;
    fiber_law<true>(st, l, W, d1, d2);
    if (d1 == 0.0 && d2 == 0.0) return; // the law is off here: no atomic at all
    if (!(fabs(d1) < INFINITY) || !(fabs(d2) < INFINITY)) return; // past the fp64 range (the energy is +inf there): nothing rather than NaN
    const double il = 1.0 / l;
    double t[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) t[r] = st.d[r] * il;
    bool live[4]; // a node that writes: c != 0 and not a projected Dirichlet node
#pragma unroll
    for (int s = 0; s < 4; ++s) live[s] = st.c[s] != 0.0 && !projected_dbc(v.dbc[st.node[s]], projectDBC);
    if (grad) {
        const double f = coef * d1;
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (live[s]) {
#pragma unroll
                for (int r = 0; r < 3; ++r) atomicAdd(&grad[3 * (size_t)st.node[s] + r], st.c[s] * (f * t[r]));
            }
    }
    if constexpr (HESS) {
        // B = kt t t^T + kc I: the two eigenvalue clamps in closed form
        const double kc = coef * fmax(0.0, d1 * il), kt = coef * fmax(0.0, d2) - kc;
        double B[9];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int q = 0; q < 3; ++q) B[r + 3 * q] = kt * t[r] * t[q] + (r == q ? kc : 0.0);
        const CsrSink sink{ v.rowBase, v.rowLen, v.ja, a, err };
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = p; q < 4; ++q) {
                if (!live[p] || !live[q]) continue;
                const double cc = st.c[p] * st.c[q];
                double A[9];
#pragma unroll
                for (int e = 0; e < 9; ++e) A[e] = cc * B[e];
                if (p == q) add_diag(sink, st.node[p], A);
                else add_off(sink, st.node[p], st.node[q], A);
            }
    }
}

// partial: [3][gridDim.x] -- min l, max l, sum W of the block; lanes past nF carry the identities
__global__ __launch_bounds__(FIBER_BLOCK) void k_fiber_state(FiberView v, const double* __restrict__ vol, double* __restrict__ perFiber, double* __restrict__ partial)
{
    __shared__ double sm[3][FIBER_BLOCK / 64];
    const int i = blockIdx.x * FIBER_BLOCK + threadIdx.x;
    double lo = INFINITY, hi = -INFINITY, W = 0.0;
    if (i < v.nF) {
        Stencil st;
        load_stencil(v, i, st);
        const double l = stretch(st);
        double d1, d2;
        fiber_law<true>(st, l, W, d1, d2);
        lo = hi = l;
        if (perFiber) {
            const size_t n = (size_t)v.nF;
            const double il = l > 0.0 ? 1.0 / l : 0.0;
            perFiber[i] = l;
            perFiber[n + i] = d1 / vol[v.fibTet[i]];
#pragma unroll
            for (int r = 0; r < 3; ++r) perFiber[(2 + r) * n + i] = st.d[r] * il;
        }
    }
    if (!partial) return;
    lo = prims::wave_min(lo);
    hi = wave_max(hi);
    W = wave_sum(W);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) {
        sm[0][wv] = lo;
        sm[1][wv] = hi;
        sm[2][wv] = W;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < FIBER_BLOCK / 64; ++w) { // the waves in index order
            lo = fmin(lo, sm[0][w]);
            hi = fmax(hi, sm[1][w]);
            W += sm[2][w];
        }
        partial[blockIdx.x] = lo;
        partial[gridDim.x + blockIdx.x] = hi;
        partial[2 * gridDim.x + blockIdx.x] = W;
    }
}
// one workgroup: lane j takes blocks j, j + FIBER_BLOCK, ... in index order, then the tree of k_fiber_state
__global__ __launch_bounds__(FIBER_BLOCK) void k_fiber_state_totals(const double* __restrict__ partial, int nb, double* __restrict__ totals3)
{
    __shared__ double sm[3][FIBER_BLOCK / 64];
    double lo = INFINITY, hi = -INFINITY, W = 0.0;
    for (int j = threadIdx.x; j < nb; j += FIBER_BLOCK) {
        lo = fmin(lo, partial[j]);
        hi = fmax(hi, partial[nb + j]);
        W += partial[2 * nb + j];
    }
    lo = prims::wave_min(lo);
    hi = wave_max(hi);
    W = wave_sum(W);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) {
        sm[0][wv] = lo;
        sm[1][wv] = hi;
        sm[2][wv] = W;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < FIBER_BLOCK / 64; ++w) {
            lo = fmin(lo, sm[0][w]);
            hi = fmax(hi, sm[1][w]);
            W += sm[2][w];
        }
        totals3[0] = lo;
        totals3[1] = hi;
        totals3[2] = W;
    }
}

} // namespace

int fiber_energy_blocks(const FiberView& v) { return std::max(1, nblk(v.nF, FIBER_BLOCK)); }

void launch_fiber_energy(const FiberView& v, double coef, double* partial, double* out, bool accumulate, hipStream_t s)
{
    const int nb = fiber_energy_blocks(v);
    hipLaunchKernelGGL(k_fiber_energy, dim3(nb), dim3(FIBER_BLOCK), 0, s, v, coef, partial);
    launch_reduce_partials(partial, nb, 1.0, accumulate, out, s);
}
void launch_fiber_energy_per_elem(const FiberView& v, double* perFiber, hipStream_t s)
{
    if (v.nF <= 0 || !perFiber) return;
    hipLaunchKernelGGL(k_fiber_energy_per_elem, dim3(nblk(v.nF, FIBER_BLOCK)), dim3(FIBER_BLOCK), 0, s, v, perFiber);
}
void launch_fiber_assemble(const FiberView& v, double coef, int projectDBC, double* grad, double* a, int* err, hipStream_t s)
{
    if (v.nF <= 0) return;
    if (a) hipLaunchKernelGGL(k_fiber_assemble<true>, dim3(nblk(v.nF, FIBER_BLOCK)), dim3(FIBER_BLOCK), 0, s, v, coef, projectDBC, grad, a, err);
    else hipLaunchKernelGGL(k_fiber_assemble<false>, dim3(nblk(v.nF, FIBER_BLOCK)), dim3(FIBER_BLOCK), 0, s, v, coef, projectDBC, grad, a, err);
}
void launch_fiber_state(const FiberView& v, const double* vol, double* perFiber, double* partial, double* totals3, hipStream_t s)
{
    if (v.nF <= 0 || (!perFiber && !totals3)) return;
    const int nb = fiber_energy_blocks(v);
    hipLaunchKernelGGL(k_fiber_state, dim3(nb), dim3(FIBER_BLOCK), 0, s, v, vol, perFiber, totals3 ? partial : nullptr);
    if (totals3) hipLaunchKernelGGL(k_fiber_state_totals, dim3(1), dim3(FIBER_BLOCK), 0, s, (const double*)partial, nb, totals3);
}

} // namespace ipcgpu
