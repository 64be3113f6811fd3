// Attachments: kernels (see attach_kernels.h for the energy).
//   k_attach_energy             one lane per attachment, one partial sum per block, reduced in a fixed order
//   k_attach_assemble<HESS>     one lane per attachment: up to 6 gradient 3-vectors + up to 21 upper 3 x 3 blocks (the clamp is closed form: no eigen-iteration)
//   k_attach_state              one lane per attachment: length and signed force
// All of them are small and run 256 wide; the slot loops are unrolled at compile time.  Register figures: DESIGN.md.
#include "attach_kernels.h"
#include "attach_plan.h"
#include "csr_scatter_device.h"
#include "stencil_hessian_device.h"
#include <algorithm>

namespace ipcgpu {

namespace {

using namespace scatter; // projected_dbc, ld3, CsrSink, add_diag, add_off, store_block_sum, nblk, launch_reduce_partials (csr_scatter_device.h)

constexpr int ATTACH_BLOCK = 256;
constexpr int S = ATTACH_SLOTS;

// the stencil of attachment i and d = sum c_s x_s (a slot with coefficient 0 is padding: not loaded)
struct Stencil {
    int node[S];
    double c[S];
    double d[3];
    double k, L;
};
__device__ __forceinline__ void load_stencil(const AttachView& v, int i, Stencil& st)
{
    const size_t n = (size_t)v.n;
    st.k = v.kL[i];
    st.L = v.kL[n + i];
    st.d[0] = st.d[1] = st.d[2] = 0.0;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        st.node[s] = v.node[s * n + i];
        st.c[s] = v.coef[s * n + i];
        if (st.c[s] != 0.0) {
            double x[3];
            ld3(v.x, st.node[s], x);
#pragma unroll
            for (int a = 0; a < 3; ++a) st.d[a] += st.c[s] * x[a];
        }
    }
}

__device__ __forceinline__ double attach_energy(const Stencil& st)
{
    const double d2 = sh::dot(st.d, st.d);
    if (st.L == 0.0) return 0.5 * st.k * d2; // a stitch: no square root
    const double dl = sqrt(d2) - st.L;
    return 0.5 * st.k * dl * dl;
}

__global__ __launch_bounds__(ATTACH_BLOCK) void k_attach_energy(AttachView v, double coef, double* __restrict__ partial)
{
    const int i = blockIdx.x * ATTACH_BLOCK + threadIdx.x;
    double e = 0.0;
    if (i < v.n) {
        Stencil st;
        load_stencil(v, i, st);
        e = coef * attach_energy(st);
    }
    store_block_sum<ATTACH_BLOCK>(e, partial);
}
__global__ __launch_bounds__(ATTACH_BLOCK) void k_attach_energy_per_elem(AttachView v, double* __restrict__ perAttach)
{
    const int i = blockIdx.x * ATTACH_BLOCK + threadIdx.x;
    if (i >= v.n) return;
    Stencil st;
    load_stencil(v, i, st);
    perAttach[i] = attach_energy(st);
}
__global__ __launch_bounds__(ATTACH_BLOCK) void k_attach_state(AttachView v, double* __restrict__ length, double* __restrict__ force)
{
    const int i = blockIdx.x * ATTACH_BLOCK + threadIdx.x;
    if (i >= v.n) return;
    Stencil st;
    load_stencil(v, i, st);
    const double l = sqrt(sh::dot(st.d, st.d));
    if (length) length[i] = l;
    if (force) force[i] = st.k * (l - st.L);
}

template <bool HESS>
__global__ __launch_bounds__(ATTACH_BLOCK) void k_attach_assemble(AttachView v, double coef, int projectDBC, double* __restrict__ grad, double* __restrict__ a,
    int* __restrict__ err)
{
    const int i = blockIdx.x * ATTACH_BLOCK + threadIdx.x;
    if (i >= v.n) return;
    Stencil st;
    load_stencil(v, i, st);
    const double ks = coef * st.k;
    // f: grad_s = c_s f;  B = kt t t^T + kc I
    double f[3], t[3] = { 0.0, 0.0, 0.0 }, kt = 0.0, kc = ks;
    if (st.L == 0.0) { // a stitch: grad_s = k c_s d, B = k I
#pragma unroll
        for (int r = 0; r < 3; ++r) f[r] = ks * st.d[r];
    }
    else {
        const double l = sqrt(sh::dot(st.d, st.d));
        if (!(l > 0.0)) return; // the two points coincide: no direction, hence no force and no block
        const double il = 1.0 / l, fl = ks * (l - st.L);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            t[r] = st.d[r] * il;
            f[r] = fl * t[r];
        }
        const double c = fmax(0.0, 1.0 - st.L * il); // the eigenvalue clamp in closed form
        kt = ks * (1.0 - c);
        kc = ks * c;
    }
    bool live[S]; // a slot that writes: a real node (coefficient != 0) that is not a projected Dirichlet node
#pragma unroll
    for (int s = 0; s < S; ++s) live[s] = st.c[s] != 0.0 && !projected_dbc(v.dbc[st.node[s]], projectDBC);
    if (grad) {
#pragma unroll
        for (int s = 0; s < S; ++s)
            if (live[s]) {
#pragma unroll
                for (int r = 0; r < 3; ++r) atomicAdd(&grad[3 * (size_t)st.node[s] + r], st.c[s] * f[r]);
            }
    }
    if constexpr (HESS) {
        double B[9];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int q = 0; q < 3; ++q) B[r + 3 * q] = kt * t[r] * t[q] + (r == q ? kc : 0.0);
        const CsrSink sink{ v.rowBase, v.rowLen, v.ja, a, err };
#pragma unroll
        for (int p = 0; p < S; ++p)
#pragma unroll
            for (int q = p; q < S; ++q) {
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

} // namespace

int attach_energy_blocks(const AttachView& v) { return std::max(1, nblk(v.n, ATTACH_BLOCK)); }

void launch_attach_energy(const AttachView& v, double coef, double* partial, double* out, bool accumulate, hipStream_t s)
{
    const int nb = attach_energy_blocks(v);
    hipLaunchKernelGGL(k_attach_energy, dim3(nb), dim3(ATTACH_BLOCK), 0, s, v, coef, partial);
    launch_reduce_partials(partial, nb, 1.0, accumulate, out, s);
}
void launch_attach_energy_per_elem(const AttachView& v, double* perAttach, hipStream_t s)
{
    if (v.n <= 0 || !perAttach) return;
    hipLaunchKernelGGL(k_attach_energy_per_elem, dim3(nblk(v.n, ATTACH_BLOCK)), dim3(ATTACH_BLOCK), 0, s, v, perAttach);
}
void launch_attach_assemble(const AttachView& v, double coef, int projectDBC, double* grad, double* a, int* err, hipStream_t s)
{
    if (v.n <= 0) return;
    if (a) hipLaunchKernelGGL(k_attach_assemble<true>, dim3(nblk(v.n, ATTACH_BLOCK)), dim3(ATTACH_BLOCK), 0, s, v, coef, projectDBC, grad, a, err);
    else hipLaunchKernelGGL(k_attach_assemble<false>, dim3(nblk(v.n, ATTACH_BLOCK)), dim3(ATTACH_BLOCK), 0, s, v, coef, projectDBC, grad, a, err);
}
void launch_attach_state(const AttachView& v, double* length, double* force, hipStream_t s)
{
    if (v.n <= 0 || (!length && !force)) return;
    hipLaunchKernelGGL(k_attach_state, dim3(nblk(v.n, ATTACH_BLOCK)), dim3(ATTACH_BLOCK), 0, s, v, length, force);
}

} // namespace ipcgpu
