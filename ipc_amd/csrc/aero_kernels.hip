// Wind and air drag: kernels (see aero_kernels.h for the model).
//   k_aero_refresh            one lane per triangle: the lagged record (n, A, c^n, pad) from given positions, four 16-byte stores
//   k_aero_energy             one lane per triangle, one partial sum per block, reduced in a fixed order
//   k_aero_assemble<HESS>     one lane per triangle: one gradient 3-vector for the three nodes; with HESS the six distinct entries of K / 9, into 3 diagonal
//                             and 3 upper off-diagonal blocks
//   k_aero_state              one lane per triangle: its force; five partial sums per block, k_aero_state_sum adds them in index order
// Register figures: DESIGN.md.
#include "aero_kernels.h"
#include "csr_scatter_device.h"
#include "stencil_hessian_device.h"
#include <algorithm>

namespace ipcgpu {

namespace {

using namespace scatter; // projected_dbc, ld3, CsrSink, add_diag, add_off, block_sum, store_block_sum, nblk, launch_reduce_partials (csr_scatter_device.h)

constexpr int AERO_BLOCK = 256;
constexpr int AERO_STATE_Q = 5; // sums of k_aero_state: force (3), power, loaded area

__device__ __forceinline__ void centroid(const double* x0, const double* x1, const double* x2, double* c)
{
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = ((x0[a] + x1[a]) + x2[a]) / 3.0;
}

// what every evaluation of triangle t needs: its nodes, a = rho_a A / 6, the lagged normal, the flow u against the air split into s_n and u_t, Cn and Ct
struct Flow {
    int node[3];
    double a, n[3], u[3], un, sn, ut[3], lt, cn, ct;
    // the parts that are there at all: a part that is off contributes exact zeros and no atomic
    __device__ __forceinline__ bool normalOn() const { return a > 0.0 && cn > 0.0 && sn != 0.0; }
    __device__ __forceinline__ bool tangentOn() const { return a > 0.0 && ct > 0.0 && lt > 0.0; }
};
__device__ __forceinline__ void load_flow(const AeroView& v, int t, Flow& F)
{
    const size_t nT = (size_t)v.nTri;
    const double2* L = reinterpret_cast<const double2*>(v.lagged) + 4 * (size_t)t;
    const double2 l0 = L[0], l1 = L[1], l2 = L[2], l3 = L[3];
    const double2* C = reinterpret_cast<const double2*>(v.coef) + 2 * (size_t)v.surfOf[t];
    const double2 c0 = C[0], c1 = C[1];
    F.n[0] = l0.x;
    F.n[1] = l0.y;
    F.n[2] = l1.x;
    F.a = v.density * l1.y / 6.0;
    const double cn[3] = { l2.x, l2.y, l3.x };
    F.cn = c0.x;
    F.ct = c0.y;
    double x[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        F.node[k] = v.tri[k * nT + t];
        ld3(v.x, F.node[k], x[k]);
    }
    double c[3];
    centroid(x[0], x[1], x[2], c);
#pragma unroll
    for (int a = 0; a < 3; ++a) F.u[a] = (c[a] - cn[a]) / v.dt - v.wind[a];
    F.un = sh::dot(F.u, F.n);
    F.sn = (c1.x != 0.0 && !(F.un > 0.0)) ? 0.0 : F.un; // one-sided: max(0, u_n)
#pragma unroll
    for (int a = 0; a < 3; ++a) F.ut[a] = F.u[a] - F.un * F.n[a];
    F.lt = sqrt(sh::dot(F.ut, F.ut));
}
__device__ __forceinline__ double flow_energy(const AeroView& v, const Flow& F)
{
    const double s = fabs(F.sn);
    return v.dt * F.a * (F.cn * (s * s * s) + F.ct * (F.lt * F.lt * F.lt));
}
// dD_t/dc / 3 = a (Cn |s_n| s_n n + Ct |u_t| u_t): the gradient entry of each of the three nodes; the force on the triangle is -3 times it
__device__ __forceinline__ void flow_gradient(const Flow& F, double* g)
{
    const double gn = F.normalOn() ? F.cn * fabs(F.sn) * F.sn : 0.0, gt = F.tangentOn() ? F.ct * F.lt : 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) g[a] = F.a * (gn * F.n[a] + gt * F.ut[a]);
}

__global__ __launch_bounds__(AERO_BLOCK) void k_aero_refresh(AeroView v, double* __restrict__ lagged)
{
    const int t = blockIdx.x * AERO_BLOCK + threadIdx.x;
    if (t >= v.nTri) return;
    const size_t nT = (size_t)v.nTri;
    double x[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) ld3(v.x, v.tri[k * nT + t], x[k]);
    double e1[3], e2[3], m[3], c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        e1[a] = x[1][a] - x[0][a];
        e2[a] = x[2][a] - x[0][a];
    }
    sh::cross(e1, e2, m);
    const double l = sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
    const bool ok = l > 0.0 && l < INFINITY; // a collapsed triangle: area 0, normal 0 -- it contributes nothing
    centroid(x[0], x[1], x[2], c);
    double2* L = reinterpret_cast<double2*>(lagged) + 4 * (size_t)t;
    L[0] = make_double2(ok ? m[0] / l : 0.0, ok ? m[1] / l : 0.0);
    L[1] = make_double2(ok ? m[2] / l : 0.0, ok ? 0.5 * l : 0.0);
    L[2] = make_double2(c[0], c[1]);
    L[3] = make_double2(c[2], 0.0);
}

__global__ __launch_bounds__(AERO_BLOCK) void k_aero_energy(AeroView v, double coef, double* __restrict__ partial)
{
    const int t = blockIdx.x * AERO_BLOCK + threadIdx.x;
    double e = 0.0;
    if (t < v.nTri) {
        Flow F;
        load_flow(v, t, F);
        e = coef * flow_energy(v, F);
    }
    store_block_sum<AERO_BLOCK>(e, partial);
}
__global__ __launch_bounds__(AERO_BLOCK) void k_aero_energy_per_elem(AeroView v, double* __restrict__ perTri)
{
    const int t = blockIdx.x * AERO_BLOCK + threadIdx.x;
    if (t >= v.nTri) return;
    Flow F;
    load_flow(v, t, F);
    perTri[t] = flow_energy(v, F);
}

template <bool HESS>
__global__ __launch_bounds__(AERO_BLOCK) void k_aero_assemble(AeroView v, double coef, int projectDBC, double* __restrict__ grad, double* __restrict__ a, int* __restrict__ err)
{
    const int t = blockIdx.x * AERO_BLOCK + threadIdx.x;
    if (t >= v.nTri) return;
    Flow F;
    load_flow(v, t, F);
    const bool nOn = F.normalOn(), tOn = F.tangentOn();
    if (!nOn && !tOn) return; // u = 0, the leeward side of a one-sided surface, a collapsed triangle: nothing is written
    bool proj[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) proj[k] = projected_dbc(v.dbc[F.node[k]], projectDBC);
    if (grad) {
        double g[3];
        flow_gradient(F, g);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (!proj[k]) {
#pragma unroll
                for (int r = 0; r < 3; ++r) atomicAdd(&grad[3 * (size_t)F.node[k] + r], coef * g[r]);
            }
    }
    if constexpr (HESS) {
        // K / 9 = (a / (3 dt)) (2 Cn |s_n| n n^T + Ct (|u_t| (I - n n^T) + u_t u_t^T / |u_t|)), once per lane
        const double s = coef * F.a / (3.0 * v.dt);
        const double kn = nOn ? 2.0 * F.cn * fabs(F.sn) : 0.0, kt = tOn ? F.ct * F.lt : 0.0, kq = tOn ? F.ct / F.lt : 0.0;
        double A[9];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = r; c < 3; ++c) A[r + 3 * c] = A[c + 3 * r] = s * (((kn - kt) * F.n[r] * F.n[c] + kq * F.ut[r] * F.ut[c]) + (r == c ? kt : 0.0));
        const CsrSink k{ v.rowBase, v.rowLen, v.ja, a, err };
#pragma unroll
        for (int I = 0; I < 3; ++I) {
            if (proj[I]) continue;
            add_diag(k, F.node[I], A);
#pragma unroll
            for (int J = I + 1; J < 3; ++J)
                if (!proj[J]) add_off(k, F.node[I], F.node[J], A); // (symmetric: the transposition of add_off changes nothing)
        }
    }
}

__global__ __launch_bounds__(AERO_BLOCK) void k_aero_state(AeroView v, double* __restrict__ force, double* __restrict__ partial)
{
    __shared__ double sm[AERO_STATE_Q][AERO_BLOCK / 64];
    const int t = blockIdx.x * AERO_BLOCK + threadIdx.x;
    double q[AERO_STATE_Q] = { 0.0, 0.0, 0.0, 0.0, 0.0 };
    if (t < v.nTri) {
        Flow F;
        load_flow(v, t, F);
        double g[3];
        flow_gradient(F, g);
#pragma unroll
        for (int a = 0; a < 3; ++a) q[a] = -3.0 * g[a];
        q[3] = 3.0 * sh::dot(g, F.u); // -f . u
        q[4] = (F.normalOn() || F.tangentOn()) ? 6.0 * F.a / v.density : 0.0; // (A itself where rho_a A / 6 is exact; within 2 u of it elsewhere)
        if (force) {
#pragma unroll
            for (int a = 0; a < 3; ++a) force[3 * (size_t)t + a] = q[a];
        }
    }
    if (!partial) return;
#pragma unroll
    for (int i = 0; i < AERO_STATE_Q; ++i) {
        const double r = block_sum<AERO_BLOCK>(q[i], sm[i]);
        if (threadIdx.x == 0) partial[(size_t)i * gridDim.x + blockIdx.x] = r;
    }
}
// workgroup i: total5[i] = the sum of the nb partial sums of quantity i, lane l takes l, l + BLOCK, ... in index order, then block_sum
__global__ __launch_bounds__(AERO_BLOCK) void k_aero_state_sum(const double* __restrict__ partial, int nb, double* __restrict__ total5)
{
    __shared__ double sm[AERO_BLOCK / 64];
    double x = 0.0;
    for (int i = threadIdx.x; i < nb; i += AERO_BLOCK) x += partial[(size_t)blockIdx.x * nb + i];
    const double r = block_sum<AERO_BLOCK>(x, sm);
    if (threadIdx.x == 0) total5[blockIdx.x] = r;
}

} // namespace

int aero_energy_blocks(const AeroView& v) { return std::max(1, nblk(v.nTri, AERO_BLOCK)); }

void launch_aero_refresh(const AeroView& v, double* lagged, hipStream_t s)
{
    if (v.nTri <= 0 || !lagged) return;
    hipLaunchKernelGGL(k_aero_refresh, dim3(nblk(v.nTri, AERO_BLOCK)), dim3(AERO_BLOCK), 0, s, v, lagged);
}
void launch_aero_energy(const AeroView& v, double coef, double* partial, double* out, bool accumulate, hipStream_t s)
{
    const int nb = aero_energy_blocks(v);
    hipLaunchKernelGGL(k_aero_energy, dim3(nb), dim3(AERO_BLOCK), 0, s, v, coef, partial);
    launch_reduce_partials(partial, nb, 1.0, accumulate, out, s);
}
void launch_aero_energy_per_elem(const AeroView& v, double* perTri, hipStream_t s)
{
    if (v.nTri <= 0 || !perTri) return;
    hipLaunchKernelGGL(k_aero_energy_per_elem, dim3(nblk(v.nTri, AERO_BLOCK)), dim3(AERO_BLOCK), 0, s, v, perTri);
}
void launch_aero_assemble(const AeroView& v, double coef, int projectDBC, double* grad, double* a, int* err, hipStream_t s)
{
    if (v.nTri <= 0 || (!grad && !a)) return;
    const dim3 grid(nblk(v.nTri, AERO_BLOCK)), block(AERO_BLOCK);
    if (a) hipLaunchKernelGGL(k_aero_assemble<true>, grid, block, 0, s, v, coef, projectDBC, grad, a, err);
    else hipLaunchKernelGGL(k_aero_assemble<false>, grid, block, 0, s, v, coef, projectDBC, grad, a, err);
}
void launch_aero_state(const AeroView& v, double* force, double* partial, double* total5, hipStream_t s)
{
    if (v.nTri <= 0 || (!force && !total5)) return;
    const int nb = aero_energy_blocks(v);
    hipLaunchKernelGGL(k_aero_state, dim3(nb), dim3(AERO_BLOCK), 0, s, v, force, total5 ? partial : nullptr);
    if (total5) hipLaunchKernelGGL(k_aero_state_sum, dim3(AERO_STATE_Q), dim3(AERO_BLOCK), 0, s, partial, nb, total5);
}

} // namespace ipcgpu
