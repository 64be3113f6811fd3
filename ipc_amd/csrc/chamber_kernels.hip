// Pressure chambers: kernels (see chamber_kernels.h for the energy).
//   k_chamber_energy            one lane per triangle, one partial sum per block, reduced in a fixed order
//   k_chamber_assemble<HESS>    one lane per triangle: 3 gradient 3-vectors; with HESS the 9 x 9 block, its Jacobi projection (jacobi9_device.h, M = 9:
//                               252 VGPRs of iteration state, hence one wave per workgroup as in k_contact_hessian) and 6 upper 3 x 3 blocks
//   k_chamber_state             one workgroup per chamber: centroid mean, then volume and area about it
// Register figures: DESIGN.md.
#include "chamber_kernels.h"
#include "csr_scatter_device.h"
#include "stencil_hessian_device.h"
#include <algorithm>

namespace ipcgpu {

namespace {

using namespace scatter; // projected_dbc, ld3, CsrSink, add_diag, add_off, store_block_sum, nblk, launch_reduce_partials (csr_scatter_device.h)

constexpr int CHAMBER_BLOCK = 256;
constexpr int CHAMBER_HESS_W = 64; // one wave per workgroup: the Jacobi iteration on 9 x 9 wants the whole register file of a SIMD lane

// nodes, pressure and y_k = x_k - r_c of triangle t
struct Tri {
    int node[3];
    double p;
    double y[3][3];
};
__device__ __forceinline__ void load_tri(const ChamberView& v, int t, Tri& T)
{
    const size_t n = (size_t)v.nTri;
    const int c = v.chamberOf[t];
    T.p = v.pressure[c];
    double r[3];
    ld3(v.ref, c, r);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        T.node[k] = v.tri[k * n + t];
        double x[3];
        ld3(v.x, T.node[k], x);
#pragma unroll
        for (int a = 0; a < 3; ++a) T.y[k][a] = x[a] - r[a];
    }
}

__device__ __forceinline__ double triple(const double (*y)[3])
{
    double c[3];
    sh::cross(y[1], y[2], c);
    return sh::dot(y[0], c);
}
__device__ __forceinline__ double tri_energy(const Tri& T) { return -(T.p / 6.0) * triple(T.y); }

__global__ __launch_bounds__(CHAMBER_BLOCK) void k_chamber_energy(ChamberView v, double coef, double* __restrict__ partial)
{
    const int t = blockIdx.x * CHAMBER_BLOCK + threadIdx.x;
    double e = 0.0;
    if (t < v.nTri) {
        Tri T;
        load_tri(v, t, T);
        e = coef * tri_energy(T);
    }
    store_block_sum<CHAMBER_BLOCK>(e, partial);
}
__global__ __launch_bounds__(CHAMBER_BLOCK) void k_chamber_energy_per_elem(ChamberView v, double* __restrict__ perTri)
{
    const int t = blockIdx.x * CHAMBER_BLOCK + threadIdx.x;
    if (t >= v.nTri) return;
    Tri T;
    load_tri(v, t, T);
    perTri[t] = tri_energy(T);
}

// C[(3 I + r, 3 J + c)] = s [w]x (r, c) for the block I < J
template <int I, int J>
__device__ __forceinline__ void set_skew(double* C, double s, const double* w)
{
    C[sh::su<9>(3 * I + 0, 3 * J + 0)] = 0.0;
    C[sh::su<9>(3 * I + 0, 3 * J + 1)] = -s * w[2];
    C[sh::su<9>(3 * I + 0, 3 * J + 2)] = s * w[1];
    C[sh::su<9>(3 * I + 1, 3 * J + 0)] = s * w[2];
    C[sh::su<9>(3 * I + 1, 3 * J + 1)] = 0.0;
    C[sh::su<9>(3 * I + 1, 3 * J + 2)] = -s * w[0];
    C[sh::su<9>(3 * I + 2, 3 * J + 0)] = -s * w[1];
    C[sh::su<9>(3 * I + 2, 3 * J + 1)] = s * w[0];
    C[sh::su<9>(3 * I + 2, 3 * J + 2)] = 0.0;
}
// node-pair block (I, J), I <= J, of the projected 9 x 9 matrix
template <int I, int J>
__device__ __forceinline__ void emit_pair(const CsrSink& k, const double* C, const int* node, const bool* proj)
{
    if (proj[I] || proj[J]) return;
    double A[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) A[r + 3 * c] = C[sh::su<9>(3 * I + r, 3 * J + c)];
    if (I == J) add_diag(k, node[I], A);
    else add_off(k, node[I], node[J], A);
}

template <bool HESS>
__global__ __launch_bounds__(HESS ? CHAMBER_HESS_W : CHAMBER_BLOCK) void k_chamber_assemble(ChamberView v, double coef, int projectDBC, double* __restrict__ grad,
    double* __restrict__ a, int* __restrict__ err)
{
    constexpr int W = HESS ? CHAMBER_HESS_W : CHAMBER_BLOCK;
    const int t = blockIdx.x * W + threadIdx.x;
    if (t >= v.nTri) return;
    Tri T;
    load_tri(v, t, T);
    if (T.p == 0.0) return; // an unpressurised chamber writes nothing (the votes of the Jacobi iteration count active lanes only)
    const double s = coef * T.p / 6.0;
    bool proj[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) proj[k] = projected_dbc(v.dbc[T.node[k]], projectDBC);
    if (grad) {
        double g[3][3];
        sh::cross(T.y[1], T.y[2], g[0]);
        sh::cross(T.y[2], T.y[0], g[1]);
        sh::cross(T.y[0], T.y[1], g[2]);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (!proj[k]) {
#pragma unroll
                for (int r = 0; r < 3; ++r) atomicAdd(&grad[3 * (size_t)T.node[k] + r], -s * g[k][r]);
            }
    }
    if constexpr (HESS) {
        double C[81];
#pragma unroll
        for (int I = 0; I < 3; ++I)
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = r; c < 3; ++c) C[sh::su<9>(3 * I + r, 3 * I + c)] = 0.0;
        set_skew<0, 1>(C, s, T.y[2]);
        set_skew<0, 2>(C, -s, T.y[1]);
        set_skew<1, 2>(C, s, T.y[0]);
        sh::project_psd<9>(C);
        const CsrSink k{ v.rowBase, v.rowLen, v.ja, a, err };
        emit_pair<0, 0>(k, C, T.node, proj);
        emit_pair<0, 1>(k, C, T.node, proj);
        emit_pair<1, 1>(k, C, T.node, proj);
        emit_pair<0, 2>(k, C, T.node, proj);
        emit_pair<1, 2>(k, C, T.node, proj);
        emit_pair<2, 2>(k, C, T.node, proj);
    }
}

// sum of NV values per lane over the workgroup, in a fixed tree; the result in sm[q * CHAMBER_BLOCK] for every lane to read
template <int NV>
__device__ __forceinline__ void block_tree(double (&val)[NV], double* sm)
{
    __syncthreads(); // (the previous use of sm is over)
#pragma unroll
    for (int q = 0; q < NV; ++q) sm[q * CHAMBER_BLOCK + threadIdx.x] = val[q];
    __syncthreads();
    for (int off = CHAMBER_BLOCK / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
#pragma unroll
            for (int q = 0; q < NV; ++q) sm[q * CHAMBER_BLOCK + threadIdx.x] += sm[q * CHAMBER_BLOCK + threadIdx.x + off];
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < NV; ++q) val[q] = sm[q * CHAMBER_BLOCK];
}

__global__ __launch_bounds__(CHAMBER_BLOCK) void k_chamber_state(ChamberView v, double* __restrict__ volume, double* __restrict__ area, double* __restrict__ refPoint)
{
    __shared__ double sm[3 * CHAMBER_BLOCK];
    const int c = blockIdx.x;
    const int begin = c ? v.triEnd[c - 1] : 0, end = v.triEnd[c];
    const size_t n = (size_t)v.nTri;
    double S[3] = { 0.0, 0.0, 0.0 };
    for (int t = begin + (int)threadIdx.x; t < end; t += CHAMBER_BLOCK) {
        double x0[3], x1[3], x2[3];
        ld3(v.x, v.tri[t], x0);
        ld3(v.x, v.tri[n + t], x1);
        ld3(v.x, v.tri[2 * n + t], x2);
#pragma unroll
        for (int a = 0; a < 3; ++a) S[a] += (x0[a] + x1[a]) + x2[a];
    }
    block_tree<3>(S, sm);
    const double m3 = 3.0 * (double)(end - begin);
    const double r[3] = { S[0] / m3, S[1] / m3, S[2] / m3 };
    if (refPoint && threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) refPoint[3 * (size_t)c + a] = r[a];
    }
    if (!volume && !area) return;
    double VA[2] = { 0.0, 0.0 };
    for (int t = begin + (int)threadIdx.x; t < end; t += CHAMBER_BLOCK) {
        double y[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double x[3];
            ld3(v.x, v.tri[k * n + t], x);
#pragma unroll
            for (int a = 0; a < 3; ++a) y[k][a] = x[a] - r[a];
        }
        VA[0] += triple(y);
        double e1[3], e2[3], nrm[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            e1[a] = y[1][a] - y[0][a];
            e2[a] = y[2][a] - y[0][a];
        }
        sh::cross(e1, e2, nrm);
        VA[1] += sqrt(sh::dot(nrm, nrm));
    }
    block_tree<2>(VA, sm);
    if (threadIdx.x == 0) {
        if (volume) volume[c] = VA[0] / 6.0;
        if (area) area[c] = 0.5 * VA[1];
    }
}

// ---- the gas law ----
constexpr int GAS_MAX = 8; // gas chambers per context (chamber_plan.h: CHAMBER_GAS_MAX)
constexpr int GAS_DOT_BLOCKS = 128; // partial sums per dot product at the most

// pass 1: one workgroup per slice, one lane per triangle of it
__global__ __launch_bounds__(CHAMBER_BLOCK) void k_chamber_gas_slice(ChamberView v, ChamberGasView g)
{
    const int t = g.sliceBegin[blockIdx.x] + (int)threadIdx.x;
    double e = 0.0;
    if (t < g.sliceEnd[blockIdx.x]) {
        Tri T;
        load_tri(v, t, T);
        e = triple(T.y);
    }
    store_block_sum<CHAMBER_BLOCK>(e, g.slicePartial);
}

// pass 2: wave w takes gas chamber w; thread 0 then adds the energies in chamber order
__global__ __launch_bounds__(64 * GAS_MAX) void k_chamber_gas_state(ChamberGasView g, double coef, double* __restrict__ out, int accumulate)
{
    __shared__ double sW[GAS_MAX];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (w < g.nGas) {
        double x = 0.0;
        for (int i = g.sliceOff[w] + lane; i < g.sliceOff[w + 1]; i += 64) x += g.slicePartial[i];
        x = wave_sum(x);
        if (lane == 0) {
            const int c = g.gasChamber[w];
            const double V = x / 6.0, pAmb = g.param[3 * c], gamma = g.param[3 * c + 1], V0 = g.param[3 * c + 2], pc = g.basePressure[c], P0 = pAmb + pc;
            double gauge = 0.0, beta = 0.0, W = INFINITY;
            if (V > 0.0) {
                // ln(V0 / V).  Near V0 from the exact difference V - V0: log(V0 / V) carries the quotient's rounding, an ABSOLUTE error of u however close V is
                // to V0, i.e. u P0 V0 in W -- with real air far above what the line search must resolve for a body at rest (the two terms of W nearly cancel
                // there).  Far from V0 the quotient is the better conditioned form (log1p amplifies the error of its argument by V0 / V).
                const double dV = V - V0;
                const double lr = fabs(dV) <= 0.5 * V0 ? -log1p(dV / V0) : log(V0 / V);
                const double grow = expm1(gamma * lr); // (V0 / V)^gamma - 1
                gauge = pc + P0 * grow;
                beta = gamma * (P0 + P0 * grow) / V;
                W = (gamma == 1.0 ? P0 * V0 * lr : P0 * V0 * (expm1((gamma - 1.0) * lr) / (gamma - 1.0))) + pAmb * (V - V0);
            }
            g.state[4 * c] = V;
            g.state[4 * c + 1] = gauge;
            g.state[4 * c + 2] = beta;
            g.state[4 * c + 3] = W;
            g.effPressure[c] = gauge;
            sW[w] = W;
        }
    }
    __syncthreads();
    if (out && threadIdx.x == 0) {
        double e = accumulate ? out[0] : 0.0;
        if (coef != 0.0) // (0 x inf of a collapsed chamber would be NaN: a zero coefficient adds nothing)
            for (int i = 0; i < g.nGas; ++i) e += coef * sW[i];
        out[0] = e;
    }
}

__global__ __launch_bounds__(CHAMBER_BLOCK) void k_chamber_gas_energy_per_elem(ChamberView v, const int* __restrict__ isGas, const double* __restrict__ state, double* __restrict__ perTri)
{
    const int t = blockIdx.x * CHAMBER_BLOCK + threadIdx.x;
    if (t >= v.nTri) return;
    const int c = v.chamberOf[t];
    if (!isGas[c]) return;
    Tri T;
    load_tri(v, t, T);
    perTri[t] = state[4 * c + 3] * ((triple(T.y) / 6.0) / state[4 * c]);
}

// dot product q of the k + k (k + 1) / 2: q < k is u_q . y, then u_i . z_j for i <= j in row order; one partial per workgroup, each workgroup a contiguous chunk
__global__ __launch_bounds__(CHAMBER_BLOCK) void k_chamber_gas_dots(int k, size_t n3, size_t chunk, const double* __restrict__ U, const double* __restrict__ Z, const double* __restrict__ y,
    double* __restrict__ partial)
{
    int q = blockIdx.y, i = q, j = -1;
    if (q >= k) {
        q -= k;
        for (i = 0; q >= k - i; ++i) q -= k - i;
        j = i + q;
    }
    const double* a = U + (size_t)i * n3;
    const double* b = j < 0 ? y : Z + (size_t)j * n3;
    const size_t begin = blockIdx.x * chunk, end = begin + chunk < n3 ? begin + chunk : n3;
    double x = 0.0;
    for (size_t e = begin + threadIdx.x; e < end; e += CHAMBER_BLOCK) x += a[e] * b[e];
    __shared__ double sm[CHAMBER_BLOCK / 64];
    const double r = block_sum<CHAMBER_BLOCK>(x, sm);
    if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = r;
}

// one wave: the second pass of the dot products, then C w = U^T y by a k x k Cholesky
__global__ __launch_bounds__(64) void k_chamber_gas_small_solve(ChamberGasView g, double coef, int nb, const double* __restrict__ partial, double* __restrict__ w)
{
    __shared__ double sd[GAS_MAX + GAS_MAX * (GAS_MAX + 1) / 2];
    const int k = g.nGas, nq = k + k * (k + 1) / 2, lane = threadIdx.x;
    for (int q = 0; q < nq; ++q) {
        double x = 0.0;
        for (int i = lane; i < nb; i += 64) x += partial[(size_t)q * nb + i];
        x = wave_sum(x);
        if (lane == 0) sd[q] = x;
    }
    __syncthreads();
    if (lane != 0) return;
    __shared__ double C[GAS_MAX][GAS_MAX], b[GAS_MAX]; // (in LDS: indexed by loop variables, registers would spill to scratch)
    __shared__ int on[GAS_MAX];
    int q = k;
    for (int i = 0; i < k; ++i) {
        const double cb = coef * g.state[4 * g.gasChamber[i] + 2];
        on[i] = cb > 0.0;
        b[i] = sd[i];
        for (int j = i; j < k; ++j) C[j][i] = C[i][j] = sd[q++];
        C[i][i] += on[i] ? 1.0 / cb : 0.0;
    }
    // a chamber without a rank-one term (beta == 0) leaves the system: its row and column become the identity's
    for (int i = 0; i < k; ++i)
        if (!on[i]) {
            for (int j = 0; j < k; ++j) C[i][j] = C[j][i] = 0.0;
            C[i][i] = 1.0;
            b[i] = 0.0;
        }
    for (int j = 0; j < k; ++j) { // C = L L^T, L in the lower triangle
        double d = C[j][j];
        for (int p = 0; p < j; ++p) d -= C[j][p] * C[j][p];
        d = sqrt(d);
        C[j][j] = d;
        for (int i = j + 1; i < k; ++i) {
            double x = C[i][j];
            for (int p = 0; p < j; ++p) x -= C[i][p] * C[j][p];
            C[i][j] = x / d;
        }
    }
    for (int i = 0; i < k; ++i) {
        double x = b[i];
        for (int p = 0; p < i; ++p) x -= C[i][p] * b[p];
        b[i] = x / C[i][i];
    }
    for (int i = k - 1; i >= 0; --i) {
        double x = b[i];
        for (int p = i + 1; p < k; ++p) x -= C[p][i] * b[p];
        b[i] = x / C[i][i];
    }
    for (int i = 0; i < GAS_MAX; ++i) w[i] = i < k ? b[i] : 0.0;
}

__global__ __launch_bounds__(CHAMBER_BLOCK) void k_chamber_gas_apply(int k, size_t n3, const double* __restrict__ Z, const double* __restrict__ w, double* __restrict__ y)
{
    const size_t e = (size_t)blockIdx.x * CHAMBER_BLOCK + threadIdx.x;
    if (e >= n3) return;
    double x = y[e];
    for (int c = 0; c < k; ++c) x -= Z[(size_t)c * n3 + e] * w[c];
    y[e] = x;
}

int gas_dot_blocks(size_t n3) { return (int)std::max<size_t>(1, std::min<size_t>(GAS_DOT_BLOCKS, (n3 + CHAMBER_BLOCK - 1) / CHAMBER_BLOCK)); }

} // namespace

void launch_chamber_gas_update(const ChamberView& v, const ChamberGasView& g, double coef, double* out, bool accumulate, hipStream_t s)
{
    if (g.nGas <= 0) return;
    hipLaunchKernelGGL(k_chamber_gas_slice, dim3(g.nSlice), dim3(CHAMBER_BLOCK), 0, s, v, g);
    hipLaunchKernelGGL(k_chamber_gas_state, dim3(1), dim3(64 * GAS_MAX), 0, s, g, coef, out, accumulate ? 1 : 0);
}
void launch_chamber_gas_energy_per_elem(const ChamberView& v, const int* isGas, const double* state, double* perTri, hipStream_t s)
{
    if (v.nTri <= 0 || !perTri) return;
    hipLaunchKernelGGL(k_chamber_gas_energy_per_elem, dim3(nblk(v.nTri, CHAMBER_BLOCK)), dim3(CHAMBER_BLOCK), 0, s, v, isGas, state, perTri);
}
void launch_chamber_volume_gradient(const ChamberView& v, const double* select, int projectDBC, double* u, size_t n3, hipStream_t s)
{
    (void)hipMemsetAsync(u, 0, n3 * sizeof(double), s);
    ChamberView one = v;
    one.pressure = select;
    launch_chamber_assemble(one, -1.0, projectDBC, u, nullptr, nullptr, s); // dW/dx = -p gradV: p = 1 and the coefficient -1 leave gradV
}
size_t chamber_gas_dot_doubles(size_t n3, int k) { return (size_t)gas_dot_blocks(n3) * (size_t)(k + k * (k + 1) / 2); }
void launch_chamber_gas_woodbury(const ChamberGasView& g, double coef, size_t n3, const double* U, const double* Z, double* y, double* dots, double* w, hipStream_t s)
{
    const int k = g.nGas;
    if (k <= 0 || !n3) return;
    const int nb = gas_dot_blocks(n3);
    const size_t chunk = (n3 + nb - 1) / nb;
    hipLaunchKernelGGL(k_chamber_gas_dots, dim3(nb, k + k * (k + 1) / 2), dim3(CHAMBER_BLOCK), 0, s, k, n3, chunk, U, Z, y, dots);
    hipLaunchKernelGGL(k_chamber_gas_small_solve, dim3(1), dim3(64), 0, s, g, coef, nb, dots, w);
    hipLaunchKernelGGL(k_chamber_gas_apply, dim3((unsigned)((n3 + CHAMBER_BLOCK - 1) / CHAMBER_BLOCK)), dim3(CHAMBER_BLOCK), 0, s, k, n3, Z, w, y);
}

int chamber_energy_blocks(const ChamberView& v) { return std::max(1, nblk(v.nTri, CHAMBER_BLOCK)); }

void launch_chamber_energy(const ChamberView& v, double coef, double* partial, double* out, bool accumulate, hipStream_t s)
{
    const int nb = chamber_energy_blocks(v);
    hipLaunchKernelGGL(k_chamber_energy, dim3(nb), dim3(CHAMBER_BLOCK), 0, s, v, coef, partial);
    launch_reduce_partials(partial, nb, 1.0, accumulate, out, s);
}
void launch_chamber_energy_per_elem(const ChamberView& v, double* perTri, hipStream_t s)
{
    if (v.nTri <= 0 || !perTri) return;
    hipLaunchKernelGGL(k_chamber_energy_per_elem, dim3(nblk(v.nTri, CHAMBER_BLOCK)), dim3(CHAMBER_BLOCK), 0, s, v, perTri);
}
void launch_chamber_assemble(const ChamberView& v, double coef, int projectDBC, double* grad, double* a, int* err, hipStream_t s)
{
    if (v.nTri <= 0) return;
    if (a) hipLaunchKernelGGL(k_chamber_assemble<true>, dim3(nblk(v.nTri, CHAMBER_HESS_W)), dim3(CHAMBER_HESS_W), 0, s, v, coef, projectDBC, grad, a, err);
    else hipLaunchKernelGGL(k_chamber_assemble<false>, dim3(nblk(v.nTri, CHAMBER_BLOCK)), dim3(CHAMBER_BLOCK), 0, s, v, coef, projectDBC, grad, a, err);
}
void launch_chamber_state(const ChamberView& v, double* volume, double* area, double* refPoint, hipStream_t s)
{
    if (v.n <= 0 || (!volume && !area && !refPoint)) return;
    hipLaunchKernelGGL(k_chamber_state, dim3(v.n), dim3(CHAMBER_BLOCK), 0, s, v, volume, area, refPoint);
}

} // namespace ipcgpu
