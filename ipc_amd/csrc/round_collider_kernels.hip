// Round collider kernels (sphere / capsule obstacle; the model is stated in round_collider_kernels.h).  Per-vertex streaming work like the half-space
// unit: one lane per surface vertex / per set entry, 24 B of position per vertex, the shape passed by value.  Each pass is bounded by HBM latency;
// beside the half-space kernels a lane pays one fp64 square root and one division for the distance (rc_eval), and the step bound up to three more of
// each for its quadratics.  Compiled with -ffp-contract=off like the half-space unit.
#include "round_collider_kernels.h"
#include "contact_device.h"
#include "device_prims.h"
#include <cmath>
#include <cstring>
#include <hipcub/hipcub.hpp>

namespace ipcgpu {
namespace {
constexpr int BLOCK = 256;
constexpr double NO_BOUND = 1.0e300;

using namespace prims;

// order-preserving map double -> uint64 so that atomicMin works for either sign (as hip_halfspace.hip)
__device__ __forceinline__ unsigned long long ordered_bits(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
inline double from_ordered_bits(unsigned long long k)
{
    const unsigned long long b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    double v;
    std::memcpy(&v, &b, sizeof(v));
    return v;
}

// distance, normal and region of one vertex: THE evaluation every kernel below calls
struct RoundEval {
    double s, invr; // signed distance side (r - R); 1 / r (0 where r == 0)
    double m[3];    // (x - q) / r, the zero vector where r == 0; the normal is side m
    int sideRegion; // closest point strictly inside the segment
};
__device__ __forceinline__ RoundEval rc_eval(const RoundShape& c, double x0, double x1, double x2)
{
    const double d[3] = { x0 - c.p0[0], x1 - c.p0[1], x2 - c.p0[2] };
    const double u = d[0] * c.axis[0] + d[1] * c.axis[1] + d[2] * c.axis[2];
    const double t = fmin(fmax(u, 0.0), c.len);
    const double w[3] = { d[0] - t * c.axis[0], d[1] - t * c.axis[1], d[2] - t * c.axis[2] };
    const double r = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    RoundEval e;
    e.invr = r > 0.0 ? 1.0 / r : 0.0;
    e.m[0] = w[0] * e.invr;
    e.m[1] = w[1] * e.invr;
    e.m[2] = w[2] * e.invr;
    e.s = c.side * (r - c.R);
    e.sideRegion = (u > 0.0 && u < c.len) ? 1 : 0;
    return e;
}
__device__ __forceinline__ RoundEval rc_eval(const RoundShape& c, const double* __restrict__ x, int v)
{
    return rc_eval(c, x[3 * (size_t)v], x[3 * (size_t)v + 1], x[3 * (size_t)v + 2]);
}

__global__ __launch_bounds__(BLOCK) void k_rc_flags(int nSVI, const int* __restrict__ svi, const double* __restrict__ x, const int* __restrict__ dbc,
    RoundShape c, double dHat, int* __restrict__ flags)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nSVI) return;
    const int v = svi[i];
    const double s = rc_eval(c, x, v).s;
    flags[i] = (dbc[v] == 0 && s * s < dHat) ? 1 : 0;
}

__global__ __launch_bounds__(BLOCK) void k_rc_energy(int n, const int* __restrict__ set, const double* __restrict__ x, RoundShape c, double dHat,
    double* __restrict__ partial)
{
    __shared__ double sm[BLOCK / 64];
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    double val = 0.0;
    if (i < n) {
        const double s = rc_eval(c, x, set[i]).s;
        double b, gb, Hb;
        cdev::barrier(s * s, dHat, &b, &gb, &Hb);
        val = b;
    }
    const double r = block_sum<BLOCK>(val, sm);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

__global__ __launch_bounds__(BLOCK) void k_rc_gradient(int n, const int* __restrict__ set, const double* __restrict__ x, RoundShape c, double dHat,
    double kappa, double* __restrict__ grad)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int v = set[i]; // vertices of one set are distinct: plain read-modify-write
    const RoundEval e = rc_eval(c, x, v);
    double b, gb, Hb;
    cdev::barrier(e.s * e.s, dHat, &b, &gb, &Hb);
    const double f = kappa * gb * 2.0 * e.s * c.side;
    grad[3 * (size_t)v] += f * e.m[0];
    grad[3 * (size_t)v + 1] += f * e.m[1];
    grad[3 * (size_t)v + 2] += f * e.m[2];
}

__global__ __launch_bounds__(BLOCK) void k_rc_hessian(int n, const int* __restrict__ set, const double* __restrict__ x, const int* __restrict__ dbc,
    const int* __restrict__ rowBase, const int* __restrict__ rowLen, RoundShape c, double dHat, double kappa, int projectDBC, double* __restrict__ a)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int v = set[i];
    if (dbc[v] != 0 && projectDBC) return;
    const RoundEval e = rc_eval(c, x, v);
    const double d = e.s * e.s;
    double b, gb, Hb;
    cdev::barrier(d, dHat, &b, &gb, &Hb);
    // the two eigenvalue coefficients, clamped at 0: the PSD projection in closed form
    double c1 = 4.0 * Hb * d + 2.0 * gb, c2 = 2.0 * gb * e.s * c.side * e.invr;
    if (!(c1 > 0.0)) c1 = 0.0;
    if (!(c2 > 0.0)) c2 = 0.0;
    if (c1 == 0.0 && c2 == 0.0) return;
    c1 *= kappa;
    c2 *= kappa;
    const double ax = e.sideRegion ? 1.0 : 0.0;
    const double* m = e.m;
    const double* ua = c.axis;
    const int p0 = rowBase[v], L = rowLen[v]; // upper triangle of the diagonal 3x3 block
    a[p0] += c1 * (m[0] * m[0]) + c2 * (1.0 - m[0] * m[0] - ax * (ua[0] * ua[0]));
    a[p0 + 1] += c1 * (m[0] * m[1]) + c2 * (-(m[0] * m[1]) - ax * (ua[0] * ua[1]));
    a[p0 + 2] += c1 * (m[0] * m[2]) + c2 * (-(m[0] * m[2]) - ax * (ua[0] * ua[2]));
    a[p0 + L] += c1 * (m[1] * m[1]) + c2 * (1.0 - m[1] * m[1] - ax * (ua[1] * ua[1]));
    a[p0 + L + 1] += c1 * (m[1] * m[2]) + c2 * (-(m[1] * m[2]) - ax * (ua[1] * ua[2]));
    a[p0 + 2 * L - 1] += c1 * (m[2] * m[2]) + c2 * (1.0 - m[2] * m[2] - ax * (ua[2] * ua[2]));
}

// smallest positive t with |d + t p| = rad for a point outside the ball (C > 0): the entry root, written without cancellation
__device__ __forceinline__ double ray_ball_entry(const double* d, const double* p, double rad)
{
    const double A = p[0] * p[0] + p[1] * p[1] + p[2] * p[2], B = d[0] * p[0] + d[1] * p[1] + d[2] * p[2];
    const double C = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] - rad * rad;
    if (!(C > 0.0) || !(B < 0.0)) return NO_BOUND;
    const double disc = B * B - A * C;
    if (!(disc >= 0.0)) return NO_BOUND;
    return C / (sqrt(disc) - B);
}
// the first t > 0 at which s(x + t p) = (1 - slackness) s(x); NO_BOUND where the ray never gets there
__device__ __forceinline__ double rc_ray(const RoundShape& c, double x0, double x1, double x2, const double* p, double slackness)
{
    const double s0 = rc_eval(c, x0, x1, x2).s;
    if (!(s0 > 0.0)) return NO_BOUND; // (an intersecting state is refused before any step is bounded)
    const double rad = c.R + c.side * ((1.0 - slackness) * s0);
    const double d[3] = { x0 - c.p0[0], x1 - c.p0[1], x2 - c.p0[2] };
    if (c.side < 0.0) { // hollow sphere: the exit root of a point inside the ball of radius rad
        const double A = p[0] * p[0] + p[1] * p[1] + p[2] * p[2], B = d[0] * p[0] + d[1] * p[1] + d[2] * p[2];
        const double C = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] - rad * rad;
        if (!(A > 0.0) || !(C < 0.0)) return NO_BOUND;
        const double sq = sqrt(B * B - A * C);
        return B <= 0.0 ? (sq - B) / A : -C / (B + sq);
    }
    double best = ray_ball_entry(d, p, rad);
    if (c.len > 0.0) {
        const double e[3] = { x0 - c.p1[0], x1 - c.p1[1], x2 - c.p1[2] };
        best = fmin(best, ray_ball_entry(e, p, rad));
        // the cylinder piece: the components across the axis, and the axial parameter at the root inside [0, len]
        const double du = d[0] * c.axis[0] + d[1] * c.axis[1] + d[2] * c.axis[2], pu = p[0] * c.axis[0] + p[1] * c.axis[1] + p[2] * c.axis[2];
        const double dp[3] = { d[0] - du * c.axis[0], d[1] - du * c.axis[1], d[2] - du * c.axis[2] };
        const double pp[3] = { p[0] - pu * c.axis[0], p[1] - pu * c.axis[1], p[2] - pu * c.axis[2] };
        const double t = ray_ball_entry(dp, pp, rad);
        if (t < NO_BOUND) {
            const double u = du + t * pu;
            if (u >= 0.0 && u <= c.len) best = fmin(best, t);
        }
    }
    return best;
}

// p_dev: one direction per node, bounded by the nodes with dbc == 0; p_dev == nullptr: the constant direction pc for every surface node (move)
__global__ __launch_bounds__(BLOCK) void k_rc_step(int nSVI, const int* __restrict__ svi, const double* __restrict__ x, const int* __restrict__ dbc,
    const double* __restrict__ p_dev, double pc0, double pc1, double pc2, RoundShape c, double slackness, unsigned long long* __restrict__ out)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    double best = NO_BOUND;
    if (i < nSVI) {
        const int v = svi[i];
        if (!p_dev || dbc[v] == 0) {
            double p[3] = { pc0, pc1, pc2 };
            if (p_dev) {
                p[0] = p_dev[3 * (size_t)v];
                p[1] = p_dev[3 * (size_t)v + 1];
                p[2] = p_dev[3 * (size_t)v + 2];
            }
            best = rc_ray(c, x[3 * (size_t)v], x[3 * (size_t)v + 1], x[3 * (size_t)v + 2], p, slackness);
        }
    }
    best = wave_min(best);
    if ((threadIdx.x & 63) == 0) atomicMin(out, ordered_bits(best));
}

__global__ __launch_bounds__(BLOCK) void k_rc_intersected(int nV, const double* __restrict__ x, const int* __restrict__ dbc, RoundShape c, int* __restrict__ flag)
{
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= nV || dbc[v] != 0) return;
    if (rc_eval(c, x, v).s <= 0.0) flag[0] = 1;
}

__global__ __launch_bounds__(BLOCK) void k_rc_dist2(int n, const int* __restrict__ verts, const double* __restrict__ x, RoundShape c, double* __restrict__ out)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const double s = rc_eval(c, x, verts[i]).s;
    out[i] = s * s;
}

__global__ __launch_bounds__(BLOCK) void k_rc_min_s(int nSVI, const int* __restrict__ svi, const double* __restrict__ x, RoundShape c, unsigned long long* __restrict__ out)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    double best = INFINITY;
    if (i < nSVI) best = rc_eval(c, x, svi[i]).s;
    best = wave_min(best);
    if ((threadIdx.x & 63) == 0) atomicMin(out, ordered_bits(best));
}

// ---- lagged friction: the half-space's terms with the lagged normal of each entry ----------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_rc_lag(int n, const int* __restrict__ set, const double* __restrict__ x, RoundShape c, double dHat, double kappa,
    double* __restrict__ lambda, double* __restrict__ normal)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const RoundEval e = rc_eval(c, x, set[i]);
    double b, gb, Hb;
    cdev::barrier(e.s * e.s, dHat, &b, &gb, &Hb);
    lambda[i] = gb * (-kappa * 2.0 * e.s);
    normal[3 * (size_t)i] = c.side * e.m[0];
    normal[3 * (size_t)i + 1] = c.side * e.m[1];
    normal[3 * (size_t)i + 2] = c.side * e.m[2];
}
__device__ __forceinline__ void rc_proj(const double* nn, const double* __restrict__ x, const double* __restrict__ xt, int v, double* vp)
{
    const double vd[3] = { x[3 * (size_t)v] - xt[3 * (size_t)v], x[3 * (size_t)v + 1] - xt[3 * (size_t)v + 1], x[3 * (size_t)v + 2] - xt[3 * (size_t)v + 2] };
    const double dn = vd[0] * nn[0] + vd[1] * nn[1] + vd[2] * nn[2];
    vp[0] = vd[0] - dn * nn[0];
    vp[1] = vd[1] - dn * nn[1];
    vp[2] = vd[2] - dn * nn[2];
}
__global__ __launch_bounds__(BLOCK) void k_rc_fric_energy(int n, const int* __restrict__ set, const double* __restrict__ lambda, const double* __restrict__ normal,
    const double* __restrict__ x, const double* __restrict__ xt, double mu, double eps2, double* __restrict__ partial)
{
    __shared__ double sm[BLOCK / 64];
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    double val = 0.0;
    if (i < n) {
        const double nn[3] = { normal[3 * (size_t)i], normal[3 * (size_t)i + 1], normal[3 * (size_t)i + 2] };
        double vp[3];
        rc_proj(nn, x, xt, set[i], vp);
        const double m2 = vp[0] * vp[0] + vp[1] * vp[1] + vp[2] * vp[2], eps = sqrt(eps2);
        val = (m2 > eps2) ? mu * lambda[i] * (sqrt(m2) - eps * 0.5) : mu * lambda[i] * m2 / eps * 0.5;
    }
    const double r = block_sum<BLOCK>(val, sm);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}
__global__ __launch_bounds__(BLOCK) void k_rc_fric_gradient(int n, const int* __restrict__ set, const double* __restrict__ lambda, const double* __restrict__ normal,
    const double* __restrict__ x, const double* __restrict__ xt, double mu, double eps2, double* __restrict__ grad)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int v = set[i];
    const double nn[3] = { normal[3 * (size_t)i], normal[3 * (size_t)i + 1], normal[3 * (size_t)i + 2] };
    double vp[3];
    rc_proj(nn, x, xt, v, vp);
    const double m2 = vp[0] * vp[0] + vp[1] * vp[1] + vp[2] * vp[2];
    const double sc = (m2 > eps2) ? mu * lambda[i] / sqrt(m2) : mu * lambda[i] / sqrt(eps2);
    for (int k = 0; k < 3; ++k) grad[3 * (size_t)v + k] += sc * vp[k];
}
// sliding: ml/|v| (P - vhat vhat^T) with P = I - n n^T, eigenvalues {ml/|v|, 0, 0}; sticking: ml/eps P -- both PSD as they stand (k_hs_fric_hessian)
__global__ __launch_bounds__(BLOCK) void k_rc_fric_hessian(int n, const int* __restrict__ set, const double* __restrict__ lambda, const double* __restrict__ normal,
    const double* __restrict__ x, const double* __restrict__ xt, const int* __restrict__ dbc, const int* __restrict__ rowBase, const int* __restrict__ rowLen,
    double mu, double eps2, int projectDBC, double* __restrict__ a)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int v = set[i];
    if (projectDBC && dbc[v] != 0) return;
    const double ml = mu * lambda[i];
    const double nn[3] = { normal[3 * (size_t)i], normal[3 * (size_t)i + 1], normal[3 * (size_t)i + 2] };
    double vp[3];
    rc_proj(nn, x, xt, v, vp);
    const double m2 = vp[0] * vp[0] + vp[1] * vp[1] + vp[2] * vp[2];
    double H[3][3];
    if (m2 > eps2) {
        const double mag = sqrt(m2);
        for (int r = 0; r < 3; ++r)
            for (int k = r; k < 3; ++k) H[r][k] = vp[r] * (-ml / m2 / mag) * vp[k] + ((r == k ? 1.0 : 0.0) - nn[r] * nn[k]) * (ml / mag);
    }
    else
        for (int r = 0; r < 3; ++r)
            for (int k = r; k < 3; ++k) H[r][k] = ((r == k ? 1.0 : 0.0) - nn[r] * nn[k]) * (ml / sqrt(eps2));
    const int p0 = rowBase[v], L = rowLen[v];
    a[p0] += H[0][0];
    a[p0 + 1] += H[0][1];
    a[p0 + 2] += H[0][2];
    a[p0 + L] += H[1][1];
    a[p0 + L + 1] += H[1][2];
    a[p0 + 2 * L - 1] += H[2][2];
}

// ---- state query: per-workgroup sums in a fixed order -----------------------------------------------------------------------------------------------
// partial[j * nb + block], j = 0..2 the barrier force on the bodies (minus the gradient), j = 3..5 its torque about p0
__global__ __launch_bounds__(BLOCK) void k_rc_state(int n, int nb, const int* __restrict__ set, const double* __restrict__ x, RoundShape c, double dHat, double kappa,
    double* __restrict__ partial)
{
    __shared__ double sm[BLOCK / 64];
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    double q[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    if (i < n) {
        const int v = set[i];
        const RoundEval e = rc_eval(c, x, v);
        double b, gb, Hb;
        cdev::barrier(e.s * e.s, dHat, &b, &gb, &Hb);
        const double f = -(kappa * gb * 2.0 * e.s * c.side);
        const double d[3] = { x[3 * (size_t)v] - c.p0[0], x[3 * (size_t)v + 1] - c.p0[1], x[3 * (size_t)v + 2] - c.p0[2] };
        q[0] = f * e.m[0];
        q[1] = f * e.m[1];
        q[2] = f * e.m[2];
        q[3] = d[1] * q[2] - d[2] * q[1];
        q[4] = d[2] * q[0] - d[0] * q[2];
        q[5] = d[0] * q[1] - d[1] * q[0];
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const double r = block_sum<BLOCK>(q[j], sm);
        if (threadIdx.x == 0) partial[(size_t)j * nb + blockIdx.x] = r;
        __syncthreads();
    }
}
// partial[j * nb + block], j = 0..2: the lagged friction force on the bodies (minus the friction gradient)
__global__ __launch_bounds__(BLOCK) void k_rc_fric_state(int n, int nb, const int* __restrict__ set, const double* __restrict__ lambda,
    const double* __restrict__ normal, const double* __restrict__ x, const double* __restrict__ xt, double mu, double eps2, double* __restrict__ partial)
{
    __shared__ double sm[BLOCK / 64];
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    double q[3] = { 0.0, 0.0, 0.0 };
    if (i < n) {
        const double nn[3] = { normal[3 * (size_t)i], normal[3 * (size_t)i + 1], normal[3 * (size_t)i + 2] };
        double vp[3];
        rc_proj(nn, x, xt, set[i], vp);
        const double m2 = vp[0] * vp[0] + vp[1] * vp[1] + vp[2] * vp[2];
        const double sc = (m2 > eps2) ? mu * lambda[i] / sqrt(m2) : mu * lambda[i] / sqrt(eps2);
        for (int k = 0; k < 3; ++k) q[k] = -(sc * vp[k]);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double r = block_sum<BLOCK>(q[j], sm);
        if (threadIdx.x == 0) partial[(size_t)j * nb + blockIdx.x] = r;
        __syncthreads();
    }
}
} // namespace

int HipRoundCollider::build(int nSVI, const int* svi_dev, const double* x_dev, const int* dbc_dev, double dHat)
{
    set.clear();
    if (!nSVI) return 0;
    flags_.alloc(nSVI);
    d_set.alloc(nSVI);
    count_.alloc(1);
    hipLaunchKernelGGL(k_rc_flags, dim3(nblk(nSVI, BLOCK)), dim3(BLOCK), 0, stream, nSVI, svi_dev, x_dev, dbc_dev, shape, dHat, flags_.p);
    size_t bytes = 0; // order-preserving compaction: ascending surface-vertex order
    HIP_CHECK(hipcub::DeviceSelect::Flagged(nullptr, bytes, svi_dev, flags_.p, d_set.p, count_.p, nSVI, stream));
    if (tmp_.n < bytes) tmp_.alloc(bytes);
    HIP_CHECK(hipcub::DeviceSelect::Flagged(tmp_.p, bytes, svi_dev, flags_.p, d_set.p, count_.p, nSVI, stream));
    int cnt = 0;
    count_.download(&cnt, 1, stream);
    set.resize(cnt);
    if (cnt) d_set.download(set.data(), cnt, stream);
    return cnt;
}

void HipRoundCollider::setSet(int cnt, const int* verts)
{
    set.assign(verts, verts + cnt);
    if (d_set.n < (size_t)cnt) d_set.alloc(cnt);
    if (cnt) HIP_CHECK(hipMemcpyAsync(d_set.p, set.data(), cnt * sizeof(int), hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
}

double HipRoundCollider::energy(const double* x_dev, double dHat, double kappa)
{
    const int cnt = (int)set.size();
    if (!cnt) return 0.0;
    const int nb = nblk(cnt, BLOCK);
    if (partial_.n < (size_t)nb + 1) partial_.alloc(nb + 1);
    hipLaunchKernelGGL(k_rc_energy, dim3(nb), dim3(BLOCK), 0, stream, cnt, d_set.p, x_dev, shape, dHat, partial_.p + 1);
    launch_reduce_partials(partial_.p + 1, nb, kappa, false, partial_.p, stream);
    double out = 0.0;
    partial_.download(&out, 1, stream);
    return out;
}

void HipRoundCollider::gradientAdd(const double* x_dev, double dHat, double kappa, double* grad_dev)
{
    const int cnt = (int)set.size();
    if (!cnt) return;
    hipLaunchKernelGGL(k_rc_gradient, dim3(nblk(cnt, BLOCK)), dim3(BLOCK), 0, stream, cnt, d_set.p, x_dev, shape, dHat, kappa, grad_dev);
}

void HipRoundCollider::hessianAdd(const double* x_dev, const int* dbc_dev, const int* rowBase_dev, const int* rowLen_dev, double dHat, double kappa,
    int projectDBC, double* a_dev)
{
    const int cnt = (int)set.size();
    if (!cnt) return;
    hipLaunchKernelGGL(k_rc_hessian, dim3(nblk(cnt, BLOCK)), dim3(BLOCK), 0, stream, cnt, d_set.p, x_dev, dbc_dev, rowBase_dev, rowLen_dev, shape, dHat, kappa,
        projectDBC, a_dev);
}

double HipRoundCollider::rayBound(int nSVI, const int* svi_dev, const double* x_dev, const int* dbc_dev, const double* p_dev, const double* pc, double slackness)
{
    minOut_.alloc(1);
    const unsigned long long init = ~0ull;
    HIP_CHECK(hipMemcpyAsync(minOut_.p, &init, sizeof(init), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_rc_step, dim3(nblk(nSVI, BLOCK)), dim3(BLOCK), 0, stream, nSVI, svi_dev, x_dev, dbc_dev, p_dev, pc ? pc[0] : 0.0, pc ? pc[1] : 0.0,
        pc ? pc[2] : 0.0, shape, slackness, minOut_.p);
    unsigned long long k = 0;
    minOut_.download(&k, 1, stream);
    return from_ordered_bits(k);
}

double HipRoundCollider::stepBound(int nSVI, const int* svi_dev, const double* x_dev, const int* dbc_dev, const double* p_dev, double slackness,
    double stepSize)
{
    if (!nSVI) return stepSize;
    return std::min(stepSize, rayBound(nSVI, svi_dev, x_dev, dbc_dev, p_dev, nullptr, slackness));
}

double HipRoundCollider::move(int nSVI, const int* svi_dev, const double* x_dev, const double* delta, double slackness)
{
    double stepSize = 1.0;
    if (nSVI) {
        const double rel[3] = { -delta[0], -delta[1], -delta[2] }; // the nodes as seen from the collider
        stepSize = std::min(1.0, rayBound(nSVI, svi_dev, x_dev, nullptr, nullptr, rel, slackness));
    }
    for (int c = 0; c < 3; ++c) {
        shape.p0[c] += stepSize * delta[c];
        shape.p1[c] += stepSize * delta[c];
    }
    return 1.0 - stepSize;
}

bool HipRoundCollider::intersected(int nV, const double* x_dev, const int* dbc_dev)
{
    if (!nV) return false;
    count_.alloc(1);
    count_.zero(stream);
    hipLaunchKernelGGL(k_rc_intersected, dim3(nblk(nV, BLOCK)), dim3(BLOCK), 0, stream, nV, x_dev, dbc_dev, shape, count_.p);
    int f = 0;
    count_.download(&f, 1, stream);
    return f != 0;
}

void HipRoundCollider::evalDist2(const std::vector<int>& verts, const double* x_dev, std::vector<double>& d2)
{
    const int cnt = (int)verts.size();
    d2.assign(cnt, 0.0);
    if (!cnt) return;
    ids_.upload(verts, stream);
    if (vals_.n < (size_t)cnt) vals_.alloc(cnt);
    hipLaunchKernelGGL(k_rc_dist2, dim3(nblk(cnt, BLOCK)), dim3(BLOCK), 0, stream, cnt, ids_.p, x_dev, shape, vals_.p);
    vals_.download(d2.data(), cnt, stream);
}

void HipRoundCollider::lagUpdate(const double* x_dev, double dHat, double kappa)
{
    lagSet = set;
    const int cnt = (int)lagSet.size();
    if (!cnt) return;
    d_lagSet.ensure(cnt);
    d_lagLambda.ensure(cnt);
    d_lagNormal.ensure(3 * (size_t)cnt);
    HIP_CHECK(hipMemcpyAsync(d_lagSet.p, d_set.p, cnt * sizeof(int), hipMemcpyDeviceToDevice, stream));
    hipLaunchKernelGGL(k_rc_lag, dim3(nblk(cnt, BLOCK)), dim3(BLOCK), 0, stream, cnt, d_lagSet.p, x_dev, shape, dHat, kappa, d_lagLambda.p, d_lagNormal.p);
}

double HipRoundCollider::frictionEnergy(const double* x_dev, const double* xt_dev, double eps2)
{
    const int cnt = (int)lagSet.size();
    if (!cnt) return 0.0;
    const int nb = nblk(cnt, BLOCK);
    if (partial_.n < (size_t)nb + 1) partial_.alloc(nb + 1);
    hipLaunchKernelGGL(k_rc_fric_energy, dim3(nb), dim3(BLOCK), 0, stream, cnt, d_lagSet.p, d_lagLambda.p, d_lagNormal.p, x_dev, xt_dev, friction, eps2,
        partial_.p + 1);
    launch_reduce_partials(partial_.p + 1, nb, 1.0, false, partial_.p, stream);
    double out = 0.0;
    partial_.download(&out, 1, stream);
    return out;
}

void HipRoundCollider::frictionGradientAdd(const double* x_dev, const double* xt_dev, double eps2, double* grad_dev)
{
    const int cnt = (int)lagSet.size();
    if (!cnt) return;
    hipLaunchKernelGGL(k_rc_fric_gradient, dim3(nblk(cnt, BLOCK)), dim3(BLOCK), 0, stream, cnt, d_lagSet.p, d_lagLambda.p, d_lagNormal.p, x_dev, xt_dev, friction,
        eps2, grad_dev);
}

void HipRoundCollider::frictionHessianAdd(const double* x_dev, const double* xt_dev, const int* dbc_dev, const int* rowBase_dev, const int* rowLen_dev,
    double eps2, int projectDBC, double* a_dev)
{
    const int cnt = (int)lagSet.size();
    if (!cnt) return;
    hipLaunchKernelGGL(k_rc_fric_hessian, dim3(nblk(cnt, BLOCK)), dim3(BLOCK), 0, stream, cnt, d_lagSet.p, d_lagLambda.p, d_lagNormal.p, x_dev, xt_dev, dbc_dev,
        rowBase_dev, rowLen_dev, friction, eps2, projectDBC, a_dev);
}

int HipRoundCollider::state(int nSVI, const int* svi_dev, const double* x_dev, const double* xt_dev, double dHat, double kappa, double eps2, double* out10)
{
    const int cnt = (int)set.size(), lag = (eps2 > 0.0 && friction > 0.0) ? (int)lagSet.size() : 0;
    out10[0] = INFINITY;
    for (int j = 1; j < 10; ++j) out10[j] = 0.0;
    if (nSVI) {
        minOut_.alloc(1);
        const unsigned long long init = ~0ull;
        HIP_CHECK(hipMemcpyAsync(minOut_.p, &init, sizeof(init), hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(k_rc_min_s, dim3(nblk(nSVI, BLOCK)), dim3(BLOCK), 0, stream, nSVI, svi_dev, x_dev, shape, minOut_.p);
        unsigned long long k = 0;
        minOut_.download(&k, 1, stream);
        out10[0] = from_ordered_bits(k);
    }
    const int nb = std::max(nblk(cnt, BLOCK), nblk(lag, BLOCK));
    if (!nb) return cnt;
    const size_t need = 9 + 6 * (size_t)nb; // the nine results, then the per-workgroup sums of one pass at a time
    if (partial_.n < need) partial_.alloc(need);
    HIP_CHECK(hipMemsetAsync(partial_.p, 0, 9 * sizeof(double), stream));
    if (cnt) {
        const int b = nblk(cnt, BLOCK);
        hipLaunchKernelGGL(k_rc_state, dim3(b), dim3(BLOCK), 0, stream, cnt, b, d_set.p, x_dev, shape, dHat, kappa, partial_.p + 9);
        for (int j = 0; j < 6; ++j) launch_reduce_partials(partial_.p + 9 + (size_t)j * b, b, 1.0, false, partial_.p + j, stream);
    }
    if (lag) {
        const int b = nblk(lag, BLOCK);
        hipLaunchKernelGGL(k_rc_fric_state, dim3(b), dim3(BLOCK), 0, stream, lag, b, d_lagSet.p, d_lagLambda.p, d_lagNormal.p, x_dev, xt_dev, friction, eps2,
            partial_.p + 9);
        for (int j = 0; j < 3; ++j) launch_reduce_partials(partial_.p + 9 + (size_t)j * b, b, 1.0, false, partial_.p + 6 + j, stream);
    }
    partial_.download(out10 + 1, 9, stream);
    return cnt;
}

} // namespace ipcgpu
