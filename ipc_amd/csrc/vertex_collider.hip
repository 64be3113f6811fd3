// Analytic obstacles (vertex_collider.h): the half-space (reference lines in hip_halfspace.h) and the sphere / capsule (model in
// round_collider_kernels.h).  Per-vertex streaming work: one lane per surface vertex / per set entry, 24 B of position per vertex, the shape passed by
// value, so every kernel is a single coalesced pass bounded by HBM latency at the sizes of the hot path (<= 45 K surface vertices at mat150).  Beside
// the plane a round collider's lane pays one fp64 square root and one division for the distance (rc_eval), and the step bound up to three more of each.
// Layout: the shapes' device functions (overloads on hsdev::Plane and RoundShape: their arithmetic differs in association and stays apart), the kernel
// templates, the host template Collider<Host>, and what only one shape has (`move`, the round collider's `state`).  Compiled with -ffp-contract=off.
#include "hip_halfspace.h"
#include "round_collider_kernels.h"
#include "contact_device.h"
#include "halfspace_device.h"
#include "device_prims.h"
#include <cmath>
#include <type_traits>
#include <utility>
#include <hipcub/hipcub.hpp>

namespace ipcgpu {
namespace {
constexpr int BLOCK = 256;
constexpr double NO_BOUND = 1.0e300;

using namespace prims;
using hsdev::Plane;
using hsdev::plane_dist;

// ---- the half-space -------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double signed_dist(const Plane& h, const double* __restrict__ x, int v) { return plane_dist(h, x, v); }
__device__ __forceinline__ bool touches(const Plane& h, const double* __restrict__ x, int v) // CollisionObject.h:386-401
{
    const double dist = plane_dist(h, x, v);
    return dist * dist <= 0.0;
}
__device__ __forceinline__ void barrier_gradient(const Plane& h, const double* __restrict__ x, int v, double dHat, double kappa, double* g)
{
    const double dist = plane_dist(h, x, v);
    double b, gb, Hb;
    cdev::barrier(dist * dist, dHat, &b, &gb, &Hb);
    g[0] = kappa * gb * 2.0 * dist * h.n0;
    g[1] = kappa * gb * 2.0 * dist * h.n1;
    g[2] = kappa * gb * 2.0 * dist * h.n2;
}
// false: nothing to add
__device__ __forceinline__ bool barrier_hessian(const Plane& h, const double* __restrict__ x, int v, double dHat, double kappa, double* h6)
{
    const double dist = plane_dist(h, x, v), d = dist * dist;
    double b, gb, Hb;
    cdev::barrier(d, dHat, &b, &gb, &Hb);
    const double param = 4.0 * Hb * d + 2.0 * gb;
    if (!(param > 0.0)) return false;
    const double nn[3] = { h.n0, h.n1, h.n2 };
    h6[0] = kappa * param * nn[0] * nn[0];
    h6[1] = kappa * param * nn[0] * nn[1];
    h6[2] = kappa * param * nn[0] * nn[2];
    h6[3] = kappa * param * nn[1] * nn[1];
    h6[4] = kappa * param * nn[1] * nn[2];
    h6[5] = kappa * param * nn[2] * nn[2];
    return true;
}
// the lagged multiplier; nn: the lagged normal (the plane's own, which no kernel stores)
__device__ __forceinline__ double lag_entry(const Plane& h, const double* __restrict__ x, int v, double dHat, double kappa, double* nn)
{
    const double dist = plane_dist(h, x, v), d = dist * dist;
    double b, gb, Hb;
    cdev::barrier(d, dHat, &b, &gb, &Hb);
    nn[0] = h.n0;
    nn[1] = h.n1;
    nn[2] = h.n2;
    return gb * (-kappa * 2.0 * sqrt(d)); // Optimizer.cpp:1563-1566
}
__device__ __forceinline__ double idle_bound(const Plane&) { return 1.0; }
__device__ __forceinline__ double step_candidate(const Plane& h, const double* __restrict__ x, int v, const double* p, double slackness)
{
    const double coef = h.n0 * p[0] + h.n1 * p[1] + h.n2 * p[2];
    return coef < 0.0 ? -plane_dist(h, x, v) / coef * slackness : 1.0;
}

// ---- the round collider ---------------------------------------------------------------------------------------------------------------------------------
// distance, normal and region of one vertex: THE evaluation every function below calls
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
__device__ __forceinline__ double signed_dist(const RoundShape& c, const double* __restrict__ x, int v) { return rc_eval(c, x, v).s; }
__device__ __forceinline__ bool touches(const RoundShape& c, const double* __restrict__ x, int v) { return rc_eval(c, x, v).s <= 0.0; }
__device__ __forceinline__ void barrier_gradient(const RoundShape& c, const double* __restrict__ x, int v, double dHat, double kappa, double* g)
{
    const RoundEval e = rc_eval(c, x, v);
    double b, gb, Hb;
    cdev::barrier(e.s * e.s, dHat, &b, &gb, &Hb);
    const double f = kappa * gb * 2.0 * e.s * c.side;
    g[0] = f * e.m[0];
    g[1] = f * e.m[1];
    g[2] = f * e.m[2];
}
__device__ __forceinline__ bool barrier_hessian(const RoundShape& c, const double* __restrict__ x, int v, double dHat, double kappa, double* h6)
{
    const RoundEval e = rc_eval(c, x, v);
    const double d = e.s * e.s;
    double b, gb, Hb;
    cdev::barrier(d, dHat, &b, &gb, &Hb);
    // the two eigenvalue coefficients, clamped at 0: the PSD projection in closed form
    double c1 = 4.0 * Hb * d + 2.0 * gb, c2 = 2.0 * gb * e.s * c.side * e.invr;
    if (!(c1 > 0.0)) c1 = 0.0;
    if (!(c2 > 0.0)) c2 = 0.0;
    if (c1 == 0.0 && c2 == 0.0) return false;
    c1 *= kappa;
    c2 *= kappa;
    const double ax = e.sideRegion ? 1.0 : 0.0;
    const double* m = e.m;
    const double* ua = c.axis;
    h6[0] = c1 * (m[0] * m[0]) + c2 * (1.0 - m[0] * m[0] - ax * (ua[0] * ua[0]));
    h6[1] = c1 * (m[0] * m[1]) + c2 * (-(m[0] * m[1]) - ax * (ua[0] * ua[1]));
    h6[2] = c1 * (m[0] * m[2]) + c2 * (-(m[0] * m[2]) - ax * (ua[0] * ua[2]));
    h6[3] = c1 * (m[1] * m[1]) + c2 * (1.0 - m[1] * m[1] - ax * (ua[1] * ua[1]));
    h6[4] = c1 * (m[1] * m[2]) + c2 * (-(m[1] * m[2]) - ax * (ua[1] * ua[2]));
    h6[5] = c1 * (m[2] * m[2]) + c2 * (1.0 - m[2] * m[2] - ax * (ua[2] * ua[2]));
    return true;
}
__device__ __forceinline__ double lag_entry(const RoundShape& c, const double* __restrict__ x, int v, double dHat, double kappa, double* nn)
{
    const RoundEval e = rc_eval(c, x, v);
    double b, gb, Hb;
    cdev::barrier(e.s * e.s, dHat, &b, &gb, &Hb);
    nn[0] = c.side * e.m[0];
    nn[1] = c.side * e.m[1];
    nn[2] = c.side * e.m[2];
    return gb * (-kappa * 2.0 * e.s);
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
__device__ __forceinline__ double idle_bound(const RoundShape&) { return NO_BOUND; }
__device__ __forceinline__ double step_candidate(const RoundShape& c, const double* __restrict__ x, int v, const double* p, double slackness)
{
    return rc_ray(c, x[3 * (size_t)v], x[3 * (size_t)v + 1], x[3 * (size_t)v + 2], p, slackness);
}

// ---- where the friction kernels take the normal of entry i from ------------------------------------------------------------------------------------------
struct UniformNormal { // the plane's, passed by value: nothing is stored or loaded per entry
    static constexpr bool PER_ENTRY = false;
    double n0, n1, n2;
    __device__ __forceinline__ void load(int, double* nn) const
    {
        nn[0] = n0;
        nn[1] = n1;
        nn[2] = n2;
    }
    __device__ __forceinline__ void store(int, const double*) const {}
};
struct LaggedNormal { // d_lagNormal: the unit normal of every entry at lag time
    static constexpr bool PER_ENTRY = true;
    double* p;
    __device__ __forceinline__ void load(int i, double* nn) const
    {
        nn[0] = p[3 * (size_t)i];
        nn[1] = p[3 * (size_t)i + 1];
        nn[2] = p[3 * (size_t)i + 2];
    }
    __device__ __forceinline__ void store(int i, const double* nn) const
    {
        p[3 * (size_t)i] = nn[0];
        p[3 * (size_t)i + 1] = nn[1];
        p[3 * (size_t)i + 2] = nn[2];
    }
};

// ---- barrier kernels ---------------------------------------------------------------------------------------------------------------------------------------
template <class Shape>
__global__ __launch_bounds__(BLOCK) void k_vc_flags(int nSVI, const int* __restrict__ svi, const double* __restrict__ x, const int* __restrict__ dbc, Shape c,
    double dHat, int* __restrict__ flags)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nSVI) return;
    const int v = svi[i];
    const double dist = signed_dist(c, x, v);
    flags[i] = (dbc[v] == 0 && dist * dist < dHat) ? 1 : 0;
}

template <class Shape>
__global__ __launch_bounds__(BLOCK) void k_vc_energy(int n, const int* __restrict__ set, const double* __restrict__ x, Shape c, double dHat,
    double* __restrict__ partial)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    double val = 0.0;
    if (i < n) {
        const double dist = signed_dist(c, x, set[i]);
        double b, gb, Hb;
        cdev::barrier(dist * dist, dHat, &b, &gb, &Hb);
        val = b;
    }
    store_block_sum<BLOCK>(val, partial);
}

template <class Shape>
__global__ __launch_bounds__(BLOCK) void k_vc_gradient(int n, const int* __restrict__ set, const double* __restrict__ x, Shape c, double dHat, double kappa,
    double* __restrict__ grad)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int v = set[i]; // vertices of one set are distinct: plain read-modify-write
    double g[3];
    barrier_gradient(c, x, v, dHat, kappa, g);
    grad[3 * (size_t)v] += g[0];
    grad[3 * (size_t)v + 1] += g[1];
    grad[3 * (size_t)v + 2] += g[2];
}

template <class Shape>
__global__ __launch_bounds__(BLOCK) void k_vc_hessian(int n, const int* __restrict__ set, const double* __restrict__ x, const int* __restrict__ dbc,
    const int* __restrict__ rowBase, const int* __restrict__ rowLen, Shape c, double dHat, double kappa, int projectDBC, double* __restrict__ a)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int v = set[i];
    if (dbc[v] != 0 && projectDBC) return;
    double h6[6];
    if (!barrier_hessian(c, x, v, dHat, kappa, h6)) return;
    add_diag_block(a, rowBase[v], rowLen[v], h6); // only the node's diagonal block (LinSysSolver.hpp:63-111)
}

// p_dev: one direction per node, bounded by the nodes with dbc == 0; p_dev == nullptr: the constant direction pc for every surface node (a round
// collider's move)
template <class Shape>
__global__ __launch_bounds__(BLOCK) void k_vc_step(int nSVI, const int* __restrict__ svi, const double* __restrict__ x, const int* __restrict__ dbc,
    const double* __restrict__ p_dev, double pc0, double pc1, double pc2, Shape c, double slackness, unsigned long long* __restrict__ out)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    double best = idle_bound(c);
    if (i < nSVI) {
        const int v = svi[i];
        if (!p_dev || dbc[v] == 0) {
            double p[3] = { pc0, pc1, pc2 };
            if (p_dev) {
                p[0] = p_dev[3 * (size_t)v];
                p[1] = p_dev[3 * (size_t)v + 1];
                p[2] = p_dev[3 * (size_t)v + 2];
            }
            best = step_candidate(c, x, v, p, slackness);
        }
    }
    atomic_min_wave(best, out);
}

// the plane moves by delta: every surface node (Dirichlet or not) bounds the fraction, coef = n . (-delta) is the same for all (HalfSpace.cpp:393-411)
__global__ __launch_bounds__(BLOCK) void k_hs_move(int nSVI, const int* __restrict__ svi, const double* __restrict__ x, Plane h, double coef, double slackness,
    unsigned long long* __restrict__ out)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    double best = 1.0;
    if (i < nSVI) best = -plane_dist(h, x, svi[i]) / coef * slackness;
    atomic_min_wave(best, out);
}

template <class Shape>
__global__ __launch_bounds__(BLOCK) void k_vc_intersected(int nV, const double* __restrict__ x, const int* __restrict__ dbc, Shape c, int* __restrict__ flag)
{
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= nV || dbc[v] != 0) return;
    if (touches(c, x, v)) flag[0] = 1;
}

template <class Shape>
__global__ __launch_bounds__(BLOCK) void k_vc_dist2(int n, const int* __restrict__ verts, const double* __restrict__ x, Shape c, double* __restrict__ out)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const double dist = signed_dist(c, x, verts[i]);
    out[i] = dist * dist;
}

template <class Shape>
__global__ __launch_bounds__(BLOCK) void k_vc_min_dist(int nSVI, const int* __restrict__ svi, const double* __restrict__ x, Shape c, unsigned long long* __restrict__ out)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    double best = INFINITY;
    if (i < nSVI) best = signed_dist(c, x, svi[i]);
    atomic_min_wave(best, out);
}

// ---- lagged friction (HalfSpace.cpp:272-381), the normal of an entry from a NormalSrc ---------------------------------------------------------------------
template <class Shape, class NormalSrc>
__global__ __launch_bounds__(BLOCK) void k_vc_lag(int n, const int* __restrict__ set, const double* __restrict__ x, Shape c, double dHat, double kappa,
    double* __restrict__ lambda, NormalSrc normal)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    double nn[3];
    lambda[i] = lag_entry(c, x, set[i], dHat, kappa, nn);
    normal.store(i, nn);
}
// the tangential part of the displacement x - x^t of node v
__device__ __forceinline__ void fric_proj(const double* nn, const double* __restrict__ x, const double* __restrict__ xt, int v, double* vp)
{
    const double vd[3] = { x[3 * (size_t)v] - xt[3 * (size_t)v], x[3 * (size_t)v + 1] - xt[3 * (size_t)v + 1], x[3 * (size_t)v + 2] - xt[3 * (size_t)v + 2] };
    const double dn = vd[0] * nn[0] + vd[1] * nn[1] + vd[2] * nn[2];
    vp[0] = vd[0] - dn * nn[0];
    vp[1] = vd[1] - dn * nn[1];
    vp[2] = vd[2] - dn * nn[2];
}
template <class NormalSrc>
__global__ __launch_bounds__(BLOCK) void k_vc_fric_energy(int n, const int* __restrict__ set, const double* __restrict__ lambda, NormalSrc normal,
    const double* __restrict__ x, const double* __restrict__ xt, double mu, double eps2, double* __restrict__ partial)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    double val = 0.0;
    if (i < n) {
        double nn[3], vp[3];
        normal.load(i, nn);
        fric_proj(nn, x, xt, set[i], vp);
        const double m2 = vp[0] * vp[0] + vp[1] * vp[1] + vp[2] * vp[2], eps = sqrt(eps2);
        val = (m2 > eps2) ? mu * lambda[i] * (sqrt(m2) - eps * 0.5) : mu * lambda[i] * m2 / eps * 0.5;
    }
    store_block_sum<BLOCK>(val, partial);
}
// the friction gradient of entry i: sc vp
template <class NormalSrc>
__device__ __forceinline__ double fric_force(int i, const int* __restrict__ set, const double* __restrict__ lambda, const NormalSrc& normal,
    const double* __restrict__ x, const double* __restrict__ xt, double mu, double eps2, double* vp)
{
    double nn[3];
    normal.load(i, nn);
    fric_proj(nn, x, xt, set[i], vp);
    const double m2 = vp[0] * vp[0] + vp[1] * vp[1] + vp[2] * vp[2];
    return (m2 > eps2) ? mu * lambda[i] / sqrt(m2) : mu * lambda[i] / sqrt(eps2);
}
template <class NormalSrc>
__global__ __launch_bounds__(BLOCK) void k_vc_fric_gradient(int n, const int* __restrict__ set, const double* __restrict__ lambda, NormalSrc normal,
    const double* __restrict__ x, const double* __restrict__ xt, double mu, double eps2, double* __restrict__ grad)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int v = set[i];
    double vp[3];
    const double sc = fric_force(i, set, lambda, normal, x, xt, mu, eps2, vp);
    for (int k = 0; k < 3; ++k) grad[3 * (size_t)v + k] += sc * vp[k];
}
// sliding: ml/|v| (P - vhat vhat^T) with P = I - n n^T has eigenvalues {ml/|v|, 0, 0}: the reference's makePD (HalfSpace.cpp:356)
// is the identity up to round-off; sticking: ml/eps P ("already SPD", :360)
template <class NormalSrc>
__global__ __launch_bounds__(BLOCK) void k_vc_fric_hessian(int n, const int* __restrict__ set, const double* __restrict__ lambda, NormalSrc normal,
    const double* __restrict__ x, const double* __restrict__ xt, const int* __restrict__ dbc, const int* __restrict__ rowBase, const int* __restrict__ rowLen,
    double mu, double eps2, int projectDBC, double* __restrict__ a)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int v = set[i];
    if (projectDBC && dbc[v] != 0) return;
    const double ml = mu * lambda[i];
    double nn[3], vp[3];
    normal.load(i, nn);
    fric_proj(nn, x, xt, v, vp);
    const double m2 = vp[0] * vp[0] + vp[1] * vp[1] + vp[2] * vp[2];
    double h6[6];
    int e = 0;
    if (m2 > eps2) {
        const double mag = sqrt(m2);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int k = r; k < 3; ++k) h6[e++] = vp[r] * (-ml / m2 / mag) * vp[k] + ((r == k ? 1.0 : 0.0) - nn[r] * nn[k]) * (ml / mag);
    }
    else {
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int k = r; k < 3; ++k) h6[e++] = ((r == k ? 1.0 : 0.0) - nn[r] * nn[k]) * (ml / sqrt(eps2));
    }
    add_diag_block(a, rowBase[v], rowLen[v], h6);
}

// ---- state query of a round collider: per-workgroup sums in a fixed order ---------------------------------------------------------------------------------
// partial[j * nb + block] = the sum of q[j] over the workgroup, j = 0..N-1
template <int N>
__device__ __forceinline__ void store_block_sums(const double* q, int nb, double* __restrict__ partial)
{
    __shared__ double sm[BLOCK / 64];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const double r = block_sum<BLOCK>(q[j], sm);
        if (threadIdx.x == 0) partial[(size_t)j * nb + blockIdx.x] = r;
        __syncthreads();
    }
}
// j = 0..2 the barrier force on the bodies (minus the gradient), j = 3..5 its torque about p0
__global__ __launch_bounds__(BLOCK) void k_rc_state(int n, int nb, const int* __restrict__ set, const double* __restrict__ x, RoundShape c, double dHat, double kappa,
    double* __restrict__ partial)
{
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
    store_block_sums<6>(q, nb, partial);
}
// j = 0..2: the lagged friction force on the bodies (minus the friction gradient)
template <class NormalSrc>
__global__ __launch_bounds__(BLOCK) void k_vc_fric_state(int n, int nb, const int* __restrict__ set, const double* __restrict__ lambda, NormalSrc normal,
    const double* __restrict__ x, const double* __restrict__ xt, double mu, double eps2, double* __restrict__ partial)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    double q[3] = { 0.0, 0.0, 0.0 };
    if (i < n) {
        double vp[3];
        const double sc = fric_force(i, set, lambda, normal, x, xt, mu, eps2, vp);
        for (int k = 0; k < 3; ++k) q[k] = -(sc * vp[k]);
    }
    store_block_sums<3>(q, nb, partial);
}

template <class... KArgs, class... Args>
void launch(void (*kernel)(KArgs...), int n, hipStream_t stream, Args... args)
{
    hipLaunchKernelGGL(kernel, dim3(nblk(n, BLOCK)), dim3(BLOCK), 0, stream, args...);
}
} // namespace

// ---- the host scaffold ---------------------------------------------------------------------------------------------------------------------------------------
template <class Launch>
double HipVertexCollider::sumOf(int cnt, double scale, Launch fill)
{
    const int nb = nblk(cnt, BLOCK);
    if (partial_.n < (size_t)nb + 1) partial_.alloc(nb + 1);
    fill(partial_.p + 1);
    launch_reduce_partials(partial_.p + 1, nb, scale, false, partial_.p, stream);
    double out = 0.0;
    partial_.download(&out, 1, stream);
    return out;
}

template <class Launch>
double HipVertexCollider::minOf(Launch fill)
{
    minOut_.alloc(1);
    const unsigned long long init = ~0ull;
    HIP_CHECK(hipMemcpyAsync(minOut_.p, &init, sizeof(init), hipMemcpyHostToDevice, stream));
    fill(minOut_.p);
    unsigned long long k = 0;
    minOut_.download(&k, 1, stream);
    return from_ordered_bits(k);
}

void HipVertexCollider::setSet(int cnt, const int* verts)
{
    set.assign(verts, verts + cnt);
    if (d_set.n < (size_t)cnt) d_set.alloc(cnt);
    if (cnt) HIP_CHECK(hipMemcpyAsync(d_set.p, set.data(), cnt * sizeof(int), hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
}

namespace {
// what the kernels take by value
Plane deviceShape(const HipHalfSpace& h) { return Plane{ h.n[0], h.n[1], h.n[2], h.D }; }
const RoundShape& deviceShape(const HipRoundCollider& h) { return h.shape; }
UniformNormal normalSrc(const HipHalfSpace& h) { return UniformNormal{ h.n[0], h.n[1], h.n[2] }; }
LaggedNormal normalSrc(const HipRoundCollider& h) { return LaggedNormal{ h.d_lagNormal.p }; }

// Host: HipHalfSpace or HipRoundCollider, which hold the shape's own parameters
template <class Host>
class Collider final : public Host {
    using Shape = std::decay_t<decltype(deviceShape(std::declval<const Host&>()))>;
    using NormalSrc = decltype(normalSrc(std::declval<const Host&>()));
    using Host::count_; // (a dependent base: every member of HipVertexCollider used below is named here)
    using Host::d_lagLambda;
    using Host::d_lagNormal;
    using Host::d_lagSet;
    using Host::d_set;
    using Host::flags_;
    using Host::friction;
    using Host::ids_;
    using Host::lagSet;
    using Host::minOf;
    using Host::set;
    using Host::stream;
    using Host::sumOf;
    using Host::tmp_;
    using Host::vals_;
    Shape dev() const { return deviceShape(*this); }
    double bound(int nSVI, const int* svi_dev, const double* x_dev, const int* dbc_dev, const double* p_dev, const double* pc, double slackness)
    {
        return minOf([&](unsigned long long* out) {
            launch(k_vc_step<Shape>, nSVI, stream, nSVI, svi_dev, x_dev, dbc_dev, p_dev, pc ? pc[0] : 0.0, pc ? pc[1] : 0.0, pc ? pc[2] : 0.0, dev(), slackness, out);
        });
    }

public:
    template <class... A>
    explicit Collider(A&&... a) : Host(std::forward<A>(a)...) {}

    int build(int nSVI, const int* svi_dev, const double* x_dev, const int* dbc_dev, double dHat) override
    {
        set.clear();
        if (!nSVI) return 0;
        flags_.alloc(nSVI);
        d_set.alloc(nSVI);
        count_.alloc(1);
        launch(k_vc_flags<Shape>, nSVI, stream, nSVI, svi_dev, x_dev, dbc_dev, dev(), dHat, flags_.p);
        size_t bytes = 0; // order-preserving compaction: the set comes out in ascending surface-vertex order like the reference's
        auto select = [&](void* tmp) { HIP_CHECK(hipcub::DeviceSelect::Flagged(tmp, bytes, svi_dev, flags_.p, d_set.p, count_.p, nSVI, stream)); };
        select(nullptr); // the size query
        if (tmp_.n < bytes) tmp_.alloc(bytes);
        select(tmp_.p);
        int cnt = 0;
        count_.download(&cnt, 1, stream);
        set.resize(cnt);
        if (cnt) d_set.download(set.data(), cnt, stream);
        return cnt;
    }

    double energy(const double* x_dev, double dHat, double kappa) override
    {
        const int cnt = (int)set.size();
        if (!cnt) return 0.0;
        return sumOf(cnt, kappa, [&](double* partial) { launch(k_vc_energy<Shape>, cnt, stream, cnt, d_set.p, x_dev, dev(), dHat, partial); });
    }

    void gradientAdd(const double* x_dev, double dHat, double kappa, double* grad_dev) override
    {
        const int cnt = (int)set.size();
        if (cnt) launch(k_vc_gradient<Shape>, cnt, stream, cnt, d_set.p, x_dev, dev(), dHat, kappa, grad_dev);
    }

    void hessianAdd(const double* x_dev, const int* dbc_dev, const int* rowBase_dev, const int* rowLen_dev, double dHat, double kappa, int projectDBC,
        double* a_dev) override
    {
        const int cnt = (int)set.size();
        if (cnt) launch(k_vc_hessian<Shape>, cnt, stream, cnt, d_set.p, x_dev, dbc_dev, rowBase_dev, rowLen_dev, dev(), dHat, kappa, projectDBC, a_dev);
    }

    double stepBound(int nSVI, const int* svi_dev, const double* x_dev, const int* dbc_dev, const double* p_dev, double slackness, double stepSize) override
    {
        if (!nSVI) return stepSize;
        return std::min(stepSize, bound(nSVI, svi_dev, x_dev, dbc_dev, p_dev, nullptr, slackness));
    }

    double move(int nSVI, const int* svi_dev, const double* x_dev, const double* delta, double slackness) override; // per shape, below

    bool intersected(int nV, const double* x_dev, const int* dbc_dev) override
    {
        if (!nV) return false;
        count_.alloc(1);
        count_.zero(stream);
        launch(k_vc_intersected<Shape>, nV, stream, nV, x_dev, dbc_dev, dev(), count_.p);
        int f = 0;
        count_.download(&f, 1, stream);
        return f != 0;
    }

    void evalDist2(const std::vector<int>& verts, const double* x_dev, std::vector<double>& d2) override
    {
        const int cnt = (int)verts.size();
        d2.assign(cnt, 0.0);
        if (!cnt) return;
        ids_.upload(verts, stream);
        if (vals_.n < (size_t)cnt) vals_.alloc(cnt);
        launch(k_vc_dist2<Shape>, cnt, stream, cnt, ids_.p, x_dev, dev(), vals_.p);
        vals_.download(d2.data(), cnt, stream);
    }

    void lagUpdate(const double* x_dev, double dHat, double kappa) override
    {
        lagSet = set;
        const int cnt = (int)lagSet.size();
        if (!cnt) return;
        d_lagSet.ensure(cnt);
        d_lagLambda.ensure(cnt);
        if (NormalSrc::PER_ENTRY) d_lagNormal.ensure(3 * (size_t)cnt);
        HIP_CHECK(hipMemcpyAsync(d_lagSet.p, d_set.p, cnt * sizeof(int), hipMemcpyDeviceToDevice, stream));
        launch(k_vc_lag<Shape, NormalSrc>, cnt, stream, cnt, d_lagSet.p, x_dev, dev(), dHat, kappa, d_lagLambda.p, normalSrc(*this));
    }

    double frictionEnergy(const double* x_dev, const double* xt_dev, double eps2) override
    {
        const int cnt = (int)lagSet.size();
        if (!cnt) return 0.0;
        return sumOf(cnt, 1.0, [&](double* partial) {
            launch(k_vc_fric_energy<NormalSrc>, cnt, stream, cnt, d_lagSet.p, d_lagLambda.p, normalSrc(*this), x_dev, xt_dev, friction, eps2, partial);
        });
    }

    void frictionGradientAdd(const double* x_dev, const double* xt_dev, double eps2, double* grad_dev) override
    {
        const int cnt = (int)lagSet.size();
        if (cnt) launch(k_vc_fric_gradient<NormalSrc>, cnt, stream, cnt, d_lagSet.p, d_lagLambda.p, normalSrc(*this), x_dev, xt_dev, friction, eps2, grad_dev);
    }

    void frictionHessianAdd(const double* x_dev, const double* xt_dev, const int* dbc_dev, const int* rowBase_dev, const int* rowLen_dev, double eps2,
        int projectDBC, double* a_dev) override
    {
        const int cnt = (int)lagSet.size();
        if (cnt)
            launch(k_vc_fric_hessian<NormalSrc>, cnt, stream, cnt, d_lagSet.p, d_lagLambda.p, normalSrc(*this), x_dev, xt_dev, dbc_dev, rowBase_dev, rowLen_dev,
                friction, eps2, projectDBC, a_dev);
    }
};

// HalfSpace::move (HalfSpace.cpp:389-416)
template <>
double Collider<HipHalfSpace>::move(int nSVI, const int* svi_dev, const double* x_dev, const double* delta, double slackness)
{
    const double coef = -(n[0] * delta[0] + n[1] * delta[1] + n[2] * delta[2]);
    double stepSize = 1.0;
    if (coef < 0.0 && nSVI) // going towards the object
        stepSize = std::min(1.0, minOf([&](unsigned long long* out) { launch(k_hs_move, nSVI, stream, nSVI, svi_dev, x_dev, dev(), coef, slackness, out); }));
    for (int c = 0; c < 3; ++c) origin[c] += stepSize * delta[c];
    D = -(n[0] * origin[0] + n[1] * origin[1] + n[2] * origin[2]); // init(origin + stepSize * deltaX, normal, ...), HalfSpace.cpp:413
    return 1.0 - stepSize;
}

template <>
double Collider<HipRoundCollider>::move(int nSVI, const int* svi_dev, const double* x_dev, const double* delta, double slackness)
{
    double stepSize = 1.0;
    if (nSVI) {
        const double rel[3] = { -delta[0], -delta[1], -delta[2] }; // the nodes as seen from the collider
        stepSize = std::min(1.0, bound(nSVI, svi_dev, x_dev, nullptr, nullptr, rel, slackness));
    }
    for (int c = 0; c < 3; ++c) {
        shape.p0[c] += stepSize * delta[c];
        shape.p1[c] += stepSize * delta[c];
    }
    return 1.0 - stepSize;
}
} // namespace

HipHalfSpace::HipHalfSpace(hipStream_t s, const double* origin, const double* normal) : HipVertexCollider(s)
{
    const double len = std::sqrt(normal[0] * normal[0] + normal[1] * normal[1] + normal[2] * normal[2]);
    if (!(len > 0.0)) throw ArgError("half-space normal must be non-zero");
    for (int c = 0; c < 3; ++c) n[c] = normal[c] / len;
    for (int c = 0; c < 3; ++c) this->origin[c] = origin[c];
    D = -(n[0] * origin[0] + n[1] * origin[1] + n[2] * origin[2]);
}

std::unique_ptr<HipHalfSpace> HipHalfSpace::create(hipStream_t s, const double* origin3, const double* normal3)
{
    return std::unique_ptr<HipHalfSpace>(new Collider<HipHalfSpace>(s, origin3, normal3));
}

std::unique_ptr<HipRoundCollider> HipRoundCollider::create(hipStream_t s, const RoundShape& shape)
{
    return std::unique_ptr<HipRoundCollider>(new Collider<HipRoundCollider>(s, shape));
}

int HipRoundCollider::state(int nSVI, const int* svi_dev, const double* x_dev, const double* xt_dev, double dHat, double kappa, double eps2, double* out10)
{
    const int cnt = (int)set.size(), lag = (eps2 > 0.0 && friction > 0.0) ? (int)lagSet.size() : 0;
    out10[0] = INFINITY;
    for (int j = 1; j < 10; ++j) out10[j] = 0.0;
    if (nSVI) out10[0] = minOf([&](unsigned long long* out) { launch(k_vc_min_dist<RoundShape>, nSVI, stream, nSVI, svi_dev, x_dev, shape, out); });
    const int nb = std::max(nblk(cnt, BLOCK), nblk(lag, BLOCK));
    if (!nb) return cnt;
    const size_t need = 9 + 6 * (size_t)nb; // the nine results, then the per-workgroup sums of one pass at a time
    if (partial_.n < need) partial_.alloc(need);
    HIP_CHECK(hipMemsetAsync(partial_.p, 0, 9 * sizeof(double), stream));
    if (cnt) {
        const int b = nblk(cnt, BLOCK);
        launch(k_rc_state, cnt, stream, cnt, b, d_set.p, x_dev, shape, dHat, kappa, partial_.p + 9);
        for (int j = 0; j < 6; ++j) launch_reduce_partials(partial_.p + 9 + (size_t)j * b, b, 1.0, false, partial_.p + j, stream);
    }
    if (lag) {
        const int b = nblk(lag, BLOCK);
        launch(k_vc_fric_state<LaggedNormal>, lag, stream, lag, b, d_lagSet.p, d_lagLambda.p, LaggedNormal{ d_lagNormal.p }, x_dev, xt_dev, friction, eps2, partial_.p + 9);
        for (int j = 0; j < 3; ++j) launch_reduce_partials(partial_.p + 9 + (size_t)j * b, b, 1.0, false, partial_.p + 6 + j, stream);
    }
    partial_.download(out10 + 1, 9, stream);
    return cnt;
}

} // namespace ipcgpu
