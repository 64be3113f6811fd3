// HipVertexCollider: what every analytic obstacle shares.  An analytic obstacle acts on single surface vertices through a signed distance; the shapes are
// the half-space (hip_halfspace.h) and the sphere / capsule (round_collider_kernels.h).  This base owns the vertex constraint set, the lagged friction
// set and the scratch buffers, and is the one interface the stepper walks.  vertex_collider.hip holds the host code and the kernel templates, written
// once and instantiated per shape; a shape supplies its distance, gradient direction, Hessian entries, lagged multiplier, step-bound candidate and
// `move`.
#pragma once
#include "common.h"
#include <vector>

namespace ipcgpu {

class HipVertexCollider {
public:
    virtual ~HipVertexCollider() = default;
    hipStream_t stream;
    std::vector<int> set; // activeSet[coI]: vertex ids, ascending surface-vertex order
    DevBuf<int> d_set;

    virtual int build(int nSVI, const int* svi_dev, const double* x_dev, const int* dbc_dev, double dHat) = 0;
    void setSet(int n, const int* verts);
    virtual double energy(const double* x_dev, double dHat, double kappa) = 0;
    virtual void gradientAdd(const double* x_dev, double dHat, double kappa, double* grad_dev) = 0;
    virtual void hessianAdd(const double* x_dev, const int* dbc_dev, const int* rowBase_dev, const int* rowLen_dev, double dHat, double kappa,
        int projectDBC, double* a_dev) = 0;
    virtual double stepBound(int nSVI, const int* svi_dev, const double* x_dev, const int* dbc_dev, const double* p_dev, double slackness,
        double stepSize) = 0;
    virtual bool intersected(int nV, const double* x_dev, const int* dbc_dev) = 0;
    // the obstacle is displaced by the largest fraction <= 1 of delta that keeps `slackness` of every surface node's distance (Dirichlet nodes
    // included); returns the fraction that is left
    virtual double move(int nSVI, const int* svi_dev, const double* x_dev, const double* delta3, double slackness) = 0;
    virtual void evalDist2(const std::vector<int>& verts, const double* x_dev, std::vector<double>& d2) = 0; // squared distance per vertex
    // lagged friction (HalfSpace.cpp:272-381, C0 clamping): activeSet_lastH / lambda_lastH of this obstacle
    double friction = 0.0; // Base::friction
    std::vector<int> lagSet;
    DevBuf<int> d_lagSet;
    DevBuf<double> d_lagLambda, d_lagNormal; // [cnt]; [3 cnt], only where the normal differs from entry to entry (never allocated by a half-space)
    void lagClear() { lagSet.clear(); }
    virtual void lagUpdate(const double* x_dev, double dHat, double kappa) = 0; // Optimizer.cpp:1560-1573 on the current `set`
    virtual double frictionEnergy(const double* x_dev, const double* xt_dev, double eps2) = 0;
    virtual void frictionGradientAdd(const double* x_dev, const double* xt_dev, double eps2, double* grad_dev) = 0;
    virtual void frictionHessianAdd(const double* x_dev, const double* xt_dev, const int* dbc_dev, const int* rowBase_dev, const int* rowLen_dev,
        double eps2, int projectDBC, double* a_dev) = 0;

protected:
    explicit HipVertexCollider(hipStream_t s) : stream(s) {}
    // the two read-backs (defined in vertex_collider.hip, for that unit alone)
    // fill(partial) launches a kernel that leaves the per-workgroup sums of cnt items: scale times their sum, in the fixed order of k_reduce_partials
    template <class Launch> double sumOf(int cnt, double scale, Launch fill);
    // fill(out) launches a kernel that takes the atomic minimum of ordered_bits into out[0]: that minimum
    template <class Launch> double minOf(Launch fill);
    DevBuf<int> flags_, count_, ids_;
    DevBuf<char> tmp_;
    DevBuf<double> partial_, vals_;
    DevBuf<unsigned long long> minOut_;
};

} // namespace ipcgpu
