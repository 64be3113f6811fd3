// Plastic flow of tetrahedral bodies (gfx950, fp64): yield, creep and isotropic hardening -- a dented can, a bent bracket, putty, stress relaxation under
// a held grip.  A project extension: the reference has none (every body of it returns to its rest shape).  The host side (validation, the parameter
// arrays) is plastic_plan.h.
//
// Every elastic kernel reads the rest configuration of element t from A_t (restTriInv, ElemView::A, SoA [9][nT]) and from nothing else, so multiplicative
// plasticity F = F_e F_p is a rewrite of A_t = X0_t^-1 F_p^-1 at the end of a time step: the energy, gradient, Hessian, patch-assembly, stress, report and
// damping kernels stay as they are and see the new rest shape from the next step on.
// Per tetrahedron t with plasticity on (yield_t < +inf), at positions x and for a time step dt:
//     F = Ds(x) A_t                                the ELASTIC deformation gradient (A_t already holds the inverse plastic part)
//     F = U diag(s) V^T                            svd3 of nh_device.h: |s0| >= |s1| >= |s2|, only s2 may be negative
//     s2 <= 0 (flat or inverted: reachable under FCR / SNH; or not a number): the element is SKIPPED this step and counted; nothing is written
//     e_i = ln s_i,  d_i = e_i - (e_0 + e_1 + e_2) / 3,  n = |d|_2                    the norm of the deviatoric Hencky strain
//     y = yield_t + harden_t alpha_t               the current yield strain; alpha_t >= 0 is the accumulated plastic strain
//     n <= y: nothing is written -- the nine doubles of A_t and alpha_t keep their bits.  (Pure dilation has n = 0 and is rejected here, before any division
//             by n, also at yield = 0.)
//     Delta = r (n - y) / (1 + harden_t),  r = -expm1(-creep_t dt)                     creep = +inf: r = 1, the rate-independent return onto the yield surface
//     G = V diag(exp(-Delta d_i / n)) V^T,  A_t <- A_t G,  alpha_t <- alpha_t + Delta
//   The new elastic strain is d (1 - Delta / n) and the new yield strain y + harden Delta, so the excess n - y shrinks by exactly 1 - r = exp(-creep dt) per
//   flow, whatever harden is.  det G = 1 (sum d_i = 0): the rest volume (d_vol), the lumped masses and det F do not change -- the flow is isochoric and never
//   creates an inversion.  G is an isotropic function of C = F^T F: well defined where singular values coincide, although V is not.
// CHOOSING THE YIELD STRAIN.  For small strains the von Mises stress (ipcgpu_elastic_stress) is sqrt(6) mu n, so a material with yield stress sigma_y and
//   shear modulus mu = E / (2 (1 + nu)) has yield = sigma_y / (sqrt(6) mu).  harden is dimensionless (yield strain gained per unit of plastic strain);
//   creep is 1 / time: the excess decays like exp(-creep t) under a held deformation.
// NOT modelled: volumetric (pressure-dependent) yield;  kinematic hardening;  a cap on the plastic strain;  plastic work as heat;  rods and attachments
//   (their rest records do not flow; the shells have a flow of their own, shell_plastic_kernels.h);  sharded contexts (refused both ways round, as for aero).
//
// k_plastic_flow: one lane per tetrahedron of [tetBegin, tetEnd).  Coalesced SoA loads of A, the three parameters and alpha, the four-node gather of the
// element kernels, svd3, three log, three exp, two 3 x 3 products; nine coalesced stores plus alpha from the lanes that yielded and from no other.  fp64
// throughout with the exact log / exp / expm1 (the fast_* seeds of nh_device.h are for the Jacobi iterations alone).  The two counters (PC_YIELDED,
// PC_SKIPPED: scalar_slots.h) are integer atomics -- a ballot per wave, the waves of a workgroup in LDS, one add per workgroup to device memory --; there
// is no floating-point atomic: the same state gives the same bits.
// k_plastic_state (read-only): n, y and alpha per element, and per workgroup the maximum of alpha and the sum of vol alpha, reduced in a fixed order
// (device_prims.h).  These two totals are functions of the state alone, so they are computed here, when somebody asks, not on the stepper's path.
#pragma once
#include <hip/hip_runtime.h>

namespace ipcgpu {

struct PlasticView {
    int nT;
    int tetBegin, tetEnd; // the elements the flow visits
    const double* x; // positions, xyz interleaved
    const int4* tet; // nT
    double* A; // restTriInv, SoA [9][nT]: read, and rewritten by the lanes that yield
    const double* vol; // nT rest volumes (never written: det G = 1)
    const double* yield; // nT; +inf: off
    const double* creep; // nT; +inf: rate-independent
    const double* harden; // nT
    double* alpha; // nT accumulated plastic strain
    double dt;
};

// One flow at v.x.  counts (device, PC_COUNT ints, zeroed by the caller): += the elements that yielded / were skipped.
void launch_plastic_flow(const PlasticView& v, int* counts, hipStream_t s);
int plastic_state_blocks(const PlasticView& v); // partial sums per quantity that launch_plastic_state writes
// perElem (nullable; column-major nT x 3): n, y, alpha of every element at v.x -- n = NaN where the flow would skip the element; y = +inf where plasticity
// is off (n is given all the same: it shows where the body would yield).  totals2 (nullable; device, PT_COUNT doubles): the maximum of alpha and the
// sum of vol alpha over ALL elements.
// partial: 2 plastic_state_blocks(v) doubles.  Writes nothing else; deterministic.
void launch_plastic_state(const PlasticView& v, double* perElem, double* partial, double* totals2, hipStream_t s);

} // namespace ipcgpu
