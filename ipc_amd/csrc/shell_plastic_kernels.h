// Plastic flow of the elastic shells (gfx950, fp64): permanent stretch, creases and dents -- a can wall that stays dented, sheet metal that keeps a crease,
// foil that stays crumpled, a membrane that sags after over-stretching.  A project extension: the reference has no shells and no plasticity.  The host side
// (validation, the parameter arrays, which hinges flow, their constants) is shell_plastic_plan.h.
//
// Every shell kernel reads the rest configuration of triangle t from rows 0-3 of triConst (B = Dm^-1, 2 x 2, column-major b00 b10 b01 b11) and of hinge i from
// row 0 of hingeConst (thetaBar), and from nowhere else, so plastic flow is a rewrite of those records at the end of a time step: the membrane, bending,
// strain-limit, energy, assemble and damping kernels stay as they are and see the new rest shape from the next step on.
// Per triangle four parameters: yield (a strain, >= 0 or +inf: +inf switches the membrane flow off), bendYield (a strain, >= 0 or +inf: +inf switches the
// hinge flow off), creep (> 0 or +inf: +inf is the rate-independent return), harden (>= 0, finite).  r = -expm1(-creep dt), as for the tetrahedra.
//
// MEMBRANE FLOW, per triangle t with yield_t < +inf, at positions x:
//     F = [x1 - x0, x2 - x0] B (3 x 2),  C = F^T F = V diag(l1, l2) V^T,  l1 >= l2            closed-form symmetric 2 x 2 eigen-decomposition, no iteration;
//                                                  a zero off-diagonal entry (which includes l1 == l2 there) is its own branch; l2 = det C / l1 with
//                                                  det C = |(x1 - x0) x (x2 - x0)|^2 (det B)^2, so that l2 carries no cancellation
//     !(l2 > 0) or anything not finite (a collapsed triangle): the triangle is SKIPPED this step and counted; nothing is written
//     e_i = ln(l_i) / 2;  the plane-stress thickness strain e3 = -c (e1 + e2),  c = triConst[5] / (2 triConst[4]) = lambda_ps / (2 mu) = nu / (1 - nu)
//     d = (e1, e2, e3) - mean,  n = |d|_2          the deviatoric Hencky norm of the 3-D strain state: the meaning of yield is the tetrahedra's, von Mises
//                                                  stress ~ sqrt(6) mu n.  n^2 = ((1 + 2 c)^2 / 3) p^2 + q^2 with p = (e1 + e2) / sqrt 2, q = (e1 - e2) / sqrt 2
//     y = yield_t + harden_t alpha_t;  n <= y: nothing is written -- the four doubles of B and alpha keep their bits (tested before any division by n, also
//                                                  at yield = 0)
//     Delta = r (n - y) / (1 + harden_t),  f = Delta / n,  G = V diag(exp(-f e1), exp(-f e2)) V^T,  B <- B G,  alpha_t <- alpha_t + Delta
//   The new elastic strain is (1 - f) e, so n' = n - Delta and the new yield strain is y + harden Delta: the excess n - y shrinks by exactly 1 - r =
//   exp(-creep dt) per flow, whatever harden is.  G is an isotropic function of C: well defined where l1 == l2, although V is not.  Rows 4 and 5 of triConst
//   (h A mu, h A lambda_ps) are NOT written: the thickness takes up the plastic change of area det G, so the rest volume h A keeps its value, and with it the
//   lumped masses, membraneK and the strain-limit scale.  A strain-limited triangle may be plastic: the barrier then limits the elastic stretch relative to the
//   flowed rest shape.  A rubber triangle has zeros in rows 4 and 5 and may not be plastic (refused both ways round, as fibres and plasticity are).
//
// HINGE FLOW, per hinge whose two triangles both have bendYield < +inf; its bendYield, creep and harden are the arithmetic means of the two triangles':
//     theta = the shell kernels' signed dihedral angle (shell_hinge_device.h: the same device function),  k = theta - thetaBar, NOT unwrapped, as the energy
//     a zero-length n1, n2 or e (or anything not finite): the hinge is SKIPPED and counted
//     eps = g |k|                                  the outer-fibre strain; the rest constant g = h_m w_e / (2 |eBar|), h_m the mean rest thickness of the two triangles
//     y = bendYield + harden alphaB;  eps <= y: nothing is written
//     Delta = r (eps - y) / (1 + harden),  thetaBar <- thetaBar + sign(k) Delta / g,  alphaB <- alphaB + Delta
//   Delta / g <= |k|: thetaBar' lies between thetaBar and theta, so it stays in (-pi, pi] without a clamp.  Row 1 of hingeConst is not written.
//
// NOT modelled: the effect of thinning on k_b and on ipcgpu_shell_thickness;  coupling of membrane and bending yield;  kinematic hardening;  a flow direction
//   that is exactly deviatoric when nu != 1/2 (the in-plane elastic strain flows radially: that is what makes the return exact);  rods and attachments (a rod's
//   bending energy has a straight rest state only);  sharded contexts (refused both ways round).
//
// k_shell_plastic_flow_tri / k_shell_plastic_flow_hinge: 256 lanes, one lane per triangle / hinge.  Coalesced SoA loads of the records, the parameters and
// the history, the node gather of the shell kernels; exact log / exp / expm1 (no fast_* seed); stores from the lanes that yielded and from no other.  The four
// counters (ShellPlasticCount, scalar_slots.h) are integer atomics in the scheme of k_plastic_flow -- a ballot per wave, the waves of a workgroup in LDS, one
// add per workgroup --; there is no floating-point atomic: the same state gives the same bits.  No scratch, no LDS beyond the counters.
// k_shell_plastic_state (read-only): per triangle n, y, alpha and the rest-area ratio det B0 / det B; per hinge eps, y, alphaB and thetaBar - thetaBar0; the
// maximum of alpha, the maximum of alphaB and the sum of h A alpha, reduced in a fixed order (device_prims.h).
// The unit is compiled without contraction into fused multiply-adds (build.py), so theta may differ in its last bits from the one the contracted energy
// kernels form from the same source; tests/shell_plastic_mp.py bounds both against mpmath.
#pragma once
#include <hip/hip_runtime.h>

namespace ipcgpu {

struct ShellPlasticView {
    int nTri, nHinge;
    const double* x; // positions, xyz interleaved
    const int* tri; // 3 nTri
    double* triConst; // SoA [6][nTri]: rows 0-3 read, and rewritten by the lanes that yield; rows 4-5 read only
    const int4* hinge; // nHinge
    double* hingeConst; // SoA [2][nHinge]: row 0 read, and rewritten by the lanes that yield
    const double* yield; // nTri; +inf: membrane flow off
    const double* creep; // nTri
    const double* harden; // nTri
    double* alpha; // nTri accumulated membrane plastic strain
    const double* hYield; // nHinge: the mean bendYield; +inf: the hinge does not flow
    const double* hCreep; // nHinge
    const double* hHarden; // nHinge
    const double* hG; // nHinge: g = h_m w_e / (2 |eBar|)
    double* alphaB; // nHinge accumulated outer-fibre plastic strain
    const double* hA; // nTri rest volumes h A (state only; never written)
    const double* B0; // SoA [4][nTri] (state only)
    const double* thetaBar0; // nHinge (state only)
    double dt;
};

// One flow at v.x.  counts (device, SPC_COUNT ints, zeroed by the caller): += triangles / hinges that yielded / were skipped.  tris / hinges: launch that kernel.
void launch_shell_plastic_flow(const ShellPlasticView& v, bool tris, bool hinges, int* counts, hipStream_t s);
int shell_plastic_state_blocks(const ShellPlasticView& v); // partials per quantity that launch_shell_plastic_state writes
// perTri (nullable; column-major nTri x 4): n, y, alpha, det B0 / det B at v.x -- n = NaN where the flow would skip the triangle (and on a rubber triangle,
// which has no c), y = +inf where the membrane flow is off.  perHinge (nullable; column-major nHinge x 4): eps, y, alphaB, thetaBar - thetaBar0 -- eps = NaN
// where the flow would skip the hinge, y = +inf where the hinge does not flow.  totals3 (nullable; device, SPT_COUNT doubles).  partial: 3
// shell_plastic_state_blocks(v) doubles.  Writes nothing else; deterministic.
void launch_shell_plastic_state(const ShellPlasticView& v, double* perTri, double* perHinge, double* partial, double* totals3, hipStream_t s);

} // namespace ipcgpu
