// Woven cloth of the elastic shells (gfx950, fp64): an orthotropic St. Venant-Kirchhoff membrane on the chosen triangles, in place of their isotropic one
// (shell_kernels.h), with its exact gradient and its exact Hessian clamped to PSD per triangle.  A project extension like the shells themselves.  The host
// side (validation, the compact list, the constants, the factor of the hinges) is shell_weave_plan.h.
//
// Per woven triangle t:  F = [x1 - x0, x2 - x0] Dm^-1 (3 x 2) and G = (F^T F - I) / 2 are the membrane's.  a is the unit warp direction in the triangle's rest
// frame (a 2-vector; shell_plan.h fixes the frame: its first axis runs along X1 - X0), b = (-a_y, a_x) the weft,
//   Eww = a^T G a,  Eff = b^T G b,  Ewf = a^T G b,
//   psi = C11 Eww^2 / 2 + C12 Eww Eff + C22 Eff^2 / 2 + 2 G12 Ewf^2,   W = h A psi,
//   C11 = E1 / (1 - nu12 nu21),  C22 = E2 / (1 - nu12 nu21),  C12 = nu12 E2 / (1 - nu12 nu21),  nu21 = nu12 E2 / E1.
//   Positive definite iff E1, E2, G12 > 0 and nu12^2 < E1 / E2.  With E1 = E2 = E, nu12 = nu, G12 = E / (2 (1 + nu)) it is the StVK membrane of
//   shell_kernels.h for every a (C11 = C22 = 2 mu + lambda_ps, C12 = lambda_ps, G12 = mu); a and -a give the same law.
// The kernels work in the yarn frame: with R = [a, b] (a rotation) the columns of F R are g1 = F a and g2 = F b, F R = [x1 - x0, x2 - x0] (Dm^-1 R), and
//   Eww = (g1 . g1 - 1) / 2,  Eff = (g2 . g2 - 1) / 2,  Ewf = g1 . g2 / 2:  the membrane's formulas with Dm^-1 R for Dm^-1 and three moduli for two.
// Gradient: dW/dF = F S,  S = h A (s_ww a a^T + s_ff b b^T + s_wf (a b^T + b a^T)),  s_ww = C11 Eww + C12 Eff,  s_ff = C12 Eww + C22 Eff,  s_wf = 2 G12 Ewf;
//   in the yarn frame dW/dg1 = s_ww g1 + s_wf g2, dW/dg2 = s_wf g1 + s_ff g2 (times h A).
// Hessian: S (x) I_3 plus the C-weighted outer products of dEww/dF = (F a) a^T, dEff/dF = (F b) b^T, dEwf/dF = ((F a) b^T + (F b) a^T) / 2; in the yarn frame
//   H11 = s_ww I + C11 g1 g1^T + G12 g2 g2^T,  H22 = s_ff I + C22 g2 g2^T + G12 g1 g1^T,  H12 = s_wf I + C12 g1 g2^T + G12 g2 g1^T,  H21 = H12^T  (times h A).
//   It annihilates the rigid translations, so it is formed as a 6 x 6 matrix in the Helmert basis of their complement, passed through sh::project_psd<6> and
//   expanded to the six upper node-pair blocks, exactly as k_shell_membrane does: the exact 9 x 9 Hessian with its eigenvalues clamped at 0.
// The law is a polynomial in F: finite at every finite F, a collapsed triangle included, so it needs no feasibility check and no step filter.
//
// Bending: every woven triangle carries two factors bendWarp, bendWeft > 0.  A hinge whose rest edge makes the angle phi with the warp bends the sheet across
//   that edge; its stiffness bendScale k_b w_e is multiplied by the mean over its two triangles of bendWarp sin^2 phi + bendWeft cos^2 phi (a triangle that is
//   not woven counts 1).  An edge along the weft (phi = 90 degrees) curves the warp yarns: bendWarp applies there.  Host arithmetic (shell_weave_plan.h); the
//   hinge kernels are untouched and read the product from row 1 of hingeConst.
//
// Not modelled: yarn sliding; locking (beyond what a strain limit on the same triangle gives); a warp direction that follows plastic flow (a woven triangle
//   can be neither plastic nor rubber); different moduli in compression and tension.
//
// One lane per woven triangle of the compact list.  Gradient entries and the six upper 3 x 3 blocks (the membrane's: no new node pairs) go through
// csr_scatter_device.h; rows, columns and gradient entries of projected Dirichlet nodes are dropped.  Without a woven triangle (nWoven == 0) nothing here is
// launched.  The StVK kernels are untouched: the two StVK constants of a woven triangle are zero in triConst, so they add exact zeros there.
#pragma once
#include "codim_view.h"
#include <hip/hip_runtime.h>

namespace ipcgpu {

struct ShellWeaveFields {
    int nTri, nWoven;
    const int* tri; // 3 nTri (the shell's)
    const double* triConst; // SoA [6][nTri] (the shell's; the first four rows, Dm^-1, are read)
    const int* wovTri; // nWoven: indices of the woven triangles
    const double* wovConst; // SoA [6][nWoven]: a_x, a_y, h A C11, h A C12, h A C22, h A G12 (shell_weave_plan.h)
};
struct ShellWeaveView : ShellWeaveFields, CodimBase {}; // (the shared fields behind the term's own: codim_view.h)

int shell_weave_energy_blocks(const ShellWeaveView& v); // partial sums launch_shell_weave_energy writes
// *out (device) = (accumulate ? *out : 0) + coef * woven energy; partial: shell_weave_energy_blocks(v) doubles.  Deterministic: fixed order.
void launch_shell_weave_energy(const ShellWeaveView& v, double coef, double* partial, double* out, bool accumulate, hipStream_t s);
void launch_shell_weave_energy_per_elem(const ShellWeaveView& v, double* perTri_nTri, hipStream_t s); // every triangle of the shell, 0 for one that is not woven
// grad (nullable) += coef * gradient; a (nullable) += coef * PSD Hessian blocks.  *err |= 1 where the pattern lacks a block (device int).
void launch_shell_weave_assemble(const ShellWeaveView& v, double coef, int projectDBC, double* grad, double* a, int* err, hipStream_t s);
// state_nTrix6 (device, column-major nTri x 6): per woven triangle Eww, Eff, the shear angle asin((F a) . (F b) / (|F a| |F b|)) and the current unit warp
// direction F a / |F a| (x, y, z); NaN where a length it divides by is 0; zeros on a triangle that is not woven.  Plain stores, one lane per triangle.
void launch_shell_weave_state(const ShellWeaveView& v, double* state_nTrix6, hipStream_t s);

} // namespace ipcgpu
