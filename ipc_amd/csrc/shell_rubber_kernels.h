// Rubber membrane of the elastic shells (gfx950, fp64): the incompressible Mooney-Rivlin membrane on the chosen triangles, in place of their St. Venant-
// Kirchhoff membrane (shell_kernels.h), with its exact gradient and its exact Hessian clamped to PSD per triangle.  A project extension like the shells
// themselves.  The host side (validation, the compact list, the constants) is shell_rubber_plan.h.
//
// Per rubber triangle t:  F = [x1 - x0, x2 - x0] Dm^-1 (3 x 2, the membrane's), C = F^T F, tr = C11 + C22, J = det C.  The stretch across the thickness is
// eliminated by incompressibility, lambda_3 = 1 / sqrt(J):
//   I1 = tr + 1 / J,   I2 = tr / J + J,   psi = c1 (I1 - 3) + c2 (I2 - 3),   c1 = mu (1 - alpha) / 2,  c2 = mu alpha / 2,  mu = E / 3,  0 <= alpha < 1,
//   W = h A psi = k1 (I1 - 3) + k2 (I2 - 3),  k1 = h A c1, k2 = h A c2.
//   alpha = 0 is the incompressible neo-Hookean membrane mu / 2 (l1^2 + l2^2 + (l1 l2)^-2 - 3).  mu = E / 3 is the incompressible shear modulus: the Poisson
//   ratio given to ipcgpu_set_shell is NOT read by this term (it still enters the hinge constant k_b).  To second order in the strain W is the StVK membrane
//   with nu = 1 / 2 and the same mu.  No SVD: W is rational in the entries of C.
//   J is formed as |f1 x f2|^2 (Lagrange's identity), never as C11 C22 - C12^2: a sum of squares, non-negative in floating point, exactly 0 for exactly
//   parallel columns, and without the cancellation of the difference for a thin triangle.
// Gradient: dW/dF = F S,  S = 2 dW/dC = a I + b adj C,  a = 2 (k1 + k2 / J),  b = 2 (k2 - (k1 + k2 tr) / J^2),  adj C = [[C22, -C12], [-C12, C11]].
// Hessian in F (6 x 6):  S (x) I_3 + p (j t^T + t j^T) + q j j^T + (b / 2) (u1 u2^T + u2 u1^T - 2 u12 u12^T)  with the 6-vectors (d/dF of tr, J, C11, C22, C12)
//   t = 2 (f1; f2),  j = 2 (C22 f1 - C12 f2; C11 f2 - C12 f1),  u1 = 2 (f1; 0),  u2 = 2 (0; f2),  u12 = (f2; f1),  p = -k2 / J^2,  q = 2 (k1 + k2 tr) / J^3:
//   the membrane's structure S (x) I + sum of f_mu f_nu^T with other coefficients.  It annihilates the rigid translations, so it is formed as a 6 x 6 matrix
//   in the Helmert basis of their complement, passed through sh::project_psd<6> and expanded to the six upper node-pair blocks, exactly as k_shell_membrane
//   does: the exact 9 x 9 Hessian with its eigenvalues clamped at 0.
// Degenerate triangle: where J is not positive, or J or one of the coefficients above is not finite in floating point, the energy is +infinity -- never NaN,
//   which the line search would accept -- and the triangle adds NOTHING to gradient and matrix (they stay finite), as rod_kernels.h and the strain limit do.
//   The 1 / J term is a barrier: a rubber triangle cannot collapse to a line at finite energy.
//
// One lane per rubber triangle of the compact list.  Gradient entries and the six upper 3 x 3 blocks (the membrane's: no new node pairs) go through
// csr_scatter_device.h; rows, columns and gradient entries of projected Dirichlet nodes are dropped.  Without a rubber triangle (nRubber == 0) nothing here
// is launched.  The StVK kernels are untouched: the two StVK constants of a rubber triangle are zero in triConst, so they add exact zeros there.
// One consequence: with positions that are not finite (NaN, or an F whose squares overflow) the StVK kernel forms 0 x inf on a rubber triangle and puts NaN
// into energy, gradient and matrix there.  "+infinity, never NaN" and "nothing added" above are promises of THIS term; they hold for the shell as a whole at
// every finite F, a collapsed triangle included (there the StVK kernel adds 0 x a finite strain), which is every state the stepper can reach from a finite one.
// The degeneracy is decided on the unscaled coefficients, so the energy, count and assemble kernels agree on it whatever their coef.
#pragma once
#include "codim_view.h"
#include <hip/hip_runtime.h>

namespace ipcgpu {

struct ShellRubberFields {
    int nTri, nRubber;
    const int* tri; // 3 nTri (the shell's)
    const double* triConst; // SoA [6][nTri] (the shell's; the first four rows, Dm^-1, are read)
    const int* rubTri; // nRubber: indices of the rubber triangles
    const double* rubConst; // SoA [2][nRubber]: k1 = h A c1, k2 = h A c2 (shell_rubber_plan.h)
};
struct ShellRubberView : ShellRubberFields, CodimBase {}; // (the shared fields behind the term's own: codim_view.h)

int shell_rubber_energy_blocks(const ShellRubberView& v); // partial sums launch_shell_rubber_energy and launch_shell_rubber_degenerate write
// *out (device) = (accumulate ? *out : 0) + coef * rubber energy, +infinity with a degenerate rubber triangle; partial: shell_rubber_energy_blocks(v) doubles.
// Deterministic: fixed order.  coef must be positive.
void launch_shell_rubber_energy(const ShellRubberView& v, double coef, double* partial, double* out, bool accumulate, hipStream_t s);
void launch_shell_rubber_energy_per_elem(const ShellRubberView& v, double* perTri_nTri, hipStream_t s); // every triangle of the shell, 0 for a StVK one
// grad (nullable) += coef * gradient; a (nullable) += coef * PSD Hessian blocks.  *err |= 1 where the pattern lacks a block (device int).
void launch_shell_rubber_assemble(const ShellRubberView& v, double coef, int projectDBC, double* grad, double* a, int* err, hipStream_t s);
// *out (device) = the number of degenerate rubber triangles (those whose energy is +infinity), as a double.  Fixed order.
void launch_shell_rubber_degenerate(const ShellRubberView& v, double* partial, double* out, hipStream_t s);

} // namespace ipcgpu
