// Strain limiting of the elastic shells (gfx950, fp64): a log barrier on the principal stretches of the limited triangles, its exact gradient and its exact
// Hessian, which is positive semidefinite as it stands.  A project extension like the shells themselves (shell_kernels.h); after the strain limit of the
// codimensional follow-up to IPC.  The host side (validation, the compact list, the constants) is shell_limit_plan.h.
//
// Per triangle t with limit s > 0, onset sHat (1 <= sHat < s) and k = stiff h A E:  F = [x1 - x0, x2 - x0] Dm^-1 (3 x 2, the membrane's), sigma1 >= sigma2 >= 0
// its singular values in closed form: with C = F^T F, m = (C11 + C22) / 2, d = (C11 - C22) / 2, r = sqrt(d^2 + C12^2): sigma1 = sqrt(m + r),
// sigma2 = |f1 x f2| / sigma1 (the product of the two is the area ratio: no cancellation for a thin triangle), sigma1^2 - sigma2^2 = 2 r.
//   W = k (b(sigma1) + b(sigma2)),   b(sigma) = 0 for sigma <= sHat,  -y^2 ln(1 - y) with y = (sigma - sHat) / (s - sHat) for sHat < sigma < s,
//   +infinity for sigma >= s -- and for a sigma that does not compare (NaN positions): the energy is never NaN, which the line search would accept.
//   b is C^2 at the onset (b ~ y^3), increasing and convex:  b' (s - sHat) = -2 y L + y^2 / z,  b'' (s - sHat)^2 = -2 L + 4 y / z + y^2 / z^2,
//   L = ln z, z = 1 - y.  {sigma1 < s} is a convex set of positions (sigma1 is the operator norm of F, F is linear in x): on a line from a feasible state
//   every shorter step is feasible too.
// Gradient: dW/dF = k sum_i b'(sigma_i) u_i v_i^T, v_i the eigenvectors of C, u_i = F v_i / sigma_i.
// Hessian in F (6 x 6), eigenpairs with u3 the unit normal of the deformed triangle:
//   u_i v_i^T: b''(sigma_i);   (u1 v2^T - u2 v1^T) / sqrt 2: (b'1 + b'2) / (sigma1 + sigma2);   (u1 v2^T + u2 v1^T) / sqrt 2: (b'1 - b'2) / (sigma1 - sigma2);
//   u3 v_i^T: b'(sigma_i) / sigma_i.   All >= 0 (b' is increasing and >= 0); each is clamped at 0 against round-off: no eigen-iteration.
//   The divided difference is formed without a cancelling subtraction: with q = (y1 - y2) / z2,
//   (b'1 - b'2)(s - sHat)^2 / (sigma1 - sigma2) = (y1 + y2 - y1 y2) / (z1 z2) - 2 (L1 + y2 log1p(-q) / (q z2)),  log1p(-q) / q = -1 at q = 0 (then it is b'').
//   With sigma2 <= sHat (b'2 = b''2 = 0) neither u2 nor u3 is formed -- both are ill-defined for a triangle collapsed to a line --: with w = F v2 = sigma2 u2
//   and P = I - u1 u1^T the same matrix is  b''1 u1v1 (x) u1v1 + (b'1 / sigma1) P (x) v1 v1^T + b'1 / (2 r) [sigma1 u1v2 (x) u1v2 + (w w^T / sigma1) (x) v1 v1^T
//   + u1v2 (x) w v1 + w v1 (x) u1v2]  (sum of the twist, flip and u3 v1^T terms; (x): outer product of 3 x 2 matrices as 6-vectors).
// A triangle with sigma1 >= s contributes +infinity to the energy and NOTHING to gradient and matrix (they stay finite); one with sigma1 <= sHat nothing at all.
//
// One lane per limited triangle.  Gradient entries and the six upper 3 x 3 blocks (the membrane's: no new node pairs) go through csr_scatter_device.h; rows,
// columns and gradient entries of projected Dirichlet nodes are dropped.  Without a limit (nLimited == 0) nothing here is launched.
#pragma once
#include "codim_view.h"
#include <hip/hip_runtime.h>

namespace ipcgpu {

struct ShellLimitFields {
    int nTri, nLimited;
    const int* tri; // 3 nTri (the shell's)
    const double* triConst; // SoA [6][nTri] (the shell's; the first four rows, Dm^-1, are read)
    const int* limTri; // nLimited: indices of the limited triangles
    const double* limConst; // SoA [3][nLimited]: onset, limit, k (shell_limit_plan.h)
    const double* triLimit; // nTri: limit per triangle, 0 = none; null without a limit (only the stretch kernel reads it)
};
struct ShellLimitView : ShellLimitFields, CodimBase {}; // (the shared fields behind the term's own: codim_view.h)

int shell_limit_energy_blocks(const ShellLimitView& v); // partial sums launch_shell_limit_energy writes
// *out (device) = (accumulate ? *out : 0) + coef * barrier energy, +infinity with a stretch at or over its limit; partial: shell_limit_energy_blocks(v) doubles.
// Deterministic: fixed order.  coef must be positive.
void launch_shell_limit_energy(const ShellLimitView& v, double coef, double* partial, double* out, bool accumulate, hipStream_t s);
void launch_shell_limit_energy_per_elem(const ShellLimitView& v, double* perTri_nTri, hipStream_t s); // every triangle of the shell, 0 for an unlimited one
// grad (nullable) += coef * gradient; a (nullable) += coef * Hessian blocks.  *err |= 1 where the pattern lacks a block (device int).
void launch_shell_limit_assemble(const ShellLimitView& v, double coef, int projectDBC, double* grad, double* a, int* err, hipStream_t s);
int shell_stretch_blocks(const ShellLimitView& v); // launch_shell_stretch needs 2 * shell_stretch_blocks(v) doubles of `partial`
// sigma (nullable): sigma1, sigma2 of triangle t at 2 t, 2 t + 1 (every triangle of the shell).  out2 (device): the maximum of sigma1 / limit over the limited
// triangles (0 without one; +infinity where a stretch is NaN), and the number of triangles with a stretch at or over the limit (as a double).  Fixed order.
void launch_shell_stretch(const ShellLimitView& v, double* sigma, double* partial, double* out2, hipStream_t s);

} // namespace ipcgpu
