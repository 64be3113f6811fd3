// Host side of the aerodynamic surfaces (ipcgpu_set_aero; aero_kernels.hip): from the caller's triangle lists -- one contiguous range per surface -- the
// validated SoA triangle list the kernels read, the surface of every triangle, the per-surface coefficients as the kernels load them, the lagged record of
// every triangle at the rest positions, and the node pairs that must be in vNeighbor so that the CSR pattern holds every block the Hessian writes.  Pure
// host arithmetic (no HIP header: tests/test_aero_plan_host.py builds it with g++).  The reference has no such load; the model is stated in aero_kernels.h.
#pragma once
#include <string>
#include <vector>

namespace ipcgpu {

// The lagged record of one triangle, eight doubles: n (3), A, c (3), 0.  In a fixed order, each product, sum and quotient rounded once (the translation
// unit is compiled without contraction into fused multiply-adds):
//   e1 = x1 - x0,  e2 = x2 - x0,  m = (e1_y e2_z - e1_z e2_y,  e1_z e2_x - e1_x e2_z,  e1_x e2_y - e1_y e2_x),  l = sqrt((m_x m_x + m_y m_y) + m_z m_z)
//   n = m / l (entry by entry),  A = 0.5 l,  c = ((x0 + x1) + x2) / 3.0;   l == 0 or not finite: n = 0 and A = 0
void aeroRecord(const double* x0, const double* x1, const double* x2, double* rec8);

struct AeroPlan {
    int n = 0, nTri = 0; // surfaces, triangles
    std::vector<int> triEnd; // n: surface s owns the triangles [triEnd[s - 1], triEnd[s]) (triEnd[-1] = 0)
    std::vector<int> tri; // SoA [3][nTri]: node k of triangle t at k nTri + t, in the caller's order and orientation
    std::vector<int> surfOf; // nTri
    std::vector<double> cn, ct; // n
    std::vector<int> oneSided; // n (0 / 1)
    std::vector<double> coef; // 4 n: Cn, Ct, oneSided as 0.0 / 1.0, 0 -- what the kernels load
    std::vector<double> restRecord; // 8 nTri: aeroRecord at the rest positions
    std::vector<int> pairs; // 2 per pair (lo, hi), lo < hi, sorted, unique: the three edges of every triangle
};

// Vrest: column-major nV x 3; triEnd: nSurf; tri: column-major nTri x 3 with nTri = triEnd[nSurf - 1]; cn, ct, oneSided: nSurf.
// false, with the reason in err (it names the surface and the triangle) and the plan empty: triEnd not ascending, an empty surface, a coefficient that is
// negative or not finite, a node id out of range, a triangle that repeats a node, a triangle whose rest area is zero (or not finite), a triangle listed
// twice -- in the same or in another surface, in any rotation or orientation.
bool buildAeroPlan(int nV, const double* Vrest, int nSurf, const int* triEnd, const int* tri, const double* cn, const double* ct, const int* oneSided, AeroPlan& plan,
    std::string& err);

} // namespace ipcgpu
