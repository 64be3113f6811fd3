// Host side of the elastic rods (ipcgpu_set_rod; rod_kernels.hip): from the segment list and the rest positions, everything the kernels read and the mesh
// has to know -- validated segments, their stretch constants, the bending triples of the interior nodes, the lumped masses, and the node pairs that must
// be in vNeighbor so that the CSR pattern holds every block the rod Hessian writes.  Pure host arithmetic (no HIP header: tests/test_rod_plan_host.py
// builds it with g++).  The reference has no rods; the energies are stated in rod_kernels.h.
#pragma once
#include <string>
#include <vector>

namespace ipcgpu {

struct RodPlan {
    int nSeg = 0, nBend = 0;
    std::vector<int> seg; // 2 nSeg, node ids of segment s at 2 s, 2 s + 1, as given
    std::vector<double> segConst; // SoA [2][nSeg]: rest length L, k_s = E pi r^2 / L
    // bending triples: one per node b with exactly two incident segments, ascending by b.  bend[3 i ..] = (a, b, c): a the far node of the incident segment
    // with the smaller index, c that of the other one.  A node with one segment is an end, one with three or more a junction: neither bends.
    std::vector<int> bend;
    std::vector<double> bendK; // k_b = E_m pi r_m^4 / 4 / (L0 + L1), E_m and r_m the means of the two segments
    std::vector<double> restKb; // |kb| of the rest polyline at the node (the rest state of the energy is straight: a value > 0 will be pulled straight)
    std::vector<double> mass; // nV: sum over the node's segments of rho pi r^2 L / 2 (0 for a node of no segment)
    std::vector<char> isRodNode; // nV
    std::vector<int> pairs; // 2 per pair (lo, hi), lo < hi, sorted, unique: (a, b) per segment and (a, c) per triple
    double lenSum = 0.0; // sum of the rest lengths (mean segment = lenSum / nSeg)
};

// |kb| = 2 |e0 x e1| / d of the polyline a - b - c with e0 = b - a, e1 = c - b, d = |e0||e1| + e0 . e1, evaluated as sqrt(4 (|e0||e1| - e0 . e1) / d)
// (= 2 tan(theta / 2), theta the turning angle); +infinity where d <= 0 (an exact fold).
double rodCurvature(const double xa[3], const double xb[3], const double xc[3]);

// seg: column-major nSeg x 2 (seg[s + nSeg k] = node k of segment s); Vrest: column-major nV x 3; radius, YM, rho: per segment; tets: 4 nTet node ids and
// shellTri: 3 nShellTri node ids (only membership is read; either may be null when its count is 0).  false, with the reason in err and the plan empty:
// a node id out of range, a segment with a == b, a repeated segment (in either direction), zero rest length, a rod node that belongs to a tetrahedron or
// to a shell triangle, or a radius, E or rho that is not positive.
bool buildRodPlan(int nV, int nSeg, const int* seg, const double* Vrest, const double* radius, const double* YM, const double* rho, int nTet, const int* tets,
    int nShellTri, const int* shellTri, RodPlan& plan, std::string& err);

} // namespace ipcgpu
