// Host side of the pressure chambers (ipcgpu_set_chambers; chamber_kernels.hip): from the caller's triangle lists -- one contiguous range per chamber --
// the validated SoA triangle list the kernels read, the chamber of every triangle, the rest volume and the rest reference point of every chamber, and the
// node pairs that must be in vNeighbor so that the CSR pattern holds every block the Hessian writes.  Pure host arithmetic (no HIP header:
// tests/test_chamber_plan_host.py builds it with g++).  The reference has no chambers; the energy is stated in chamber_kernels.h.
#pragma once
#include <string>
#include <vector>

namespace ipcgpu {

struct ChamberPlan {
    int n = 0, nTri = 0;
    std::vector<int> triEnd; // n: chamber c owns the triangles [triEnd[c - 1], triEnd[c]) (triEnd[-1] = 0)
    std::vector<int> tri; // SoA [3][nTri]: node k of triangle t at k nTri + t, in the caller's order and orientation
    std::vector<int> chamberOf; // nTri
    std::vector<double> pressure; // n
    // Both in a fixed order, triangle after triangle of the chamber's range, one accumulator per number:
    //   restRef[3 c + a] = (sum_t ((X0_a + X1_a) + X2_a)) / (3 m), m the chamber's triangle count: the mean of the triangle centroids
    //   restVolume[c]    = (sum_t (y0_x (y1_y y2_z - y1_z y2_y) + y0_y (y1_z y2_x - y1_x y2_z)) + y0_z (y1_x y2_y - y1_y y2_x)) / 6,  y_k = X_k - restRef
    // (each product and sum rounded once: the translation unit is compiled without contraction into fused multiply-adds)
    std::vector<double> restRef; // 3 n
    std::vector<double> restVolume; // n
    std::vector<int> pairs; // 2 per pair (lo, hi), lo < hi, sorted, unique: the three edges of every triangle
};

// Vrest: column-major nV x 3; triEnd: nCh; tri: column-major nTri x 3 with nTri = triEnd[nCh - 1]; pressure: nCh.
// false, with the reason in err (it names the chamber and the triangle or edge) and the plan empty: triEnd not ascending, an empty chamber, a pressure that
// is not finite, a node id out of range, a triangle that repeats a node, an edge of a chamber that is not used by exactly two of that chamber's triangles,
// two triangles that traverse a shared edge in the same direction, a rest volume <= 0 (the chamber is oriented inward).
bool buildChamberPlan(int nV, const double* Vrest, int nCh, const int* triEnd, const int* tri, const double* pressure, ChamberPlan& plan, std::string& err);

// The gas law of the chambers (ipcgpu_chamber_set_gas; the model is stated in chamber_kernels.h): which chambers follow it, their parameters, and the cut of
// every gas chamber's triangle range into slices for the two-pass volume reduction.  nGas == 0: every chamber is constant and nothing else is ever read.
constexpr int CHAMBER_GAS_MAX = 8; // gas chambers per context: the rank of the correction inside the linear solve
constexpr int CHAMBER_GAS_SLICE = 256; // triangles per slice at the most: one workgroup of the first pass

struct ChamberGas {
    int nGas = 0;
    std::vector<int> isGas; // n (0 / 1)
    std::vector<double> ambient, gamma, fillVolume; // n; of a constant chamber 0, 1 and its rest volume
    std::vector<int> gasChamber; // nGas: the gas chambers, ascending
    // the slices: chamber after chamber (gas chambers only), inside a chamber by ascending triangle index; every slice holds 1 .. CHAMBER_GAS_SLICE triangles of
    // ONE chamber, and the slices of gas chamber g (the g-th of gasChamber) are [sliceOff[g], sliceOff[g + 1])
    std::vector<int> sliceBegin, sliceEnd; // nSlice: triangles [begin, end)
    std::vector<int> sliceOff; // nGas + 1
    int nSlice() const { return (int)sliceBegin.size(); }
};

// isGas, ambient, gamma: n values each; fillVolume: nullable, and a value <= 0 means the chamber's rest volume.  The parameters of a chamber with isGas == 0 are
// not looked at.  false, with the reason in err (it names the chamber) and gas empty: no chambers, a null argument, a value that is not finite, ambient < 0,
// gamma < 1, ambient + pressure <= 0, more than CHAMBER_GAS_MAX gas chambers.
bool buildChamberGas(const ChamberPlan& plan, const int* isGas, const double* ambient, const double* gamma, const double* fillVolume, ChamberGas& gas, std::string& err);
// may the chambers take these pressures: false, naming the chamber, where a gas chamber would get ambient + pressure <= 0
bool chamberGasPressureOk(const ChamberGas& gas, int n, const double* pressure, std::string& err);

} // namespace ipcgpu
