// Host side of the attachments (ipcgpu_set_attachments; attach_kernels.hip): from the caller's two points per attachment -- each up to three (node, weight)
// pairs -- the merged stencil the kernels read (distinct node ids with signed coefficients c_i = weight in A - weight in B), the constants, and the node
// pairs that must be in vNeighbor so that the CSR pattern holds every block the Hessian writes.  Pure host arithmetic (no HIP header:
// tests/test_attach_plan_host.py builds it with g++).  The reference has no attachments; the energy is stated in attach_kernels.h.
#pragma once
#include <string>
#include <vector>

namespace ipcgpu {

constexpr int ATTACH_SLOTS = 6; // at most three nodes per point, two points

struct AttachPlan {
    int n = 0;
    std::vector<int> count; // n: distinct nodes with a coefficient != 0 (2 to 6)
    // SoA [6][n]: slot s of attachment i at s n + i.  Slots 0 .. count - 1 hold the distinct nodes in the order of their first appearance (A's slots, then
    // B's) without those whose coefficients cancel; the slots behind them repeat the node of slot 0 with coefficient 0 (the kernels skip a zero coefficient)
    std::vector<int> node;
    std::vector<double> coef;
    std::vector<double> kL; // SoA [2][n]: stiffness k, rest length L
    std::vector<int> pairs; // 2 per pair (lo, hi), lo < hi, sorted, unique: every pair among the nodes of one attachment
};

// nodesA, weightsA, nodesB, weightsB: 3 n each, attachment-major (slot s of attachment i at 3 i + s); an unused slot is node id -1 with weight 0.
// false, with the reason in err and the plan empty: a node id out of range, a point with no node, a weight that is negative or not finite, a weight != 0 in
// an unused slot, weights of a point that do not sum to 1 within 1e-12, k <= 0 or L < 0 or either not finite, an attachment whose merged coefficients are all
// zero (A and B are the same point).
bool buildAttachPlan(int nV, int n, const int* nodesA, const double* weightsA, const int* nodesB, const double* weightsB, const double* k, const double* L,
    AttachPlan& plan, std::string& err);

// |sum_i c_i X_i| of attachment i at the rest positions Vrest (column-major nV x 3): the distance of its two points there
double attachRestDistance(const AttachPlan& plan, int i, int nV, const double* Vrest);

} // namespace ipcgpu
