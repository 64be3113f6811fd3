// Coarse space of the two-level preconditioner of the iterative solver (pcg.h, IPCGPU_PRECOND_TWO_LEVEL): a greedy aggregation of the node graph and
// everything the Galerkin product P^T A P needs to run on the device without a search.  Pure integer logic on the node-block pattern, host only (no HIP
// header: tests/test_pcg_coarse.py builds it with g++).  HipLinSysSolver uploads the arrays as they stand here.
//
// Every aggregate I carries six coarse unknowns, stored as two coarse "nodes" of three: 2 I (translation) and 2 I + 1 (rotation about the centroid of
// the aggregate's free nodes).  The coarse matrix is therefore a symmetric-upper CSR of 3x3 node blocks with the row lay-out of the fine one
// (LinSysSolver.hpp:63-111: the three rows of a node hold len, len - 1, len - 2 entries), which the multifrontal solver analyses and factorises.
#pragma once
#include <vector>

namespace ipcgpu {

struct PcgCoarse {
    int nNodes = 0, nAgg = 0;
    std::vector<int> aggOf; // [nNodes] aggregate of every node (fixed nodes included: they are in the graph, only P has no entries for them)
    std::vector<int> aggPtr, aggNodes; // [nAgg + 1], [nNodes]: the nodes of every aggregate, ascending
    std::vector<int> aggFree; // [nAgg] nodes of the aggregate that are not fixed (fewer than 4: translations only)
    // coarse pattern: 6 nAgg rows, upper, columns ascending, diagonal first; per coarse node the first slot of its row 3 c and that row's length
    std::vector<int> cia, cja, cRowBase, cRowLen;
    // One record per aggregate pair I <= J that at least one fine block connects, sorted by (I, J).  pairSlot[4 p + q]: the slot in row 0 of the coarse
    // block (translation|rotation of I) x (translation|rotation of J), q = 0 TT, 1 TR, 2 RT, 3 RR; on the diagonal (I == J) TT and RR are diagonal blocks
    // and RT = -1 (it is the transpose of TR).
    std::vector<int> pairI, pairJ, pairPtr, pairSlot;
    // The fine blocks of a pair, pairPtr[p] .. pairPtr[p + 1], in the order of the fine storage.  Every stored block (u, w), u <= w, of the upper storage is
    // in exactly one list, exactly once: entSlot = the slot of its first entry in row 3 u, entRow = u, entCol = w, entTrans = 1 when agg(u) > agg(w), i.e. the
    // pair receives the block's transpose (w, u).  Through symmetry that covers every block of the full matrix once: an off-diagonal block inside one
    // aggregate stands for itself and its mirror image, which the product adds as M + M^T.
    std::vector<int> entSlot, entRow, entCol, entTrans;

    // ia is not needed: a node's blocks are the runs of three columns behind the diagonal block in ja[rowBase[u] .. rowBase[u] + rowLen[u])
    void build(int nNodes, const int* ja, const int* rowBase, const int* rowLen, const unsigned char* fixed);
};

} // namespace ipcgpu
