// Growth of the contact part of the solver's pattern (the reference's vNeighbor_IP, Optimizer.cpp:3560-3612): host-only integer logic on node pairs, no HIP
// header, so that tests/test_contact_pattern.py drives it without a GPU.  HipOptimizer::growPattern feeds it.
#pragma once
#include <functional>
#include <utility>
#include <vector>

namespace ipcgpu {

using NodePairs = std::vector<std::pair<int, int>>;

// the pairs that are not mesh edges (nbPtr / nb: the mesh adjacency as sorted CSR), sorted by (first, second) and unique: only those change the pattern
NodePairs nonMeshPairs(const NodePairs& pairs, const int* nbPtr, const int* nb);

// The contact pairs inside the current pattern.  The reference rebuilds pattern + symbolic analysis whenever the contact graph changes (:3570-3592); here the
// list only ever GROWS inside the stepper: pairs that left the constraint set keep their (zero) slots, so a new analysis is needed only when a pair shows up
// that no earlier iteration had.  Same matrix, fewer host-side analyses; the union is dropped again once it has grown far beyond the live set.
class ContactPattern {
public:
    const NodePairs& pairs() const { return pairs_; }
    const std::vector<int>& flat() const { return flat_; } // pairs() interleaved, int[2 n]: what set_pattern takes
    // live: the pairs of the live sets, or null = not formed on the host, the device has already said that the pattern lacks one of their blocks.  lookAhead:
    // the pairs of the look-ahead sets (empty for an exact pattern); they cost constraint-set builds, so they are asked for only once growth is certain.  Both
    // as nonMeshPairs leaves them.  Returns whether a new pattern is needed; pairs() and flat() then hold it.
    bool grow(const NodePairs* live, const std::function<NodePairs()>& lookAhead);

private:
    NodePairs pairs_;
    std::vector<int> flat_;
};

} // namespace ipcgpu
