// Contact groups (ipcgpu_set_contact_groups): validation of the caller's tables and the per-node word the contact kernels read.  Every mesh component
// belongs to one of up to 16 groups; collide[g][h] says whether primitives of groups g and h form contact pairs at all, fricScale[g][h] multiplies the
// lagged normal force of a friction stencil between them.  Pure host logic (no HIP header: tests/test_contact_groups_host.py builds it with g++).
//
// The word of a node (pair_filtered / k_pair_flags, hip_contact.hip): bits 0-2 are the flags the kernel fills in (Dirichlet, obstacle, obstacle-only)
// and stay 0 here; bits 4-7 hold the group of the node's component; bits 16-31 hold that group's row of `collide` (bit 16 + h: collides with group h).
// A pair of nodes (a, b) is filtered when bit 16 + group(b) of a's word is 0 -- with a symmetric matrix either operand tells.
#pragma once
#include <string>
#include <vector>

namespace ipcgpu {

constexpr int CONTACT_GROUPS_MAX = 16;
// group 0, colliding with every group: the word of every node without a table
constexpr unsigned CONTACT_GROUP_DEFAULT_WORD = 0xFFFF0000u;

inline int contactGroupOfWord(unsigned w) { return (int)((w >> 4) & 15u); }

// compNodeEnd: the accumulated node ends of the nCompTable components (non-decreasing, the last one nV).  group[nComp], collide[nGroups^2] (0 / 1),
// fricScale[nGroups^2] or null (all 1).  On success returns true, words has nV entries and scale16 16 x 16 (row-major; 1 outside the caller's table).
// On failure returns false with the reason in err; words and scale16 are empty.
bool buildContactGroupWords(int nV, int nCompTable, const int* compNodeEnd, int nComp, const int* group, int nGroups, const unsigned char* collide,
    const double* fricScale, std::vector<int>& words, std::vector<double>& scale16, std::string& err);

} // namespace ipcgpu
