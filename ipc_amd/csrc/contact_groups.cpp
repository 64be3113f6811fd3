// Contact groups: validation and the per-node packed words.  See contact_groups.h.  Host only.
#include "contact_groups.h"
#include <cmath>
#include <cstddef>

namespace ipcgpu {

bool buildContactGroupWords(int nV, int nCompTable, const int* compNodeEnd, int nComp, const int* group, int nGroups, const unsigned char* collide,
    const double* fricScale, std::vector<int>& words, std::vector<double>& scale16, std::string& err)
{
    words.clear();
    scale16.clear();
    auto fail = [&](const char* what) {
        err = what;
        return false;
    };
    if (nV < 0 || nCompTable < 1 || !compNodeEnd) return fail("contact groups: no component table");
    for (int c = 0; c < nCompTable; ++c)
        if (compNodeEnd[c] < (c ? compNodeEnd[c - 1] : 0)) return fail("contact groups: the component table's node ends decrease");
    if (compNodeEnd[nCompTable - 1] != nV) return fail("contact groups: the component table does not end at the node count");
    if (nComp != nCompTable) return fail("contact groups: one group per component of ipcgpu_opt_set_components (the default table has one component)");
    if (!group || !collide) return fail("contact groups: null table");
    if (nGroups < 1 || nGroups > CONTACT_GROUPS_MAX) return fail("contact groups: between 1 and 16 groups");
    for (int c = 0; c < nComp; ++c)
        if (group[c] < 0 || group[c] >= nGroups) return fail("contact groups: a component's group lies outside [0, nGroups)");
    const std::size_t n = (std::size_t)nGroups;
    for (std::size_t g = 0; g < n; ++g)
        for (std::size_t h = 0; h < n; ++h) {
            if (collide[g * n + h] > 1) return fail("contact groups: collide holds something other than 0 or 1");
            if (collide[g * n + h] != collide[h * n + g]) return fail("contact groups: collide is not symmetric");
            if (!fricScale) continue;
            const double s = fricScale[g * n + h];
            if (!std::isfinite(s) || s < 0.0) return fail("contact groups: a friction scale is negative or not finite");
            if (s != fricScale[h * n + g]) return fail("contact groups: fricScale is not symmetric");
        }
    unsigned wordOf[CONTACT_GROUPS_MAX];
    for (std::size_t g = 0; g < n; ++g) {
        unsigned row = 0;
        for (std::size_t h = 0; h < n; ++h) row |= (unsigned)collide[g * n + h] << h;
        wordOf[g] = ((unsigned)g << 4) | (row << 16);
    }
    words.resize((std::size_t)nV);
    for (int c = 0, v = 0; c < nComp; ++c)
        for (; v < compNodeEnd[c]; ++v) words[(std::size_t)v] = (int)wordOf[group[c]];
    scale16.assign((std::size_t)CONTACT_GROUPS_MAX * CONTACT_GROUPS_MAX, 1.0);
    if (fricScale)
        for (std::size_t g = 0; g < n; ++g)
            for (std::size_t h = 0; h < n; ++h) scale16[g * CONTACT_GROUPS_MAX + h] = fricScale[g * n + h];
    err.clear();
    return true;
}

} // namespace ipcgpu
