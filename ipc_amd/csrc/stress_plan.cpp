// Node -> element incidence list of the nodal stress pass: see stress_plan.h.  Host only.
#include "stress_plan.h"
#include <cstddef>

namespace ipcgpu {

bool buildNodeElementIncidence(int nV, int nT, const int* F, std::vector<int>& ptr, std::vector<int>& elems)
{
    ptr.clear();
    elems.clear();
    if (nV < 0 || nT < 0 || (nT > 0 && !F) || (long long)nT * 4 > 0x7fffffffLL) return false;
    const std::size_t n4 = 4 * (std::size_t)nT;
    for (std::size_t i = 0; i < n4; ++i)
        if (F[i] < 0 || F[i] >= nV) return false;
    // counting sort by node: counts, exclusive scan, then the elements in index order -- so every row comes out ascending
    ptr.assign((std::size_t)nV + 1, 0);
    for (std::size_t i = 0; i < n4; ++i) ++ptr[(std::size_t)F[i] + 1];
    for (int v = 0; v < nV; ++v) ptr[(std::size_t)v + 1] += ptr[v];
    elems.resize(n4);
    std::vector<int> at(ptr.begin(), ptr.end() - 1);
    for (int t = 0; t < nT; ++t)
        for (int k = 0; k < 4; ++k) elems[(std::size_t)at[F[t + (std::size_t)nT * k]]++] = t;
    return true;
}

} // namespace ipcgpu
