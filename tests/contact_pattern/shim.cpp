// TEST INFRASTRUCTURE (host only): the growth rules of the contact pattern (ipc_amd/csrc/contact_pattern.cpp) behind plain C calls for
// tests/test_contact_pattern.py.  Pairs travel interleaved, int[2 n].  Built by the test with g++.
#include "../../ipc_amd/csrc/contact_pattern.h"
#include <algorithm>
using namespace ipcgpu;
static ContactPattern g_pat;
static NodePairs unflat(int n, const int* p)
{
    NodePairs v;
    for (int i = 0; i < n; ++i) v.emplace_back(p[2 * i], p[2 * i + 1]);
    return v;
}
static int flatten(const NodePairs& v, int* out)
{
    for (size_t i = 0; i < v.size(); ++i) {
        out[2 * i] = v[i].first;
        out[2 * i + 1] = v[i].second;
    }
    return (int)v.size();
}
extern "C" int shim_non_mesh_pairs(int n, const int* pairs, const int* nbPtr, const int* nb, int* out)
{
    return flatten(nonMeshPairs(unflat(n, pairs), nbPtr, nb), out);
}
extern "C" void shim_clear() { g_pat = ContactPattern(); }
// nLive < 0: the live pairs were not formed.  *asked: whether the look-ahead pairs were asked for.  Returns ContactPattern::grow's answer.
extern "C" int shim_grow(int nLive, const int* live, int nAhead, const int* ahead, int* asked)
{
    const NodePairs l = unflat(std::max(nLive, 0), live);
    *asked = 0;
    return g_pat.grow(nLive < 0 ? nullptr : &l, [&] {
        *asked = 1;
        return unflat(nAhead, ahead);
    });
}
extern "C" int shim_size() { return (int)g_pat.pairs().size(); }
extern "C" int shim_fetch(int* pairs, int* flat)
{
    std::copy(g_pat.flat().begin(), g_pat.flat().end(), flat);
    flatten(g_pat.pairs(), pairs);
    return (int)g_pat.flat().size();
}
