// TEST INFRASTRUCTURE (host only): the aggregation unit of the two-level preconditioner (ipc_amd/csrc/pcg_coarse.cpp) behind plain C calls for
// tests/test_pcg_coarse.py.  Built by the test with g++.
#include "../../ipc_amd/csrc/pcg_coarse.h"
#include <algorithm>
using namespace ipcgpu;
static PcgCoarse g_c;
extern "C" void shim_build(int nNodes, const int* ja, const int* rowBase, const int* rowLen, const unsigned char* fixed)
{
    g_c = PcgCoarse();
    g_c.build(nNodes, ja, rowBase, rowLen, fixed);
}
// out4 = { aggregates, coarse nnz, aggregate pairs, list entries }
extern "C" void shim_dims(int* out4)
{
    out4[0] = g_c.nAgg, out4[1] = (int)g_c.cja.size(), out4[2] = (int)g_c.pairI.size(), out4[3] = (int)g_c.entSlot.size();
}
static void put(const std::vector<int>& v, int* out)
{
    if (out) std::copy(v.begin(), v.end(), out);
}
extern "C" void shim_aggregates(int* aggOf, int* aggPtr, int* aggNodes, int* aggFree)
{
    put(g_c.aggOf, aggOf), put(g_c.aggPtr, aggPtr), put(g_c.aggNodes, aggNodes), put(g_c.aggFree, aggFree);
}
extern "C" void shim_coarse_pattern(int* cia, int* cja, int* cRowBase, int* cRowLen)
{
    put(g_c.cia, cia), put(g_c.cja, cja), put(g_c.cRowBase, cRowBase), put(g_c.cRowLen, cRowLen);
}
extern "C" void shim_pairs(int* pairI, int* pairJ, int* pairPtr, int* pairSlot)
{
    put(g_c.pairI, pairI), put(g_c.pairJ, pairJ), put(g_c.pairPtr, pairPtr), put(g_c.pairSlot, pairSlot);
}
extern "C" void shim_entries(int* slot, int* row, int* col, int* trans)
{
    put(g_c.entSlot, slot), put(g_c.entRow, row), put(g_c.entCol, col), put(g_c.entTrans, trans);
}
