#include "pcg_coarse.h"
#include <algorithm>
#include <numeric>

namespace ipcgpu {

void PcgCoarse::build(int nNodes_, const int* ja, const int* rowBase, const int* rowLen, const unsigned char* fixed)
{
    nNodes = nNodes_;
    // ---- the node graph, both directions, neighbours ascending (counting pass, fill pass: the lower neighbours arrive in ascending order, the upper ones are)
    std::vector<int> nbPtr(nNodes + 1, 0);
    auto upper = [&](int u, auto&& f) {
        for (int k = rowBase[u] + 3; k < rowBase[u] + rowLen[u]; k += 3) f(ja[k] / 3, k);
    };
    for (int u = 0; u < nNodes; ++u)
        upper(u, [&](int w, int) { nbPtr[u + 1]++, nbPtr[w + 1]++; });
    for (int v = 0; v < nNodes; ++v) nbPtr[v + 1] += nbPtr[v];
    std::vector<int> nb(nbPtr[nNodes]), pos(nbPtr.begin(), nbPtr.end() - 1);
    for (int u = 0; u < nNodes; ++u)
        upper(u, [&](int w, int) { nb[pos[w]++] = u; });
    for (int u = 0; u < nNodes; ++u)
        upper(u, [&](int w, int) { nb[pos[u]++] = w; });

    // ---- greedy aggregation, nodes in index order
    aggOf.assign(nNodes, -1);
    nAgg = 0;
    // a node none of whose neighbours is aggregated yet seeds an aggregate with all of them
    for (int v = 0; v < nNodes; ++v) {
        if (aggOf[v] >= 0 || nbPtr[v] == nbPtr[v + 1]) continue;
        bool clear = true;
        for (int k = nbPtr[v]; k < nbPtr[v + 1] && clear; ++k) clear = aggOf[nb[k]] < 0;
        if (!clear) continue;
        aggOf[v] = nAgg;
        for (int k = nbPtr[v]; k < nbPtr[v + 1]; ++k) aggOf[nb[k]] = nAgg;
        ++nAgg;
    }
    // a leftover node joins the seeded aggregate that holds most of its neighbours (the smallest id among equals); it has one, or it would have been a seed
    {
        const std::vector<int> seeded(aggOf);
        std::vector<int> ids;
        for (int v = 0; v < nNodes; ++v) {
            if (seeded[v] >= 0) continue;
            ids.clear();
            for (int k = nbPtr[v]; k < nbPtr[v + 1]; ++k)
                if (seeded[nb[k]] >= 0) ids.push_back(seeded[nb[k]]);
            std::sort(ids.begin(), ids.end());
            int best = -1, bestCnt = 0;
            for (size_t i = 0; i < ids.size();) {
                size_t j = i;
                while (j < ids.size() && ids[j] == ids[i]) ++j;
                if ((int)(j - i) > bestCnt) best = ids[i], bestCnt = (int)(j - i);
                i = j;
            }
            aggOf[v] = best >= 0 ? best : nAgg++; // (no neighbour at all: a singleton)
        }
    }
    aggPtr.assign(nAgg + 1, 0);
    aggFree.assign(nAgg, 0);
    for (int v = 0; v < nNodes; ++v) {
        aggPtr[aggOf[v] + 1]++;
        if (!fixed || !fixed[v]) aggFree[aggOf[v]]++;
    }
    for (int I = 0; I < nAgg; ++I) aggPtr[I + 1] += aggPtr[I];
    aggNodes.resize(nNodes);
    pos.assign(aggPtr.begin(), aggPtr.end() - 1);
    for (int v = 0; v < nNodes; ++v) aggNodes[pos[aggOf[v]]++] = v;

    // ---- the fine blocks by aggregate pair: a stable sort keeps the order of the fine storage inside a pair
    struct Ent {
        long long key;
        int slot, row, col, trans;
    };
    std::vector<Ent> ents;
    ents.reserve(nb.size() / 2 + nNodes);
    for (int u = 0; u < nNodes; ++u) {
        ents.push_back({ (long long)aggOf[u] * nAgg + aggOf[u], rowBase[u], u, u, 0 });
        upper(u, [&](int w, int k) {
            const int I = aggOf[u], J = aggOf[w];
            ents.push_back({ (long long)std::min(I, J) * nAgg + std::max(I, J), k, u, w, I > J ? 1 : 0 });
        });
    }
    std::stable_sort(ents.begin(), ents.end(), [](const Ent& a, const Ent& b) { return a.key < b.key; });
    pairI.clear(), pairJ.clear(), pairPtr.clear();
    entSlot.resize(ents.size()), entRow.resize(ents.size()), entCol.resize(ents.size()), entTrans.resize(ents.size());
    for (size_t e = 0; e < ents.size(); ++e) {
        if (e == 0 || ents[e].key != ents[e - 1].key) {
            pairI.push_back((int)(ents[e].key / nAgg));
            pairJ.push_back((int)(ents[e].key % nAgg));
            pairPtr.push_back((int)e);
        }
        entSlot[e] = ents[e].slot, entRow[e] = ents[e].row, entCol[e] = ents[e].col, entTrans[e] = ents[e].trans;
    }
    pairPtr.push_back((int)ents.size());
    const int nPairs = (int)pairI.size();

    // ---- the coarse pattern.  Upper neighbours of coarse node 2 I: 2 I + 1, then (2 J, 2 J + 1) for every pair I < J; of 2 I + 1: the same without the first
    std::vector<int> nUp(nAgg, 0);
    for (int p = 0; p < nPairs; ++p)
        if (pairI[p] != pairJ[p]) nUp[pairI[p]]++;
    const int nc = 2 * nAgg;
    cRowBase.assign(nc, 0), cRowLen.assign(nc, 0), cia.assign(3 * (size_t)nc + 1, 0);
    for (int c = 0; c < nc; ++c) {
        const int len = 3 + 3 * (2 * nUp[c / 2] + (c % 2 == 0 ? 1 : 0));
        cRowBase[c] = cia[3 * c], cRowLen[c] = len;
        cia[3 * c + 1] = cia[3 * c] + len;
        cia[3 * c + 2] = cia[3 * c + 1] + len - 1;
        cia[3 * c + 3] = cia[3 * c + 2] + len - 2;
    }
    cja.resize(cia[3 * (size_t)nc]);
    pairSlot.assign(4 * (size_t)nPairs, -1);
    std::vector<int> up; // the upper coarse-node neighbours of the current aggregate's translation node
    for (int p = 0; p < nPairs;) {
        const int I = pairI[p];
        up.assign(1, 2 * I + 1);
        int k = 0;
        for (; p < nPairs && pairI[p] == I; ++p) {
            const int J = pairJ[p], t = cRowBase[2 * I], r = cRowBase[2 * I + 1];
            if (J == I) { // (the first pair of I: the lists are sorted and every node has its diagonal block)
                pairSlot[4 * p + 0] = t, pairSlot[4 * p + 1] = t + 3, pairSlot[4 * p + 3] = r;
                continue;
            }
            pairSlot[4 * p + 0] = t + 3 + 3 * (1 + 2 * k), pairSlot[4 * p + 1] = t + 3 + 3 * (2 + 2 * k);
            pairSlot[4 * p + 2] = r + 3 + 3 * (2 * k), pairSlot[4 * p + 3] = r + 3 + 3 * (2 * k + 1);
            up.push_back(2 * J), up.push_back(2 * J + 1);
            ++k;
        }
        for (int half = 0; half < 2; ++half) {
            const int c = 2 * I + half;
            for (int row = 0; row < 3; ++row) {
                int q = cia[3 * c + row];
                for (int col = row; col < 3; ++col) cja[q++] = 3 * c + col;
                for (size_t i = half; i < up.size(); ++i)
                    for (int col = 0; col < 3; ++col) cja[q++] = 3 * up[i] + col;
            }
        }
    }
}

} // namespace ipcgpu
