// Stand-alone driver of ipc_amd/csrc/contact_groups.cpp (validation of the contact-group tables, the per-node packed words) for
// tests/test_contact_groups_host.py.
// stdin: any number of cases `nV nCompTable end[nCompTable] nComp group[nComp] nGroups collide[nGroups^2] hasScale (scale[nGroups^2])`; a negative
// nGroups sends null tables with |nGroups|.  stdout per case one line: `0 <reason>` for rejected tables, else `1`, the nV words (as unsigned) and the
// 256 friction scales.
#include "contact_groups.h"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

int main()
{
    int nV, nTable;
    while (std::scanf("%d %d", &nV, &nTable) == 2) {
        std::vector<int> ends(nTable > 0 ? (size_t)nTable : 0);
        for (int& e : ends)
            if (std::scanf("%d", &e) != 1) return 2;
        int nComp, nGroups, hasScale;
        if (std::scanf("%d", &nComp) != 1) return 2;
        std::vector<int> group(nComp > 0 ? (size_t)nComp : 0);
        for (int& g : group)
            if (std::scanf("%d", &g) != 1) return 2;
        if (std::scanf("%d", &nGroups) != 1) return 2;
        const bool nullTables = nGroups < 0;
        const size_t n2 = nGroups > 0 ? (size_t)nGroups * (size_t)nGroups : 0;
        std::vector<unsigned char> collide(n2);
        for (unsigned char& c : collide) {
            int v;
            if (std::scanf("%d", &v) != 1) return 2;
            c = (unsigned char)v;
        }
        if (std::scanf("%d", &hasScale) != 1) return 2;
        std::vector<double> scale(hasScale ? n2 : 0);
        for (double& s : scale)
            if (std::scanf("%lf", &s) != 1) return 2;
        std::vector<int> words;
        std::vector<double> scale16;
        std::string err;
        const bool ok = ipcgpu::buildContactGroupWords(nV, nTable, ends.empty() ? nullptr : ends.data(), nComp, nullTables ? nullptr : group.data(),
            std::abs(nGroups), nullTables ? nullptr : collide.data(), hasScale ? scale.data() : nullptr, words, scale16, err);
        if (!ok) {
            if (!words.empty() || !scale16.empty() || err.empty()) return 3;
            std::printf("0 %s\n", err.c_str());
            continue;
        }
        if ((int)words.size() != nV || scale16.size() != 256) return 3;
        std::printf("1");
        for (int w : words) std::printf(" %u", (unsigned)w);
        for (double s : scale16) std::printf(" %.17g", s);
        std::printf("\n");
    }
    return 0;
}
