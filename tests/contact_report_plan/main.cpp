// Stand-alone driver of ipc_amd/csrc/contact_report_plan.cpp for tests/test_contact_report_plan_host.py.  One case per input line:
//   K nComp nHalf                    -> key count, then per key "a b key'" (key' = the key of the decoded pair), then the decode status of -1 and of the key count
//   H nComp nHalf width n c_0..c_n-1 -> rows, then per row "a b end", slices, then per slice "row begin end", then the nRows + 1 slice starts
#include "contact_report_plan.h"
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

int main()
{
    using namespace ipcgpu;
    std::string op;
    while (std::cin >> op) {
        int nComp, nHalf;
        std::cin >> nComp >> nHalf;
        if (op == "K") {
            const int nKeys = (int)contactReportKeyCount(nComp, nHalf);
            std::printf("%d", nKeys);
            for (int k = 0; k < nKeys; ++k) {
                int a = -7, b = -7;
                if (!contactReportPair(nComp, nHalf, k, &a, &b)) return 2;
                std::printf(" %d %d %d", a, b, contactReportKey(nComp, nHalf, a, b));
            }
            int a, b;
            std::printf(" %d %d\n", (int)contactReportPair(nComp, nHalf, -1, &a, &b), (int)contactReportPair(nComp, nHalf, nKeys, &a, &b));
        }
        else {
            int width, n;
            std::cin >> width >> n;
            std::vector<int> count(n), rowKey, rowEnd, pairs, sliceStart;
            for (int& c : count) std::cin >> c;
            compactContactHistogram(n, count.data(), rowKey, rowEnd);
            const int nRows = (int)rowKey.size();
            if (!contactReportRowsValid(n, nRows, rowKey.data(), rowEnd.data())) return 3;
            std::vector<ReportSlice> slices;
            buildContactReportPlan(nComp, nHalf, nRows, rowKey.data(), rowEnd.data(), width, pairs, slices, sliceStart);
            std::printf("%d", nRows);
            for (int r = 0; r < nRows; ++r) std::printf(" %d %d %d", pairs[2 * r], pairs[2 * r + 1], rowEnd[r]);
            std::printf(" %d", (int)slices.size());
            for (const ReportSlice& s : slices) std::printf(" %d %d %d", s.comp, s.begin, s.end);
            for (int s : sliceStart) std::printf(" %d", s);
            std::printf("\n");
        }
    }
    return 0;
}
