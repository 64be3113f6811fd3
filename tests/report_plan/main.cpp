// Stand-alone driver of ipc_amd/csrc/report_plan.cpp (the slice list of the system report) for tests/test_system_report_host.py.
// stdin: any number of cases `width n nComp end_0 .. end_{nComp-1}`; stdout per case: `valid` (0 | 1), and for a valid table the number of slices,
// the slices as `comp begin end` triples and the nComp + 1 slice starts, all on one line.
#include "report_plan.h"
#include <cstdio>
#include <vector>

int main()
{
    int width, n, nComp;
    while (std::scanf("%d %d %d", &width, &n, &nComp) == 3) {
        std::vector<int> end((size_t)(nComp > 0 ? nComp : 0));
        for (int& e : end)
            if (std::scanf("%d", &e) != 1) return 2;
        if (!ipcgpu::reportEndsValid(nComp, end.data(), n)) {
            std::printf("0\n");
            continue;
        }
        std::vector<ipcgpu::ReportSlice> slices;
        std::vector<int> start;
        ipcgpu::buildReportSlices(nComp, end.data(), width, slices, start);
        std::printf("1 %zu", slices.size());
        for (const auto& s : slices) std::printf(" %d %d %d", s.comp, s.begin, s.end);
        for (int s : start) std::printf(" %d", s);
        std::printf("\n");
    }
    return 0;
}
