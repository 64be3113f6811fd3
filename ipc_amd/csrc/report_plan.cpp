// Slice list of the system report: see report_plan.h.  Host only.
#include "report_plan.h"
#include <cstddef>

namespace ipcgpu {

bool reportEndsValid(int nComp, const int* compEnd, int n)
{
    if (nComp < 1 || !compEnd) return false;
    int prev = 0;
    for (int c = 0; c < nComp; ++c) {
        if (compEnd[c] < prev) return false;
        prev = compEnd[c];
    }
    return prev == n;
}

void buildReportSlices(int nComp, const int* compEnd, int width, std::vector<ReportSlice>& slices, std::vector<int>& sliceStart)
{
    sliceStart.assign((std::size_t)nComp + 1, (int)slices.size());
    for (int c = 0; c < nComp; ++c) {
        const int e = compEnd[c];
        for (int b = c ? compEnd[c - 1] : 0; b < e;) {
            const int next = e - b > width ? b + width : e; // (b + width may not fit an int near INT_MAX)
            slices.push_back(ReportSlice{ c, b, next });
            b = next;
        }
        sliceStart[c + 1] = (int)slices.size();
    }
}

} // namespace ipcgpu
