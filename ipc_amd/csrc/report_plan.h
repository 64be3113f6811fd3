// Slice list of the system report (ipcgpu_opt_system_report; k_report_slices / k_report_components of nh_kernels.hip): the index range [0, n) of the
// nodes, or of the elements, cut into slices of at most `width` entries none of which spans two components.  Pure integer logic, host only (no HIP
// header: tests/test_system_report_host.py builds it with g++).
#pragma once
#include <vector>

namespace ipcgpu {

struct ReportSlice {
    int comp, begin, end; // entries [begin, end) of component comp, 0 < end - begin <= width
};

// compEnd[nComp]: accumulated ends as the reference stores them (compVAccSize / compFAccSize, main.cpp:1111-1112).
// true: non-decreasing, none negative, the last one equal to n
bool reportEndsValid(int nComp, const int* compEnd, int n);

// Appends the slices of every component in index order, component c's from its begin in steps of `width` (an empty component has none), and sets
// sliceStart[c] .. sliceStart[c + 1] to component c's range in the list (nComp + 1 entries; the list may already hold other slices).
void buildReportSlices(int nComp, const int* compEnd, int width, std::vector<ReportSlice>& slices, std::vector<int>& sliceStart);

} // namespace ipcgpu
