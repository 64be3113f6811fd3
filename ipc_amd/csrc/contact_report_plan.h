// Row plan of the contact report (ipcgpu_contact_report; the "contact report" section of hip_contact.hip): which key a pair of components, or a component
// and a half-space, has in the dense histogram, the order of the rows, the compaction of a histogram into rows and the slice list of the rows' record
// ranges.  Pure integer logic, host only (no HIP header: tests/test_contact_report_plan_host.py builds it with g++); the key formula alone is also
// compiled for the device, so that the record kernels and the host decode one encoding.
#pragma once
#include "report_plan.h"
#include <vector>

#if defined(__HIPCC__)
#define IPCGPU_CRP_HD __host__ __device__
#else
#define IPCGPU_CRP_HD
#endif

namespace ipcgpu {

// A row is an unordered pair: two components (a, b), a <= b, or component a and half-space h, written (a, -1 - h).  Rows ascend by a; inside one a the
// component rows b = a .. nComp - 1 come first, then the half-space rows h = 0 .. nHalf - 1: the key of a pair is its position in that order.
constexpr long long CONTACT_REPORT_MAX_KEYS = 1LL << 22; // dense counters and starts: 48 MB at the limit (about 2 890 components without a half-space)

inline long long contactReportKeyCount(long long nComp, long long nHalf) { return nComp * (nComp + 1) / 2 + nComp * nHalf; }
// first key of component a's rows (a = nComp: the key count)
IPCGPU_CRP_HD inline int contactReportRowBase(int nComp, int nHalf, int a) { return a * nComp - a * (a - 1) / 2 + a * nHalf; }
// b >= a: a component; b < 0: half-space -1 - b
IPCGPU_CRP_HD inline int contactReportKey(int nComp, int nHalf, int a, int b) { return contactReportRowBase(nComp, nHalf, a) + (b >= 0 ? b - a : nComp - a + (-1 - b)); }
// the inverse; false: key outside [0, key count)
bool contactReportPair(int nComp, int nHalf, int key, int* a, int* b);

// histogram -> rows: the keys with a non-zero count in ascending order and their accumulated ends (what k_creport_publish writes on the device)
void compactContactHistogram(int nKeys, const int* count, std::vector<int>& rowKey, std::vector<int>& rowEnd);
// true: keys strictly ascending inside [0, nKeys), ends strictly ascending from above zero
bool contactReportRowsValid(int nKeys, int nRows, const int* rowKey, const int* rowEnd);
// the rows' (a, b) pairs (2 per row) and the slices of their record ranges: at most `width` records each, none spanning two rows (buildReportSlices on
// the accumulated ends); sliceStart[r] .. sliceStart[r + 1] is row r's range in the list
void buildContactReportPlan(int nComp, int nHalf, int nRows, const int* rowKey, const int* rowEnd, int width, std::vector<int>& pairs,
    std::vector<ReportSlice>& slices, std::vector<int>& sliceStart);

} // namespace ipcgpu
