// Row plan of the contact report: see contact_report_plan.h.  Host only.
#include "contact_report_plan.h"
#include <cstddef>

namespace ipcgpu {

bool contactReportPair(int nComp, int nHalf, int key, int* a, int* b)
{
    if (nComp < 1 || nHalf < 0 || key < 0 || key >= contactReportRowBase(nComp, nHalf, nComp)) return false;
    int lo = 0, hi = nComp - 1; // the last a whose row base is <= key
    while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        if (contactReportRowBase(nComp, nHalf, mid) <= key) lo = mid;
        else hi = mid - 1;
    }
    const int off = key - contactReportRowBase(nComp, nHalf, lo);
    *a = lo;
    *b = off < nComp - lo ? lo + off : -1 - (off - (nComp - lo));
    return true;
}

void compactContactHistogram(int nKeys, const int* count, std::vector<int>& rowKey, std::vector<int>& rowEnd)
{
    rowKey.clear();
    rowEnd.clear();
    int end = 0;
    for (int k = 0; k < nKeys; ++k)
        if (count[k] > 0) {
            end += count[k];
            rowKey.push_back(k);
            rowEnd.push_back(end);
        }
}

bool contactReportRowsValid(int nKeys, int nRows, const int* rowKey, const int* rowEnd)
{
    if (nRows < 0 || (nRows && (!rowKey || !rowEnd))) return false;
    int key = -1, end = 0;
    for (int r = 0; r < nRows; ++r) {
        if (rowKey[r] <= key || rowKey[r] >= nKeys || rowEnd[r] <= end) return false;
        key = rowKey[r];
        end = rowEnd[r];
    }
    return true;
}

void buildContactReportPlan(int nComp, int nHalf, int nRows, const int* rowKey, const int* rowEnd, int width, std::vector<int>& pairs,
    std::vector<ReportSlice>& slices, std::vector<int>& sliceStart)
{
    pairs.assign(2 * (std::size_t)nRows, 0);
    for (int r = 0; r < nRows; ++r) (void)contactReportPair(nComp, nHalf, rowKey[r], &pairs[2 * (std::size_t)r], &pairs[2 * (std::size_t)r + 1]);
    slices.clear();
    if (nRows) buildReportSlices(nRows, rowEnd, width, slices, sliceStart);
    else sliceStart.assign(1, 0);
}

} // namespace ipcgpu
