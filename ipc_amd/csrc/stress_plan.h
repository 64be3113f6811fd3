// Node -> element incidence list of the nodal stress pass (ipcgpu_elastic_stress; k_stress_nodes of nh_kernels.hip) in CSR form: row v holds the
// elements that have node v among their four, in ascending element index -- the order the kernel sums in.  Pure integer logic, host only (no HIP
// header: tests/test_stress_plan_host.py builds it with g++).
#pragma once
#include <vector>

namespace ipcgpu {

// F: column-major nT x 4 (F[t + nT k] = node k of element t), as HipMesh keeps it.  ptr gets nV + 1 entries with ptr[0] = 0 and ptr[nV] = 4 nT, elems
// 4 nT; a node without an element has an empty row.  false (and both vectors empty): a negative size or a node index outside [0, nV).
bool buildNodeElementIncidence(int nV, int nT, const int* F, std::vector<int>& ptr, std::vector<int>& elems);

} // namespace ipcgpu
