// What every codimensional energy term (shell_kernels.h, shell_limit_kernels.h, rod_kernels.h, attach_kernels.h) reads beside its own constants: positions, Dirichlet types
// and the CSR map.  Each term's view derives from this base; HipOptimizer::codimBase fills it once.  Plain host and device data only.
// A view names its own fields in a struct of its own and derives from that FIRST and from CodimBase second, so that the shared fields lie behind the
// term's own in the kernel argument, where they lay before there was a base: with them in front the compiler orders the loads, and behind them the
// atomic adds, of four scatter kernels differently, and their sums then agree with the earlier ones to rounding only (tests/test_gpu_codim_parity.py).
#pragma once

namespace ipcgpu {

struct CodimBase {
    const double* x; // positions, xyz interleaved
    const int* dbc; // nV, DirichletBCType
    // CSR map (valid after set_pattern; only the Hessian kernels read it)
    const int* rowBase; // nV: ia[3 v]
    const int* rowLen; // nV: ia[3 v + 1] - ia[3 v]
    const int* ja;
};

} // namespace ipcgpu
