// TEST INFRASTRUCTURE -- every member of HipLinSysSolver compiled (explicit instantiation), the iterative selection among them, against
// whichever LinSysSolver.hpp is on the include path: the stand-ins of tests/mock_ipc or the reference's own header.  Nothing touches the GPU.
#include "HipLinSysSolver.hpp"
#include <cstdio>

template class IPC::HipLinSysSolver<Eigen::VectorXi, Eigen::VectorXd>;

int main()
{
    typedef IPC::HipLinSysSolver<Eigen::VectorXi, Eigen::VectorXd> S;
    void (S::*sel)(bool) = &S::setIterative;
    void (S::*par)(double, int, int, int) = &S::setIterativeParameters;
    static_assert(IPCGPU_SOLVER_PCG == 2 && IPCGPU_PRECOND_BLOCK_JACOBI == 0 && IPCGPU_PRECOND_LAGGED_CHOLESKY == 1, "ipcgpu.h");
    std::printf("iterative adapter compiled and linked (%d)\n", (int)(sel != nullptr && par != nullptr));
    return 0;
}
