// Preconditioned conjugate gradients on the symmetric-upper CSR of HipLinSysSolver (solver type 2; the reference's iterative choice is
// AMGCLSolver.cpp:24-25, 173-241: CG, relative tolerance, iteration cap, zero initial guess).  Kernels and launchers only: the loop, the
// preconditioner choice and the factor's ageing live in HipLinSysSolver (hip_linsys.hip).
#pragma once
#include "common.h"

namespace ipcgpu {

// What the device keeps of a running solve.  Every kernel of the iteration returns at once when `done` is set, so the launches a batch
// still holds behind the converged (or broken-down) iteration cost their dispatch only.
struct PcgState {
    double rz, rr, pAp, alpha, beta; // r.z, r.r of the current residual, p.Ap, the two step scalars
    double bb, tol2; // |b|^2, (rel_tol |b|)^2
    double trueRes2; // |b - A x|^2 recomputed with one extra product once the iteration has ended
    int iter, maxIter;
    int done; // 0 running, 1 converged, 2 p.Ap <= 0 (not positive definite), 3 iteration cap
    int pad;
};
enum { PCG_RUNNING = 0, PCG_CONVERGED = 1, PCG_BREAKDOWN = 2, PCG_MAXITER = 3 };
constexpr int PCG_STATE_WORDS = (int)(sizeof(PcgState) / 4);

// The strictly lower part of the matrix, read from the upper storage: per row (scalar patterns) or per node (3x3 block patterns) the
// list of value slots that hold its transposed entries.  Built in one O(nnz) host pass per pattern (PcgPattern::build).
struct PcgPattern {
    int nRows = 0, nNodes = 0;
    bool blocks = false; // node block rows (rowBase / rowLen exist) or scalar rows (set_pattern_csr)
    long long nnz = 0;
    // blocks: lowPtr[nNodes + 1]; lowNode[k] = the earlier node u, lowSlot[k] = slot of the block's first entry in row 3 u, lowLen[k] = rowLen[u]
    // scalar: lowPtr[nRows + 1]; lowNode[k] = the earlier row, lowSlot[k] = the value slot
    DevBuf<int> lowPtr, lowNode, lowSlot, lowLen;
    DevBuf<int> diagSlot; // [6][nNodes]: slots of (00, 01, 02, 11, 12, 22) of every 3x3 diagonal block, -1 where the pattern has none
    DevBuf<double> dinv; // [6][nNodes]: the inverses of the diagonal blocks (symmetric, same order)
    void build(int nRows, const std::vector<int>& ia, const std::vector<int>& ja, const std::vector<int>& rowBase, const std::vector<int>& rowLen,
        hipStream_t s);
};

struct PcgWork {
    DevBuf<double> r, z, p0, p1, Ap, partial;
    DevBuf<PcgState> state;
    DevBuf<int> flag;
    PinnedBuf<PcgState> hState;
    int nPartial = 0;
    void ensure(int nRows);
};

// y = A x from the upper storage, no atomics, fixed summation order.  With pOut != nullptr the vector multiplied is p = x + beta pOld (beta from
// the state; first = 1: p = x; x is CG's z), written to pOut on the way, and the partial sums of p.Ap go to partial[0 .. pcg_symv_grid).
// gate: 0 always (st may be nullptr), 1 only while the iteration runs, 2 only once it has ended.
void launch_pcg_symv(const PcgPattern& P, const int* ia, const int* ja, const int* rowBase, const int* rowLen, const double* a, const double* x,
    const double* pOld, double* pOut, int first, double* y, double* partial, const PcgState* st, int gate, hipStream_t s);
int pcg_symv_grid(const PcgPattern& P);
// inverts the 3x3 diagonal blocks into P.dinv; flag[0] |= 1 when one of them is not positive definite
void launch_pcg_invert_blocks(PcgPattern& P, const double* a, int* flag, hipStream_t s);
// start of a solve: x = 0, r = b (restart: x kept, r = b - yAx), block Jacobi: z = Dinv r; then the state of iteration 0 (restart: the
// iteration count and the tolerance stay)
void launch_pcg_begin(const PcgPattern& P, bool jacobi, bool restart, const double* b, const double* yAx, double* x, PcgWork& W, double relTol, int maxIter,
    hipStream_t s);
// lagged factor: rz = r.z for a z computed elsewhere (first = 1: initial rz; else beta = rz_new / rz)
void launch_pcg_rz(int n, const double* r, const double* z, PcgWork& W, int first, hipStream_t s);
// alpha = rz / pAp from the product's partials (nPartialAp of them); p.Ap <= 0 ends the solve with PCG_BREAKDOWN
void launch_pcg_alpha(PcgWork& W, int nPartialAp, hipStream_t s);
// x += alpha p, r -= alpha Ap, (block Jacobi: z = Dinv r, r.z), r.r; then the convergence test, the iteration count and (block Jacobi) beta
void launch_pcg_update(const PcgPattern& P, bool jacobi, const double* p, const double* Ap, double* x, PcgWork& W, hipStream_t s);
// once the iteration has ended (runs only when st->done): |b - y|^2 with y = A x into the state; the state into mapped host memory
void launch_pcg_residual(int n, const double* b, const double* y, PcgWork& W, hipStream_t s);
void launch_pcg_publish(PcgWork& W, hipStream_t s);

// ---- two-level preconditioner (IPCGPU_PRECOND_TWO_LEVEL): z = Dinv r + P Ac^-1 P^T r with Ac = P^T A P -------------------------------------------
// The device copy of a PcgCoarse (pcg_coarse.h) and what factorize() computes from the current positions.  Node i of aggregate I contributes the 3x6
// block [ I | S(x_i - c_I) ] to P (S(d) w = d x w, c_I the centroid of the aggregate's free nodes); a fixed node contributes nothing; an aggregate with
// fewer than 4 free nodes has no rotation columns and an identity in its rotation block of Ac.
struct PcgCoarseDev {
    int nNodes = 0, nAgg = 0, nPairs = 0;
    DevBuf<int> aggOf, aggPtr, aggNodes, pairIJ, pairPtr, pairSlot, cRowLen;
    DevBuf<int> ent; // [4 per list entry] slot, row node, column node, transposed
    DevBuf<double> geo; // [4][nNodes]: x_i - c_I (zero where the aggregate has no rotation columns or the node is fixed), and the weight 1 (free) / 0 (fixed)
    DevBuf<int> aggFlags; // per aggregate: bit 0 it has a free node (translation columns), bit 1 it has 4 or more (rotation columns)
    DevBuf<double> rc, xc; // [6 nAgg] restricted residual, coarse solution
    void upload(const struct PcgCoarse& C, hipStream_t s);
};
// once per factorize(): centroids, offsets and flags from the positions (xyz per node) and the Dirichlet types (0 = free) the context holds
void launch_pcg_coarse_geometry(PcgCoarseDev& C, const double* x, const int* dbcType, hipStream_t s);
// Ac = P^T A P from the fine values a (upper storage, node block rows) into the coarse solver's value array ca: one lane group per aggregate pair walks
// the pair's list, the 36 sums are reduced over the group in a fixed order, every coarse slot is written exactly once
void launch_pcg_galerkin(const PcgCoarseDev& C, const int* rowLen, const double* a, double* ca, hipStream_t s);
// rc = P^T r, one lane group per aggregate over its node list (gate as launch_pcg_symv)
void launch_pcg_restrict(const PcgCoarseDev& C, const double* r, double* rc, const PcgState* st, int gate, hipStream_t s);
// z = Dinv r + P xc and r.z (first = 1: the initial r.z; else beta = rz_new / rz), as launch_pcg_rz for the lagged factor
void launch_pcg_prolong(const PcgPattern& P, const PcgCoarseDev& C, const double* xc, PcgWork& W, int first, int gate, hipStream_t s);

} // namespace ipcgpu
