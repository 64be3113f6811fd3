/* ipcgpu.h -- C ABI of the MI355X-native IPC Newton hot path (libipcgpu.so).
 *
 * The reference has no FFI: its hot path sits behind three C++ class interfaces
 * (SURVEY.md 8b).  A maintainer drops this library in by adding three thin adapter
 * subclasses (shown in INTEGRATION.md) that forward to the entry points below:
 *
 *   LinSysSolver<VectorXi,VectorXd>   src/LinSysSolver/LinSysSolver.hpp:31-467
 *   Energy<3> / NeoHookeanEnergy<3>   src/Energy/Energy.hpp:27-138
 *   Optimizer<3>                      src/TimeStepper/Optimizer.hpp:28-283
 *
 * Conventions
 *   - plain pointers and sizes only; every function returns an int status:
 *       IPCGPU_OK 0, IPCGPU_NOT_PD 1 (factorize: matrix not positive definite,
 *       the reference's `factorize() == false`, CHOLMODSolver.cpp:130-137),
 *       negative = error (message via ipcgpu_last_error()).  No exceptions cross
 *       the boundary.  One opaque context per Optimizer; a context is not thread-safe.
 *   - layouts are the reference's: V is column-major nV x 3 (Eigen::MatrixXd,
 *     Mesh.hpp:61), F is column-major nT x 4 int32 (Mesh.hpp:64), nodal vectors
 *     are xyzxyz... of length 3 nV (Optimizer.hpp:91-92), the matrix is the
 *     symmetric-UPPER CSR with 3x3 node blocks of LinSysSolver.hpp:46-150, 0-based.
 *   - host pointers unless the name ends in _dev.  Device state (positions, CSR
 *     values, factor) stays resident in HBM between calls.
 *   - all arithmetic is fp64, all indices int32, like the reference.
 */
#ifndef IPCGPU_H
#define IPCGPU_H

#ifdef __cplusplus
extern "C" {
#endif

#define IPCGPU_OK 0
#define IPCGPU_NOT_PD 1
#define IPCGPU_ERR_ARG -1
#define IPCGPU_ERR_HIP -2
#define IPCGPU_ERR_STATE -3
#define IPCGPU_ERR_UNSUPPORTED -4

typedef struct ipcgpu_ctx ipcgpu_ctx;

/* DirichletBCType, src/Mesh.hpp:41-45 */
enum { IPCGPU_NOT_DBC = 0, IPCGPU_DBC_ZERO = 1, IPCGPU_DBC_NONZERO = 2 };

/* linear-solver back ends selectable per context (the reference selects CHOLMOD / EIGEN /
 * AMGCL through LinSysSolver::create, LinSysSolver.cpp:10-28) */
enum { IPCGPU_SOLVER_MULTIFRONTAL = 0, IPCGPU_SOLVER_ROCSOLVER_CSRRF = 1, IPCGPU_SOLVER_PCG = 2 };
/* preconditioners of IPCGPU_SOLVER_PCG (ipcgpu_linsys_set_iterative) */
enum { IPCGPU_PRECOND_BLOCK_JACOBI = 0, IPCGPU_PRECOND_LAGGED_CHOLESKY = 1, IPCGPU_PRECOND_TWO_LEVEL = 2 };

const char* ipcgpu_last_error(void);
int ipcgpu_version(void);

/* ---- context ------------------------------------------------------------------------ */
int ipcgpu_ctx_create(int device_id, ipcgpu_ctx** out);
int ipcgpu_ctx_destroy(ipcgpu_ctx*);
int ipcgpu_ctx_set_solver(ipcgpu_ctx*, int solver_type);
/* Sharding of the assembly for multi-GPU runs, one context per rank.  Together with ipcgpu_linsys_set_shard (same world) this is
 * OWNER-COMPUTES ROWS: the rank assembles exactly the CSR rows its fronts read (the rows of the nodes its subtrees eliminate plus the separator rows
 * above the cut; elements and contact stencils on a cut are evaluated by both sides) and NO matrix value crosses ranks -- see ipcgpu_opt_comm_stats
 * below.  Energies, step bounds and the CCD sweeps are split by index ranges (elements [nT rank / world, nT (rank + 1) / world) in the order given to
 * set_mesh) and combined by scalar all-reduces through the hook of ipcgpu_opt_set_allreduce[_stream].  Without a sharded solver (and for runs with
 * lagged damping) the element pass is split by that same element range and the partial gradient / matrix values are summed by the hook.
 * A consumer of the WHOLE matrix on an owner-computes context (ipcgpu_linsys_get_values / multiply / precondition_diag) gets IPCGPU_ERR_STATE until
 * ipcgpu_opt_complete_matrix has been called on every rank.  Default: rank 0 of 1. */
int ipcgpu_ctx_set_shard(ipcgpu_ctx*, int rank, int world_size);

/* ---- tet-mesh files (host only, no GPU) ------------------------------------------------ */
/* IglUtils::readTetMesh (src/Utils/IglUtils.cpp:451-584): Gmsh MSH 4.1 / 2.2 ASCII (the MshIO path) and the reference's own
 * "msh 4.0" dialect with its optional $Surface section; nodes in file order, elements by tag - 1.  The surface is taken from
 * $Surface when the dialect carries it, otherwise found as in IglUtils::findSurfaceTris (:203-233) in (tet, local face) order
 * (the reference's order is that of a std::unordered_map).  Column-major outputs like the rest of this header. */
typedef struct ipcgpu_tetmesh ipcgpu_tetmesh;
int ipcgpu_read_tet_mesh(const char* path, ipcgpu_tetmesh** mesh, int* nV, int* nT, int* nSF);
int ipcgpu_tet_mesh_get(const ipcgpu_tetmesh*, double* V_colmajor, int* T_colmajor, int* SF_colmajor);
void ipcgpu_tet_mesh_free(ipcgpu_tetmesh*);
/* IglUtils::saveTetMesh (src/Utils/IglUtils.cpp:300-361): MSH 4.1 ASCII + $Surface */
int ipcgpu_save_tet_mesh(const char* path, int nV, int nT, const double* V_colmajor, const int* T_colmajor);

/* ---- mesh = the Mesh<3> data contract ----------------------------------------------- */
/* Replaces Mesh::computeFeatures + computeMassMatrix + setLameParam
 * (src/Mesh.cpp:414-527, 246-266, 399-401, 660-671): restTriInv, triArea, lumped mass,
 * vNeighbor and the Lame parameters are derived here from the rest shape. */
int ipcgpu_set_mesh(ipcgpu_ctx*, int nV, int nT, const double* V_rest_colmajor,
    const int* F_colmajor, double youngs_modulus, double poisson_ratio, double density);
/* vertexDBCType (Mesh.hpp:131-144) */
int ipcgpu_set_dbc(ipcgpu_ctx*, int n, const int* vert_ids, int dbc_type);
int ipcgpu_clear_dbc(ipcgpu_ctx*);
/* one `componentMaterial` entry of Mesh::setLameParam (Mesh.cpp:661-671; `shapes ... material rho E nu` in the scene script):
 * nodes [nodeBegin, nodeEnd) get density rho, tets [tetBegin, tetEnd) get (YM, PR).  Call after ipcgpu_set_mesh. */
int ipcgpu_set_component_material(ipcgpu_ctx*, int nodeBegin, int nodeEnd, int tetBegin, int tetEnd, double rho, double YM, double PR);
/* Config `energy NH|FCR` (src/Config.cpp:23-24,107-111; selects NeoHookeanEnergy or FixedCoRotEnergy in main.cpp): 0 = NH,
 * 1 = FCR (src/Energy/Physics_Elasticity/FixedCoRotEnergy.cpp:62-153).  FCR has no element-inversion safeguard
 * (Energy<dim>(false)): inversion checks and the injective step filter are skipped as in Optimizer.cpp:252,517,545,2710.
 * 2 = SNH, the stable neo-Hookean energy (Smith, de Goes, Kim, "Stable Neo-Hookean Flesh Simulation", ACM TOG 2018; no counterpart in the reference).  The
 * element's Lame parameters (ipcgpu_get_features / ipcgpu_set_mesh_features) keep their meaning; the kernels apply the paper's 3-D reparametrisation where
 * they load them:  mu = 4/3 mu_L, lam = lam_L + 5/6 mu_L, alpha = 1 + 3 mu / (4 lam), and with I_C = |F|_F^2, J = det F, c = I_C / (I_C + 1), k = lam (J - alpha)
 *   psi = mu/2 (I_C - 3) + lam/2 (J - alpha)^2 - mu/2 log(I_C + 1) - psi0,  psi0 = 9 mu^2 / (32 lam) - mu/2 log 4  (psi(I) = 0),   P = mu c F + k cof F.
 * Finite and C2 for every F (inverted, flat, F = 0), rest-stable, and d2psi/dF2 at F = I is Hooke's tensor of (mu_L, lam_L).  Energy and gradient need no SVD;
 * the projected Hessian uses the sigma-space blocks A_ii = mu c + 2 mu s_i^2 / (I_C+1)^2 + lam n_i^2, A_ij = 2 mu s_i s_j / (I_C+1)^2 + lam n_i n_j + k s_m
 * (n_i the product of the other two singular values, m the third index) and B_ij = [[mu c, -k s_m], [-k s_m, mu c]], eigenvalues mu c -+ k s_m clamped at 0.
 * Like FCR, SNH has no element-inversion safeguard: ipcgpu_filter_step_size returns the step untouched and the stepper neither launches nor consults an
 * inversion check.  ipcgpu_check_inversion under SNH is the plain mesh query (det < 0 of some element).  Any other value: IPCGPU_ERR_ARG. */
int ipcgpu_set_energy_type(ipcgpu_ctx*, int energy_type);
/* Mesh::V (current positions) */
int ipcgpu_set_positions(ipcgpu_ctx*, const double* V_colmajor);
int ipcgpu_get_positions(ipcgpu_ctx*, double* V_colmajor);
/* Optimizer::xTilta (Optimizer.cpp:1236-1257) */
int ipcgpu_set_xtilde(ipcgpu_ctx*, const double* xTilta_colmajor);
/* read back derived per-element / per-node data (any pointer may be NULL).  restTriInv is the CURRENT one: once ipcgpu_set_plasticity was called it is
 * downloaded from the device, where the plastic flow rewrites it. */
int ipcgpu_get_features(ipcgpu_ctx*, double* restTriInv_9nT, double* triArea_nT, double* mass_nV,
    double* mu_nT, double* lambda_nT);
/* nV = nT = 0 until ipcgpu_set_mesh was called */
int ipcgpu_get_mesh_dims(ipcgpu_ctx*, int* nV, int* nT);
/* Hand over the arrays Mesh<3> already holds instead of having them re-derived from (V_rest, F, E, nu, rho): restTriInv
   (Mesh.hpp:163, one 3x3 per tet, column-major inside the 9), triArea (:151), the diagonal of massMatrix (:148, lumped),
   u / lambda (:150, per tet).  Any pointer may be NULL (that array keeps what ipcgpu_set_mesh computed).  Call after
   ipcgpu_set_mesh; lets per-element state the reference modified after construction (component materials, rescaled
   masses) reach the device unchanged.  A restTriInv argument resets the plastic history (ipcgpu_set_plasticity): it becomes
   both the current rest shape and the one ipcgpu_plastic_reset restores, and the accumulated plastic strain is zero again. */
int ipcgpu_set_mesh_features(ipcgpu_ctx*, const double* restTriInv_9nT, const double* triArea_nT, const double* mass_nV,
    const double* mu_nT, const double* lambda_nT);
/* Mesh::checkInversion (Mesh.cpp:715-764): *ok = 1 when no element has det < 0 */
int ipcgpu_check_inversion(ipcgpu_ctx*, int* ok);

/* ---- Energy<3> plugin (NeoHookeanEnergy) -------------------------------------------- */
/* Energy::computeEnergyVal (Energy.hpp:42, Energy.cpp:195-242): E = coef * sum_t vol_t psi(F_t) */
int ipcgpu_elastic_energy(ipcgpu_ctx*, double coef, double* energy);
/* Energy::getEnergyValPerElemBySVD (Energy.hpp:66) */
int ipcgpu_elastic_energy_per_elem(ipcgpu_ctx*, double* perElem_nT);
/* Stress fields of the positions the context holds (no counterpart in the reference, which writes positions and energies only).  Per element the
 * Cauchy stress sigma = P F^T / J of the configured energy (ipcgpu_set_energy_type), P the first Piola-Kirchhoff stress the gradient is built from,
 * F the deformation gradient, J = det F, mu / lam the element's Lame parameters:
 *   NH   sigma = (mu (F F^T - I) + lam ln J I) / J
 *   FCR  sigma = 2 mu (F - R) F^T / J + lam (J - 1) I,  R = U V^T the rotation of the SVD F = U diag(s) V^T (only s_2 may be negative)
 *   SNH  sigma = mu c F F^T / J + k I  with the reparametrised mu, lam and c, k of ipcgpu_set_energy_type; finite for J < 0 (nInvalid = 0) like FCR, inf or
 *        NaN, uncounted, at J = 0 exactly
 * perElem: column-major nT x 8 -- sxx, syy, szz, sxy, syz, sxz (the symmetric-tensor order of VTK), the von Mises stress sqrt(3/2 dev sigma : dev
 * sigma), J.  An element without stiffness (mu = lam = 0) gets zeros and its J.  An NH element with J <= 0 has no stress: NaN in all eight entries,
 * and *nInvalid counts such elements; FCR is finite for inverted elements (nInvalid = 0) as long as J != 0 -- at J = 0 exactly P F^T / J is inf or
 * NaN, uncounted.
 * perNode: column-major nV x 8 -- the mean of the tensors of the node's elements weighted by their rest volumes (summed in ascending element
 * index), the von Mises stress OF THAT MEAN TENSOR (not the mean of the elements' von Mises stresses), the sum of those rest volumes (a sum that is exactly zero has no mean: NaN).  A node without
 * an element (surface-only and codimensional nodes) gets zeros; a NaN element makes the seven stress entries of its four nodes NaN (the volume sum stays).
 * Any pointer may be null; the nodal pass is skipped when perNode is null.  Valid after ipcgpu_set_mesh (positions: ipcgpu_set_positions) and at
 * any point between time steps after ipcgpu_opt_init (before a mesh is set: IPCGPU_ERR_STATE); changes no state.  fp64, a fixed summation order, no
 * floating-point atomics: the same state gives the same bits.  On a sharded context (ipcgpu_ctx_set_shard, world > 1): IPCGPU_ERR_UNSUPPORTED.
 * The stress is the ISOTROPIC part alone: the fibre term of ipcgpu_set_fibers is not in it (ipcgpu_fiber_state gives the fibre tension per element). */
int ipcgpu_elastic_stress(ipcgpu_ctx*, double* perElem_nTx8, double* perNode_nVx8, int* n_invalid);
/* Energy::computeGradient (Energy.hpp:47, Energy.cpp:245-289) */
int ipcgpu_elastic_gradient(ipcgpu_ctx*, double coef, int projectDBC, double* grad_3nV);
/* Energy::computeHessian (Energy.hpp:53, Energy.cpp:292-331) into the context's CSR values:
 * a += elastic Hessian (projectSPD, vInd sign convention of Energy.cpp:402-407) */
int ipcgpu_elastic_hessian_add(ipcgpu_ctx*, double coef, int projectDBC);
/* Energy::filterStepSize (Energy.hpp:129, Energy.cpp:565-581), slackness 0.2, tol 1e-6 */
int ipcgpu_filter_step_size(ipcgpu_ctx*, const double* searchDir_3nV, double* stepSize_inout);

/* ---- LinSysSolver plugin ------------------------------------------------------------ */
/* LinSysSolver::set_pattern(vNeighbor, fixedVert) (LinSysSolver.hpp:46-150).  extra_pairs adds
 * contact connectivity on top of the mesh's vNeighbor (augmentConnectivity,
 * SelfCollisionHandler.cpp:330-415); pass n_extra = 0 for the mesh pattern. */
int ipcgpu_linsys_set_pattern(ipcgpu_ctx*, int n_extra, const int* extra_pairs_2n);
/* LinSysSolver::set_pattern on a caller-provided 0-based symmetric-upper CSR (get_ia/get_ja) */
int ipcgpu_linsys_set_pattern_csr(ipcgpu_ctx*, int n_rows, const int* ia, const int* ja);
int ipcgpu_linsys_get_dims(ipcgpu_ctx*, int* n_rows, int* nnz); /* getNumRows / getNumNonzeros */
int ipcgpu_linsys_get_pattern(ipcgpu_ctx*, int* ia, int* ja); /* get_ia / get_ja */
int ipcgpu_linsys_set_zero(ipcgpu_ctx*); /* setZero, :348 */
int ipcgpu_linsys_get_values(ipcgpu_ctx*, double* a); /* get_a, :465 */
int ipcgpu_linsys_set_values(ipcgpu_ctx*, const double* a);
/* Batched form of the per-entry calls below for an adapter that keeps LinSysSolver's host-side addCoeff / setCoeff calls
   (LinSysSolver.hpp:331-348, 402-410) but owns the values in HBM: for every entry k of the CSR
   a[k] = (isSet && isSet[k]) ? setVal[k] + delta[k] : a[k] + delta[k].  isSet / setVal may be NULL (pure accumulate). */
int ipcgpu_linsys_apply_host_updates(ipcgpu_ctx*, const double* delta_nnz, const unsigned char* isSet_nnz, const double* setVal_nnz);
int ipcgpu_linsys_add_coeff(ipcgpu_ctx*, int row, int col, double v); /* addCoeff :402 (row>col ignored) */
int ipcgpu_linsys_set_coeff(ipcgpu_ctx*, int row, int col, double v); /* setCoeff :331 */
int ipcgpu_linsys_multiply(ipcgpu_ctx*, const double* x, double* Ax); /* multiply :238 */
int ipcgpu_linsys_analyze_pattern(ipcgpu_ctx*); /* analyze_pattern, CHOLMODSolver.cpp:123-128 */
int ipcgpu_linsys_factorize(ipcgpu_ctx*); /* factorize, :130-137; returns IPCGPU_NOT_PD */
int ipcgpu_linsys_solve(ipcgpu_ctx*, const double* rhs, double* result); /* solve, :139-154 */
int ipcgpu_linsys_precondition_diag(ipcgpu_ctx*, const double* in, double* out); /* :411-420 */
/* TEST HOOK, not part of the solver interface the adapters use (its flags2 and the upload of result exist for tests/test_gpu_solve_boundary.py; it may change
 * or go with them).  factorize + solve in one go, as the time stepper calls them (IPCGPU_SOLVER_MULTIFRONTAL: the forward sweep runs beside the factorisation).  result is
 * uploaded first and read back afterwards, so an entry the solver does not write keeps the caller's value.  negate_rhs != 0: solves A x = -rhs.  wait == 0:
 * everything is enqueued before the pivot flag is looked at, as in the stepper's Newton iteration.  flags2 (may be null): { the pivot flag as published to
 * the host, the pivot flag read from device memory }, 0 = positive definite.  Returns IPCGPU_NOT_PD like ipcgpu_linsys_factorize. */
int ipcgpu_linsys_factorize_solve(ipcgpu_ctx*, const double* rhs, double* result, int negate_rhs, int wait, int* flags2);
/* IPCGPU_SOLVER_PCG: preconditioned conjugate gradients from x = 0, the reference's iterative choice (`linearSolver AMGCL`: CG to a relative
 * residual, AMGCLSolver.cpp:24-25, 44, 201, 225-232; its smoothed-aggregation hierarchy is not rebuilt: IPCGPU_PRECOND_TWO_LEVEL is a two-level
 * method with a coarse space of its own).  Defaults when set_iterative is never
 * called: rel_tol 1e-5, max_iter 1000 (solver.tol / solver.maxiter, :24-25), block Jacobi, max_factor_age 1 (the best of 1, 2, 4, 8, 16
 * in a Newton run of the headline workload, profiles/pcg_bench.json).  The LinSysSolver calls then mean:
 *   analyze_pattern  BLOCK_JACOBI: no symbolic analysis at all, only the index of the lower triangle the product needs (AMGCLSolver.hpp: the
 *                    base class's no-op).  LAGGED_CHOLESKY: the multifrontal solver's analysis and set-up, as for IPCGPU_SOLVER_MULTIFRONTAL.
 *   factorize        (AMGCLSolver.cpp:173-191 rebuilds the preconditioner and returns true.)  BLOCK_JACOBI: inverts the 3x3 diagonal node
 *                    blocks (entries the pattern does not hold count as zero); IPCGPU_NOT_PD when one is not positive definite.
 *                    LAGGED_CHOLESKY: factorises when there is no factor for the current analysis, when the kept factor would be serving its
 *                    max_factor_age-th factorize() call (1 = always), or when the previous solve did not converge; otherwise keeps the
 *                    factor and counts its age.  IPCGPU_NOT_PD as for the multifrontal solver.
 *   solve            (AMGCLSolver.cpp:193-243.)  IPCGPU_NOT_PD when a search direction has p.Ap <= 0: the caller takes the diagonal fallback as
 *                    after a failed factorize (Optimizer.cpp:2331-2348).  Not converged after max_iter with a factor of age > 0: the current
 *                    values are factorised once and the solve runs again.  Still not converged: IPCGPU_OK with converged = 0 in the
 *                    statistics, as the reference goes on with what AMGCL returned (:230-241).
 * IPCGPU_PRECOND_TWO_LEVEL: z = D^-1 r + P Ac^-1 P^T r, block Jacobi plus an exact solve on a coarse space of six rigid-body modes per aggregate of
 * nodes (additive, so symmetric positive definite whenever A is; max_factor_age is ignored).  Node i of aggregate I contributes the 3x6 block
 * [ I | S(x_i - c_I) ] to P, S(d) w = d x w, c_I the centroid of the aggregate's free nodes; nodes with a Dirichlet type (ipcgpu_set_dbc) contribute
 * nothing; an aggregate with fewer than 4 free nodes gets translations only and an identity in its rotation block of Ac = P^T A P.
 *   analyze_pattern  aggregates the node graph of the pattern (greedy, in index order: deterministic) and analyses the coarse pattern with the
 *                    multifrontal solver; the fine matrix gets no symbolic analysis.  Needs a node pattern on the context's mesh
 *                    (ipcgpu_linsys_set_pattern): IPCGPU_ERR_UNSUPPORTED on an ipcgpu_linsys_set_pattern_csr pattern.
 *   factorize        inverts the diagonal blocks (IPCGPU_NOT_PD as for BLOCK_JACOBI), then builds P from the positions and Dirichlet types the
 *                    context holds at this call, assembles Ac on the device and factorises it.  An Ac that is not positive definite although every
 *                    diagonal block is leaves this matrix to block Jacobi alone: IPCGPU_OK, counted in ipcgpu_linsys_coarse_stats.
 *   solve            as for BLOCK_JACOBI; the coarse solver's sweeps run once per iteration.
 * Together with ipcgpu_linsys_set_shard(world > 1): IPCGPU_ERR_UNSUPPORTED.
 * ipcgpu_linsys_iter_stats, of the last solve: out6 = { iterations, |b - A x|_2 / |b|_2 at exit recomputed with one extra product, converged 0/1,
 * numeric factorisations this context's iterative solver has done so far, age of the factor the solve used (in factorize() calls), host
 * synchronisations the solve made }.
 * ipcgpu_linsys_multiply_sym: the solver's product (LinSysSolver.hpp:238-253) -- the lower triangle read from the upper storage through a
 * per-pattern index, no atomics, the same bits on every run; available with every solver type. */
int ipcgpu_linsys_set_iterative(ipcgpu_ctx*, double rel_tol, int max_iter, int precond, int max_factor_age);
int ipcgpu_linsys_iter_stats(ipcgpu_ctx*, double* out6);
/* The coarse level of IPCGPU_PRECOND_TWO_LEVEL.  coarse_stats: out5 = { aggregates, coarse rows (6 per aggregate), entries of the coarse upper CSR,
 * coarse factorisations this context has done so far, factorize() calls that fell back to block Jacobi alone }; the first three are 0 without a coarse
 * level.  coarse_dims: the same three sizes (0 without a coarse level).  coarse_get, after analyze_pattern: agg_of_node[n_nodes], the coarse
 * symmetric-upper CSR coarse_ia[rows + 1] / coarse_ja[nnz] (aggregate I owns rows 6 I .. 6 I + 2, translations, and 6 I + 3 .. 6 I + 5, rotations) and,
 * after factorize, its values coarse_a[nnz] as assembled on the device; any pointer may be NULL. */
int ipcgpu_linsys_coarse_stats(ipcgpu_ctx*, double* out5);
int ipcgpu_linsys_coarse_dims(ipcgpu_ctx*, int* n_aggregates, int* n_rows, int* nnz);
int ipcgpu_linsys_coarse_get(ipcgpu_ctx*, int* agg_of_node, int* coarse_ia, int* coarse_ja, double* coarse_a);
int ipcgpu_linsys_multiply_sym(ipcgpu_ctx*, const double* x, double* Ax);
/* Multi-GPU direct solver (one process per GPU): the assembly tree is cut below its top separators; rank r factorises and solves
   the subtrees it owns; a front above the cut is executed by ONE rank (the one that holds its most expensive child), and the update
   matrices / vectors of children on other ranks and the solution entries of ancestors travel point to point through the exchange hook
   (ipcgpu_opt_set_exchange[_stream] below: set it first, together with an all-reduce hook for the pivot flag and the solution vector).
   A rank needs the matrix values of the fronts it executes: replicated assembly, or ipcgpu_ctx_set_shard (owner-computes rows, see
   ipcgpu_opt_comm_stats below).  Takes effect at the next analyze_pattern.  ipcgpu_linsys_shard_stats (after analyze_pattern):
   out2[0] = world size, out2[1] = the share of the factorisation flops that lies above the cut (executed once each, on the chain of the cut's levels). */
int ipcgpu_linsys_set_shard(ipcgpu_ctx*, int rank, int world_size);
int ipcgpu_linsys_shard_stats(ipcgpu_ctx*, double* out2);
/* out4 = bytes THIS rank sent, bytes it received point to point through the solver's exchange hook so far, number of collective / group calls, and the
 * milliseconds this rank's stream spent inside those groups (HIP events around each: a rank that executes nothing at a level of the cut waits in its receive) */
int ipcgpu_linsys_exchange_stats(ipcgpu_ctx*, double* out4);
/* inputs of the strong-scaling model that bench.py prints beside its measured N-GPU value, after analyze_pattern: out5 = { dependent
 * 32-column pivot steps on the critical path of the assembly tree (per level the widest front's steps, summed), the same over the fronts ABOVE the cut of
 * ipcgpu_linsys_set_shard only, the largest rank's share of the flops below the cut (1 / world when balanced), levels, levels holding a front above the cut }.
 * No counterpart in the reference: CHOLMOD (CHOLMODSolver.cpp:118-154) is single-process. */
int ipcgpu_linsys_critical_path(ipcgpu_ctx*, double* out5);
/* Owner-computes sharding (round 4; SURVEY.md 8e, the north star's "RCCL all-reduce of the shared-node gradient / Hessian rows"): a context that has BOTH
   ipcgpu_ctx_set_shard and ipcgpu_linsys_set_shard (same world) assembles, per rank, exactly the CSR rows its fronts read -- the rows of the nodes its
   subtrees eliminate plus the separator rows above the cut, which every rank repeats (elements and contact stencils on a cut are evaluated by both sides) --
   so NO matrix value crosses ranks: the nodal gradient (one all-reduce, every node contributed by one rank), scalars, and the solver's update matrices /
   vectors / solution do.  ipcgpu_opt_comm_stats: out6 = bytes and calls all-reduced by the time stepper, by the solver, then the number of nodes whose
   rows this rank assembles and the number of nodes; ipcgpu_opt_complete_matrix: the rare consumer of the WHOLE matrix (ipcgpu_linsys_get_a / multiply on
   such a context) sums the rows over the ranks first.  IPCGPU_NO_OWNER_COMPUTES=1 keeps the older all-reduce of the values. */
int ipcgpu_opt_comm_stats(ipcgpu_ctx*, double* out6);
int ipcgpu_opt_complete_matrix(ipcgpu_ctx*);
/* diagnosis / tests (multifrontal solver, after analyze_pattern): for every entry k of the CSR pattern (ipcgpu_linsys_get_pattern order) the offset of its slot in
 * the front buffer, as the device kernel of the set-up computed it -- the same numbers mf_entry_destinations (ipc_amd/csrc/mf_symbolic.cpp) computes on the host */
int ipcgpu_linsys_entry_destinations(ipcgpu_ctx*, long long* dst_nnz);
/* The two parameters of the multifrontal factorisation a caller may set (every other one is fixed; their sweeps are under profiles/): levels of the assembly
 * tree whose 32-column step launches move at least bulk_min_mb MB of own columns factor them in outer blocks of bulk_block columns (two-level blocking;
 * defaults 48 MB / 256, reached by meshes beyond ~200 K nodes).  Takes effect at the next ipcgpu_linsys_analyze_pattern.  No counterpart in the reference
 * (CHOLMOD's supernodal blocking is internal, CHOLMODSolver.cpp:118-131); exists so that tests can force the path at test sizes. */
int ipcgpu_linsys_set_tuning(ipcgpu_ctx*, double bulk_min_mb, int bulk_block);
/* factor statistics: nnz(L), factorisation flops, number of supernodes / levels */
int ipcgpu_linsys_stats(ipcgpu_ctx*, double* stats4);

/* ---- Optimizer<3> building blocks --------------------------------------------------- */
/* setZero + elastic Hessian + mass / DBC diagonal: computePrecondMtr without contact
 * (Optimizer.cpp:3549-3668).  Fused with the gradient when grad_3nV != NULL
 * (computeGradient, Optimizer.cpp:3409-3450: elasticity + m (x - xTilta)). */
int ipcgpu_assemble_newton(ipcgpu_ctx*, double dtSq, int projectDBC, double* grad_3nV /*nullable*/);
/* computeEnergyVal (Optimizer.cpp:3199-3239): dtSq * elastic + 1/2 m |x - xTilta|^2 */
int ipcgpu_incremental_potential(ipcgpu_ctx*, double dtSq, double* energy);
/* computeGradient alone */
int ipcgpu_gradient(ipcgpu_ctx*, double dtSq, int projectDBC, double* grad_3nV);

/* ---- SelfCollisionHandler<3> (barrier contact) ------------------------------------- */
/* Mesh::SF (column-major nSF x 3 surface triangles, outward).  SVI and SFEdges are derived exactly as
 * Mesh::computeFeatures / computeBoundaryVert do (src/Mesh.cpp:495-515, 890-930), so edge and vertex indices
 * agree with the reference's. */
int ipcgpu_set_surface(ipcgpu_ctx*, int nSF, const int* SF_colmajor);
/* The same with the codimensional parts of Mesh<3> (`.seg` / `.pt` shapes, main.cpp:957-1005): CE = Mesh::CE, nCE node pairs.  The
 * segments enter vNeighbor and -- behind the triangles' edges, in the order given -- SFEdges, their ends SVI (Mesh.cpp:490-493, 513-515,
 * 912-915); a node that has no neighbour at all (no tetrahedron, triangle or segment: a `.pt` point) is a surface vertex as well
 * (:916-920) and is tested against every tetrahedron by the intersection check (SelfCollisionHandler.cpp:3301-3338).  Their masses:
 * ipcgpu_set_codim_nodes (segments: density * l^3 pi / 12 per end, Mesh.cpp:279-295; points: the mean nodal mass, :405-411). */
int ipcgpu_set_surface_codim(ipcgpu_ctx*, int nSF, const int* SF_colmajor, int nCE, const int* CE_pairs);
/* A build of the reference with USE_PREDICATES (CMakeLists.txt:137-140; not what the shipped CMake configures) decides the plane-side tests
 * of IglUtils::segTriIntersect (IglUtils.hpp:222-233) and IglUtils::pointInsideTetrahedron (:280-294) with the exact orient3d of
 * igl::predicates instead of floating-point products.  on != 0: the intersection checks do the same (orient3d_exact.h: Shewchuk's predicate
 * restated -- floating-point filter, exact expansion arithmetic behind it).  Default off = the default build. */
int ipcgpu_set_exact_predicates(ipcgpu_ctx*, int on);
int ipcgpu_get_surface(ipcgpu_ctx*, int* counts3 /*nSVI,nSF,nSFEdges*/, int* SVI /*nullable*/, int* SFEdges_2n /*nullable*/);
/* Kinematic mesh obstacles (MeshCO, src/CollisionObject/MeshCO.cpp:37-80; `meshCO` script keyword, Config.cpp:448-474): the
   obstacle rides along as a surface-only component of the mesh handed to ipcgpu_set_mesh -- extra nodes that belong to no
   tetrahedron (no mass, Dirichlet: ipcgpu_set_dbc), its triangles in the surface of ipcgpu_set_surface.  This call marks those
   nodes.  obstacle_only != 0: the contact sets, CCD and intersection checks keep only primitive pairs that involve an obstacle
   (a scene with `meshCO` but `selfCollisionOff`: Optimizer.cpp:2448-2470 asks only the collision objects).  Bounding box and
   mean nodal mass (dHat, kappa) are taken over element nodes, so the obstacle does not change them.  Call after set_surface. */
int ipcgpu_set_obstacle_nodes(ipcgpu_ctx*, int n, const int* vert_ids, int obstacle_only);
/* Contact groups: which bodies collide at all, and a friction factor per pair of groups (a project extension; the reference has neither).
 * Every component of ipcgpu_opt_set_components (default: one, the whole mesh) gets a group g in [0, nGroups), nGroups <= 16.
 *   collide[g * nGroups + h]    symmetric, 0 / 1: do primitives of groups g and h form contact pairs?
 *   fricScale[g * nGroups + h]  symmetric, finite, >= 0 (null: all 1): factor on the lagged normal force of a friction stencil between g and h
 * The group of a surface primitive (vertex, edge, triangle) is the group of its FIRST node -- the convention of the contact report; a primitive never
 * spans components.  A primitive pair with collide == 0 does not exist for contact: it is absent from the active set, the mollified set (paraEEMMCVIDSet
 * and paraEEeIeJSet) and the CCD candidate list that ipcgpu_contact_build and the time stepper form, it is not swept by ipcgpu_ccd_full,
 * ipcgpu_ccd_full_reference (vertex-vertex, vertex-edge, vertex-triangle and edge-edge pairs) or -- through the candidate list -- ipcgpu_ccd_partial, and
 * it is not tested by ipcgpu_is_intersected (edge against triangle; a codimensional point against a tetrahedron by the group of the tetrahedron's
 * first node).  collide[g][g] == 0 also removes the pairs INSIDE every component of group g.  The filter adds to the existing ones (incident
 * primitives, all-Dirichlet pairs, obstacle_only of ipcgpu_set_obstacle_nodes).  Sets handed in with ipcgpu_contact_set / ipcgpu_halfspace_set are
 * taken as they are: the filter applies to what the library builds.
 * Friction: the lagged multiplier of a stencil between groups ga and gb is multiplied by fricScale[ga][gb], on top of the factors of
 * ipcgpu_opt_set_friction_scales, so the effective coefficient is selfFric x scale: pass the LARGEST coefficient to ipcgpu_opt_set_friction and the
 * ratios here.  A scale of 0 leaves the stencil in the lagged set with a zero multiplier (it adds exact zeros): neither the number of lagged stencils
 * nor the matrix pattern depends on the scales.
 * Half-spaces take no part: a plane collides with every group and keeps its own coefficient (ipcgpu_opt_set_half_space_friction).
 * nComp must equal the number of components (else IPCGPU_ERR_ARG, as for a group outside [0, nGroups), nGroups outside [1, 16], an asymmetric matrix,
 * a collide entry other than 0 / 1, a negative or non-finite scale).  nComp == 0 goes back to the default, which is also the state after
 * ipcgpu_set_mesh and after ipcgpu_opt_set_components: every node in group 0, group 0 collides with itself, all scales 1.  Before ipcgpu_set_mesh:
 * IPCGPU_ERR_STATE.  Sharded context: IPCGPU_ERR_UNSUPPORTED.
 * ipcgpu_get_contact_groups: the number of groups and, per node, the word the contact kernels read: bits 4-7 the node's group, bits 16-31 the
 * group's row of collide (bit 16 + h), other bits 0; 0xFFFF0000 everywhere in the default state.  Either pointer may be null. */
int ipcgpu_set_contact_groups(ipcgpu_ctx*, int nComp, const int* group_nComp, int nGroups, const unsigned char* collide_nGroups2,
    const double* fricScale_nGroups2 /*nullable: all 1*/);
int ipcgpu_get_contact_groups(ipcgpu_ctx*, int* nGroups, int* nodeWord_nV /*nullable*/);
/* Surface-only ("codimensional") components of the simulated mesh: nodes of no tetrahedron that nevertheless belong to Mesh<3> --
 * the triangle meshes listed under `shapes` (componentCoDim 2; src/main.cpp, src/Mesh.cpp:310-345).  Unlike the nodes of a MeshCO
 * (ipcgpu_set_obstacle_nodes), which the reference keeps outside the mesh, they carry lumped masses: density x a third of the areas
 * of the adjacent triangles.  Like a MeshCO they stay OUT of the bounding box behind dHat / eps_v / the Newton tolerance and out of
 * the mean nodal mass behind kappa: the Optimizer sizes those with matSpaceBBoxSize2(dim) / avgNodeMass(dim), i.e. over the
 * tetrahedral components only (Mesh.cpp:576-637).  The scripts
 * fix or move them as Dirichlet nodes (`script DCOFix`: ipcgpu_set_dbc(ids, NONZERO)).  Call after ipcgpu_set_mesh, before
 * ipcgpu_opt_init / ipcgpu_opt_enable_self_collision. */
int ipcgpu_set_codim_nodes(ipcgpu_ctx*, int n, const int* node_ids, const double* node_mass);
/* Elastic shells (no counterpart in the reference): membrane and bending energy on triangle components.  Per triangle with rest positions X, positions
 * x, thickness h, Lame parameters from (E, nu) and rest area A:
 *   membrane  St. Venant-Kirchhoff, plane stress: Dm = [X1 - X0, X2 - X0] in the rest plane, F = [x1 - x0, x2 - x0] Dm^-1, G = (F^T F - I) / 2,
 *             psi = mu |G|_F^2 + lambda_ps tr(G)^2 / 2, mu = E / (2 (1 + nu)), lambda_ps = E nu / (1 - nu^2); energy h A psi; exact gradient; the 9 x 9
 *             Hessian projected to PSD per triangle.  A polynomial, finite everywhere: no inversion check, no step filter (as for FCR and SNH).
 *   bending   one hinge per edge shared by two triangles, nodes (x0, x1) on the edge and (x2, x3) opposite: bendScale k_b w_e (theta - thetaBar)^2 with
 *             theta the signed dihedral angle (atan2 of the two normals about the edge), thetaBar the same at rest (curved rest shapes are stress-free),
 *             w_e = 3 |eBar|^2 / (A1 + A2), k_b = E h^3 / (24 (1 - nu^2)) (mean of the two triangles).  Exact gradient; Gauss-Newton Hessian
 *             2 bendScale k_b w_e grad theta grad theta^T.  theta - thetaBar is NOT unwrapped: a hinge folded through +-pi is a self-intersection, which
 *             contact prevents.
 * ipcgpu_set_shell: tri_colmajor nTri x 3 node ids; thickness, E, nu, rho per triangle; bendScale >= 0.  After ipcgpu_set_mesh, before ipcgpu_opt_init
 * (else IPCGPU_ERR_STATE) and before ipcgpu_linsys_set_pattern: the node pairs of the shell (triangle edges and the opposite pair of every hinge) join
 * vNeighbor, so a pattern built afterwards holds every block the shell Hessian writes (a node pattern that exists already is rebuilt by this call from
 * the new vNeighbor, without extra pairs; a pattern given by ipcgpu_linsys_set_pattern_csr is the caller's business).  It sets the lumped masses of the shell nodes itself
 * (sum rho h A / 3) and marks them as element nodes: they enter the bounding box behind dHat, eps_v and the tolerance and the mean nodal mass behind
 * kappa -- a cloth-only scene sizes those from the cloth.  The surface triangles still come through ipcgpu_set_surface.  IPCGPU_ERR_ARG: a node id out of
 * range, a triangle that repeats a node, zero rest area, an edge shared by more than two triangles, two triangles that traverse a shared edge in the
 * same direction, a shell node that belongs to a tetrahedron, h, E, rho <= 0 or nu outside (-1, 1).  nTri == 0 removes the shell (no-op without one), a
 * second call replaces it: the nodes of the old shell get back the masses they had before it (those of ipcgpu_set_codim_nodes, or 0).
 * Sharded context (ipcgpu_ctx_set_shard, world > 1): IPCGPU_ERR_UNSUPPORTED.  ipcgpu_set_mesh drops the shell.
 * With a shell set its terms enter the stepper and the building blocks (ipcgpu_assemble_newton, ipcgpu_incremental_potential, ipcgpu_gradient) wherever
 * the tetrahedral elastic term does, with the same coefficient; ipcgpu_opt_system_report returns IPCGPU_ERR_UNSUPPORTED (its slices do not know the shell
 * energy); ipcgpu_elastic_stress keeps its zeros for nodes without tetrahedra.  Without a shell no shell kernel is ever launched.
 * ipcgpu_shell_get: counts2 = { nTri, nHinge }; hinge_4n hinge-major (x0, x1, x2, x3), ascending by (x0, x1) with x0 < x1, x2 opposite in the triangle
 * that traverses x0 -> x1; restAngle, hingeWeight (w_e) per hinge; rest areas per triangle; mass_nV the shell's lumped masses (0 elsewhere).  Any pointer
 * may be null.
 * ipcgpu_shell_energy: coef * (membrane + bending) at the current positions; it uses the optimizer's reduction buffers, hence after ipcgpu_opt_init (before:
 * IPCGPU_ERR_STATE).  The three entry points below need only the mesh and the shell (and the pattern, for the Hessian).  ipcgpu_shell_energy_per_elem: the
 * unscaled terms.  Without a shell all of them return IPCGPU_OK and do nothing: the energy is 0, the per-element arrays have length 0, grad and the
 * matrix stay as they are.
 * ipcgpu_shell_gradient_add: grad (host, 3 nV, xyz interleaved) += coef * gradient; entries of projected Dirichlet nodes are dropped (type ZERO always,
 * NONZERO with projectDBC).  ipcgpu_shell_hessian_add: the PSD blocks into the upper CSR values (after ipcgpu_linsys_set_pattern), rows and columns of
 * projected Dirichlet nodes dropped; a block the pattern lacks: IPCGPU_ERR_STATE.  fp64 atomics: sums agree to rounding, not to the bit. */
int ipcgpu_set_shell(ipcgpu_ctx*, int nTri, const int* tri_colmajor, const double* thickness_nTri, const double* YM_nTri, const double* PR_nTri,
    const double* rho_nTri, double bendScale);
int ipcgpu_shell_get(ipcgpu_ctx*, int* counts2, int* hinge_4n, double* restAngle, double* hingeWeight, double* area_nTri, double* mass_nV);
int ipcgpu_shell_energy(ipcgpu_ctx*, double coef, double* energy);
int ipcgpu_shell_energy_per_elem(ipcgpu_ctx*, double* perTri_nTri, double* perHinge_nHinge);
int ipcgpu_shell_gradient_add(ipcgpu_ctx*, double coef, int projectDBC, double* grad_3nV);
int ipcgpu_shell_hessian_add(ipcgpu_ctx*, double coef, int projectDBC);
/* Strain limiting of the shell (no counterpart in the reference): a log barrier on the principal stretches of the limited triangles.  With F the 3 x 2
 * deformation gradient of the membrane, sigma1 >= sigma2 its singular values (closed form), per triangle with limit s > 0, onset sHat and stiffness stiff:
 *   W = stiff h A E (b(sigma1) + b(sigma2)),  b = 0 for sigma <= sHat,  -y^2 ln(1 - y) with y = (sigma - sHat) / (s - sHat) below s,  +infinity from s on
 *   (never NaN).  b is C^2 at the onset, increasing and convex.  Exact gradient; the exact Hessian is PSD as it stands (closed-form eigenpairs, each clamped
 *   at 0 against round-off).  A triangle at or over its limit adds +infinity to the energy and nothing to gradient and matrix, which stay finite.
 * ipcgpu_shell_set_strain_limit: limit per triangle, 0 = unlimited; onset (null: 1) and stiff (null: 1) per triangle, read where limit > 0.  All limits zero,
 * or a null limit, removes the term.  After ipcgpu_set_shell (without a shell: IPCGPU_ERR_STATE), at any time: it changes no mass and adds no node pair --
 * the blocks are the membrane's, so the pattern stays.  ipcgpu_set_shell and ipcgpu_set_mesh drop the limit.  IPCGPU_ERR_ARG: 0 < limit <= onset,
 * onset < 1, stiff <= 0, a negative limit or a value that is not finite.
 * With a limit set the term is part of the shell energy everywhere: ipcgpu_shell_energy, ipcgpu_shell_gradient_add and ipcgpu_shell_hessian_add include it,
 * and through the stepper's shell terms so do ipcgpu_assemble_newton, ipcgpu_gradient, ipcgpu_incremental_potential and the stiffness damping.  The stepper
 * never accepts a state with a stretch at or over its limit: a trial energy of +infinity is backtracked by the line search; a scripted Dirichlet move is
 * shortened until the moved state is feasible (the augmented-Lagrangian solve takes the nodes the rest of the way); a time step that starts from a state
 * at or over a limit returns IPCGPU_ERR_STATE, the message naming the number of such triangles, and changes nothing.  Without a limit none of the limit
 * kernels is ever launched.
 * ipcgpu_shell_limit_energy / _energy_per_elem / _gradient_add / _hessian_add: the limit term alone, with the semantics of their ipcgpu_shell_* namesakes
 * (perTri has nTri entries, 0 for an unlimited triangle; coef > 0).  Without a limit they return IPCGPU_OK and add nothing.
 * ipcgpu_shell_stretch: sigma_2nTri (nullable) = sigma1, sigma2 of triangle t at 2 t, 2 t + 1; maxRatio (nullable) = the maximum of sigma1 / limit over the
 * limited triangles, exactly the maximum of those quotients of the returned values, 0 without a limited triangle.  Works with or without a limit; without
 * a shell it returns IPCGPU_OK, maxRatio 0. */
int ipcgpu_shell_set_strain_limit(ipcgpu_ctx*, const double* limit_nTri, const double* onset_nTri, const double* stiff_nTri);
int ipcgpu_shell_limit_energy(ipcgpu_ctx*, double coef, double* energy);
int ipcgpu_shell_limit_energy_per_elem(ipcgpu_ctx*, double* perTri_nTri);
int ipcgpu_shell_limit_gradient_add(ipcgpu_ctx*, double coef, int projectDBC, double* grad_3nV);
int ipcgpu_shell_limit_hessian_add(ipcgpu_ctx*, double coef, int projectDBC);
int ipcgpu_shell_stretch(ipcgpu_ctx*, double* sigma_2nTri, double* maxRatio);
/* Rubber membrane of the shell (no counterpart in the reference): the incompressible Mooney-Rivlin membrane on chosen triangles, in place of their StVK
 * membrane.  With F the 3 x 2 deformation gradient of the membrane, C = F^T F and the thickness stretch eliminated by incompressibility (1 / sqrt(det C)):
 *   I1 = tr C + 1 / det C,  I2 = tr C / det C + det C,  W = h A (c1 (I1 - 3) + c2 (I2 - 3)),  c1 = mu (1 - alpha) / 2,  c2 = mu alpha / 2,  mu = E / 3.
 *   alpha = 0 is the incompressible neo-Hookean membrane.  mu = E / 3 is the incompressible shear modulus: the Poisson ratio given to ipcgpu_set_shell is not
 *   read by this term (it still enters the bending constant of the hinges).  Exact gradient; the exact Hessian with its eigenvalues clamped at 0 per triangle.
 *   A degenerate rubber triangle (det C not positive, or not finite in floating point: collapsed to a line) adds +infinity to the energy and nothing to gradient
 *   and matrix, which stay finite; the 1 / det C term is a barrier, so a rubber triangle cannot collapse at finite energy.
 * ipcgpu_shell_set_membrane: model per triangle, 0 = StVK as without this call, 1 = rubber; alpha (null: 0) per triangle, read where model is 1.  All models
 *   zero, or a null model, removes the term.  After ipcgpu_set_shell (without a shell: IPCGPU_ERR_STATE), at any time between steps: it changes no mass and adds
 *   no node pair -- the blocks are the membrane's, so the pattern stays.  ipcgpu_set_shell and ipcgpu_set_mesh drop it.  IPCGPU_ERR_ARG: a model other than 0
 *   or 1, alpha outside [0, 1) or not finite.  A rubber triangle carries no StVK membrane energy; its hinges keep their bending term; a strain limit on the
 *   same triangle composes with it unchanged.
 * With rubber triangles the term is part of the shell energy everywhere: ipcgpu_shell_energy, ipcgpu_shell_gradient_add and ipcgpu_shell_hessian_add include
 *   it, and so do the time stepper and the stiffness damping.  The stepper never accepts a state with a degenerate rubber triangle: a trial energy of +infinity
 *   is backtracked by the line search; a scripted Dirichlet move that would flatten a rubber triangle is shortened; ipcgpu_opt_begin_timestep from a state
 *   with a degenerate rubber triangle returns IPCGPU_ERR_STATE, the message naming the number of such triangles, and changes nothing.  Without a rubber
 *   triangle none of the rubber kernels is launched and every result is bit-identical to a context that never made this call.
 * ipcgpu_shell_membrane_get: model and alpha per triangle as set (zeros without the term); either pointer may be null.
 * ipcgpu_shell_rubber_energy / _energy_per_elem / _gradient_add / _hessian_add: the rubber term alone, with the semantics of their ipcgpu_shell_* namesakes
 *   (perTri has nTri entries, 0 for a StVK triangle; coef > 0).  Without a rubber triangle they return IPCGPU_OK and add nothing.
 * ipcgpu_shell_thickness: the current thickness per triangle: h / (sigma1 sigma2) on a rubber triangle (sigma as ipcgpu_shell_stretch returns them), the rest
 *   thickness h on a StVK triangle, whose law does not thin. */
int ipcgpu_shell_set_membrane(ipcgpu_ctx*, const int* model_nTri, const double* alpha_nTri);
int ipcgpu_shell_membrane_get(ipcgpu_ctx*, int* model_nTri, double* alpha_nTri);
int ipcgpu_shell_rubber_energy(ipcgpu_ctx*, double coef, double* energy);
int ipcgpu_shell_rubber_energy_per_elem(ipcgpu_ctx*, double* perTri_nTri);
int ipcgpu_shell_rubber_gradient_add(ipcgpu_ctx*, double coef, int projectDBC, double* grad_3nV);
int ipcgpu_shell_rubber_hessian_add(ipcgpu_ctx*, double coef, int projectDBC);
int ipcgpu_shell_thickness(ipcgpu_ctx*, double* h_nTri);
/* Woven cloth of the shell (no counterpart in the reference): an orthotropic St. Venant-Kirchhoff membrane on chosen triangles, in place of their isotropic
 * one, and direction-dependent bending.  The model is stated in ipc_amd/csrc/shell_weave_kernels.h.  With F and G = (F^T F - I) / 2 the membrane's, a the unit
 * warp direction in the triangle's rest plane and b the weft at right angles to it:  Eww = a^T G a, Eff = b^T G b, Ewf = a^T G b,
 *   W = h A (C11 Eww^2 / 2 + C12 Eww Eff + C22 Eff^2 / 2 + 2 G12 Ewf^2),  C11 = E1 / (1 - nu12 nu21),  C22 = E2 / (1 - nu12 nu21),  C12 = nu12 E2 / (1 - nu12 nu21),
 *   nu21 = nu12 E2 / E1.  Exact gradient; the exact Hessian with its eigenvalues clamped at 0 per triangle.  A polynomial in F: finite at every finite state.
 *   With E1 = E2 = E, nu12 = nu, G12 = E / (2 (1 + nu)) it is the StVK membrane for every direction.  The E and nu given to ipcgpu_set_shell are not read by
 *   this term on a woven triangle (they still enter the bending constant k_b of its hinges).
 *   Bending: the stiffness of a hinge whose rest edge makes the angle phi with the warp is multiplied by the mean over its two triangles of
 *   bendWarp sin^2 phi + bendWeft cos^2 phi (a triangle that is not woven counts 1): an edge along the weft curves the warp yarns.
 * ipcgpu_shell_set_weave: woven per triangle, 0 = as without this call, 1 = woven; dir: 3 per triangle (x, y, z of triangle t at 3 t), a vector of rest space,
 *   projected into the triangle's rest plane and normalised; E1 (warp), E2 (weft), G12 (shear), nu12 (null: 0), bendWarp, bendWeft (null: 1) per triangle; all
 *   read where woven is 1.  All selectors zero, or a null woven, removes the term.  After ipcgpu_set_shell (without a shell: IPCGPU_ERR_STATE), at any time
 *   between steps, before or after ipcgpu_opt_init: it changes no mass and adds no node pair.  ipcgpu_set_shell and ipcgpu_set_mesh drop it.  IPCGPU_ERR_ARG,
 *   the message naming the triangle and nothing changed: a selector other than 0 or 1; a value that is not finite; E1, E2 or G12 <= 0; nu12^2 >= E1 / E2; a bend
 *   factor <= 0; a direction of zero length, or one normal to the triangle (its projection shorter than 1e-6 of its length).  A woven triangle can be neither
 *   rubber nor plastic (flow rewrites the rest metric, in which a and b would stop being orthonormal): IPCGPU_ERR_UNSUPPORTED naming the triangle from this call
 *   on a rubber or plastic triangle, from ipcgpu_shell_set_membrane with rubber on a woven triangle and from ipcgpu_shell_set_plasticity on a woven triangle.
 *   A strain limit on the same triangle composes unchanged; ipcgpu_shell_thickness returns the rest h there; ipcgpu_shell_get keeps returning the plan's values.
 * With woven triangles the term is part of the shell energy everywhere: ipcgpu_shell_energy, ipcgpu_shell_gradient_add and ipcgpu_shell_hessian_add include it,
 *   and so do the time stepper and the stiffness damping.  Without one none of its kernels is launched and every result is bit-identical to a context that
 *   never made this call.
 * ipcgpu_shell_weave_get: woven (nTri), a (nTri x 2, row-major: a_x, a_y in the rest frame whose first axis runs along X1 - X0), const4 (nTri x 4, row-major:
 *   C11, C12, C22, G12, without h A) -- zeros on a triangle that is not woven -- and the factor per hinge (1 without the term); any pointer may be null.
 * ipcgpu_shell_weave_energy / _energy_per_elem / _gradient_add / _hessian_add: the term alone, with the semantics of the ipcgpu_shell_rubber_* namesakes (any
 *   coef).  ipcgpu_shell_weave_state: column-major nTri x 6 -- Eww, Eff, the shear angle asin((F a) . (F b) / (|F a| |F b|)) and the current unit warp direction
 *   F a / |F a| (x, y, z); NaN where a length it divides by is 0, zeros on a triangle that is not woven.  Without a shell these return IPCGPU_OK and do nothing. */
int ipcgpu_shell_set_weave(ipcgpu_ctx*, const int* woven_nTri, const double* dir_3nTri, const double* E1_nTri, const double* E2_nTri, const double* G12_nTri,
                           const double* nu12_nTri, const double* bendWarp_nTri, const double* bendWeft_nTri);
int ipcgpu_shell_weave_get(ipcgpu_ctx*, int* woven_nTri, double* a_2nTri, double* const4_nTri, double* hingeFactor_nHinge);
int ipcgpu_shell_weave_energy(ipcgpu_ctx*, double coef, double* energy);
int ipcgpu_shell_weave_energy_per_elem(ipcgpu_ctx*, double* perTri_nTri);
int ipcgpu_shell_weave_gradient_add(ipcgpu_ctx*, double coef, int projectDBC, double* grad_3nV);
int ipcgpu_shell_weave_hessian_add(ipcgpu_ctx*, double coef, int projectDBC);
int ipcgpu_shell_weave_state(ipcgpu_ctx*, double* perTri_nTrix6);
/* ---- Plastic flow of the shell: permanent stretch, creases and dents.  No counterpart in the reference (it has no shell and no plasticity).  The model is
 * stated in ipc_amd/csrc/shell_plastic_kernels.h.  Every shell kernel reads the rest shape of a triangle from B = Dm^-1 (rows 0-3 of its constants) and of a
 * hinge from thetaBar, so at the end of every time step (after the BE / Newmark update, before the lagged damping matrix) two kernels rewrite those records:
 *   membrane, per triangle with a finite yield: C = F^T F = V diag(l1, l2) V^T, skipped and counted where l2 <= 0; e_i = ln(l_i) / 2, e3 = -nu / (1 - nu)
 *     (e1 + e2), n = |dev(e1, e2, e3)|; y = yield + harden alpha; where n > y: Delta = -expm1(-creep dt) (n - y) / (1 + harden), B <- B V diag(exp(-Delta e_i
 *     / n)) V^T, alpha += Delta.  h A mu, h A lambda_ps, masses and the strain-limit scale do not change (the thickness takes up det G).  For small strains
 *     the von Mises stress is sqrt(6) mu n, as for the tetrahedra.
 *   hinges, per hinge whose two triangles both have a finite bendYield (its parameters are the means of theirs): eps = g |theta - thetaBar|, g = h_m w_e /
 *     (2 |eBar|), skipped and counted where n1, n2 or e has zero length; where eps > y = bendYield + harden alphaB: Delta as above, thetaBar += sign(theta -
 *     thetaBar) Delta / g, alphaB += Delta.
 * ipcgpu_shell_set_plasticity (no counterpart in the reference): triangles [triBegin, triEnd) get (yield, bendYield, creep, harden); later calls overwrite.
 *   yield, bendYield >= 0 or +inf (+inf switches that flow off), creep > 0 or +inf (+inf: the rate-independent return), harden >= 0 and finite, nothing NaN,
 *   0 <= triBegin <= triEnd <= nTri: IPCGPU_ERR_ARG otherwise, and nothing is changed.  Without a shell: IPCGPU_ERR_STATE.  Touches neither the pattern nor
 *   the masses: allowed before or after ipcgpu_opt_init, between time steps.  The first call keeps copies B0 and thetaBar0 of the current records.  With
 *   nothing switched on the stepper launches nothing and every result is bit-identical to a context that never called this.  IPCGPU_ERR_UNSUPPORTED on a
 *   rubber triangle (ipcgpu_shell_set_membrane on a plastic triangle returns the same) and on a sharded context (ipcgpu_ctx_set_shard with world > 1 on a
 *   context with a plastic shell returns the same).  ipcgpu_set_shell and ipcgpu_set_mesh drop parameters and history.  ipcgpu_shell_set_membrane keeps a
 *   flowed B.  ipcgpu_shell_get keeps returning the plan's rest angle; the current thetaBar comes from the calls below.
 * ipcgpu_shell_plastic_get (no counterpart): yield, bendYield, creep, harden, alpha per triangle; triConst_nTrix6 column-major, the CURRENT six constants of
 *   every triangle as the kernels read them (B in columns 0-3, h A mu, h A lambda_ps); B0_nTrix4 column-major; hinge_nHingex4 column-major: mean bendYield
 *   (+inf: the hinge does not flow), mean creep, mean harden, g; alphaB, the CURRENT thetaBar and thetaBar0 per hinge.  Any pointer may be NULL.
 * ipcgpu_shell_plastic_update (no counterpart): ONE flow of both kinds at the held positions with the given dt, outside the stepper -- the kernels' test
 *   entry, like the *_hessian_add calls.  counts4 (nullable): triangles rewritten, triangles skipped, hinges rewritten, hinges skipped.
 * ipcgpu_shell_plastic_state (no counterpart): read-only.  perTri (nullable, column-major nTri x 4): n, the current y, alpha, the rest-area ratio det B0 /
 *   det B; n = NaN for a triangle the flow would skip, y = +inf where the membrane flow is off.  perHinge (nullable, column-major nHinge x 4): eps, the
 *   current y, alphaB, thetaBar - thetaBar0.  totals7 (nullable): counts4 of the last flow, max alpha, max alphaB, sum of h A alpha.  Deterministic: fixed
 *   summation order, no floating-point atomics.
 * ipcgpu_shell_plastic_set_state (no counterpart): B (nTri x 4 column-major), alpha, thetaBar, alphaB from the caller (any may be NULL); needs
 *   ipcgpu_shell_set_plasticity first.  ipcgpu_shell_plastic_reset (no counterpart): B = B0, thetaBar = thetaBar0, alpha = alphaB = 0.
 * ipcgpu_opt_save_status appends a section `shellplastic <nTri> 5 <nHinge> 2` (B and alpha per triangle, then thetaBar and alphaB per hinge) when something
 * is plastic -- the file is otherwise byte for byte what it was; ipcgpu_opt_load_status reads it (a file without it leaves the records untouched; a
 * truncated section is refused with a message that names it). */
int ipcgpu_shell_set_plasticity(ipcgpu_ctx*, int triBegin, int triEnd, double yield, double bendYield, double creep, double harden);
int ipcgpu_shell_plastic_get(ipcgpu_ctx*, double* yield_nTri, double* bendYield_nTri, double* creep_nTri, double* harden_nTri, double* alpha_nTri,
    double* triConst_nTrix6, double* B0_nTrix4, double* hinge_nHingex4, double* alphaB_nHinge, double* thetaBar_nHinge, double* thetaBar0_nHinge);
int ipcgpu_shell_plastic_update(ipcgpu_ctx*, double dt, int* counts4);
int ipcgpu_shell_plastic_state(ipcgpu_ctx*, double* perTri_nTrix4, double* perHinge_nHingex4, double* totals7);
int ipcgpu_shell_plastic_set_state(ipcgpu_ctx*, const double* B_nTrix4, const double* alpha_nTri, const double* thetaBar_nHinge, const double* alphaB_nHinge);
int ipcgpu_shell_plastic_reset(ipcgpu_ctx*);
/* Elastic rods (no counterpart in the reference): stretching and bending energy on segment components.
 *   stretching  per segment (a, b): rest length L, length l, radius r, Young's modulus E, A = pi r^2, k_s = E A / L, W_s = k_s (l - L)^2 / 2.  Exact gradient.
 *               With t = (x_b - x_a) / l the 3 x 3 block is B = k_s [t t^T + max(0, 1 - L / l) (I - t t^T)], the 6 x 6 Hessian [[B, -B], [-B, B]]: the clamp
 *               at 0 is the exact eigenvalue projection of the full Hessian (spectrum 2 k_s, 2 k_s (1 - L / l) twice, 0 three times).
 *   bending     per interior node b (exactly two incident segments (a, b), (b, c)): e0 = x_b - x_a, e1 = x_c - x_b, kb = 2 e0 x e1 / d,
 *               d = |e0||e1| + e0 . e1, W_b = bendScale k_b |kb|^2, k_b = E_m I / (L0 + L1), I = pi r_m^4 / 4 (means of the two segments): the bending term of
 *               discrete elastic rods without twist (|kb| = 2 tan(theta / 2)), with a STRAIGHT rest state.  Exact gradient 2 bendScale k_b J^T kb,
 *               J = d kb / d (x_a, x_b, x_c); Gauss-Newton Hessian 2 bendScale k_b J^T J (rank <= 3, PSD).  W_b grows without bound as the node folds flat
 *               (d -> 0), which keeps two adjacent segments -- they share a node and form no contact pair -- from folding onto each other; where d <= 0 in
 *               floating point the energy is +infinity, never NaN, and the line search backtracks.
 * Not modelled: twist and material frames; rest curvature (ipcgpu_rod_get returns the rest |kb| per interior node: a curved rest polyline will be pulled
 * straight; bendScale = 0 switches bending off); bending at junctions (a node with three or more segments carries stretching only); a thickness offset in
 * contact (the gap stays dHat around the centre line).
 * ipcgpu_set_rod: seg_colmajor nSeg x 2 node ids; radius, E, rho per segment; bendScale >= 0.  After ipcgpu_set_mesh, before ipcgpu_opt_init (else
 * IPCGPU_ERR_STATE) and before ipcgpu_linsys_set_pattern: the node pairs of the rod (segments and the outer pair (a, c) of every bending triple) join
 * vNeighbor (a node pattern that exists already is rebuilt by this call, without extra pairs).  It sets the lumped masses of the rod nodes itself (sum
 * rho pi r^2 L / 2) and marks them as element nodes, as ipcgpu_set_shell does for shell nodes.  Collision still needs the segments passed to
 * ipcgpu_set_surface (its CE list): this call gives them elasticity, not contact.  IPCGPU_ERR_ARG: a node id out of range, a segment with a == b, a repeated
 * segment (in either direction), zero rest length, a rod node that belongs to a tetrahedron or to a shell triangle, radius, E or rho <= 0 (and ipcgpu_set_shell
 * refuses a shell node that belongs to a rod segment).  nSeg == 0 removes
 * the rod (no-op without one), a second call replaces it: the nodes of the old rod get back the masses they had before it.  Sharded context:
 * IPCGPU_ERR_UNSUPPORTED.  ipcgpu_set_mesh drops the rod.
 * With a rod set its terms enter the stepper and the building blocks wherever the shell and the tetrahedral elastic terms do, with the same coefficient;
 * ipcgpu_opt_system_report returns IPCGPU_ERR_UNSUPPORTED; ipcgpu_elastic_stress keeps its zeros for rod nodes.  Without a rod no rod kernel is ever launched.
 * ipcgpu_rod_get: counts2 = { nSeg, nBend }; bend_3n triple-major (a, b, c), ascending by b; rest lengths and k_s per segment; k_b (without bendScale) and
 * the rest |kb| per triple; mass_nV the rod's lumped masses (0 elsewhere).  Any pointer may be null.
 * ipcgpu_rod_energy / _energy_per_elem / _gradient_add / _hessian_add: the semantics of their ipcgpu_shell_* namesakes (the energy after ipcgpu_opt_init;
 * per-element terms unscaled; projected Dirichlet entries dropped; a block the pattern lacks: IPCGPU_ERR_STATE; fp64 atomics).  Without a rod all of them
 * return IPCGPU_OK and do nothing. */
int ipcgpu_set_rod(ipcgpu_ctx*, int nSeg, const int* seg_colmajor, const double* radius_nSeg, const double* YM_nSeg, const double* rho_nSeg, double bendScale);
int ipcgpu_rod_get(ipcgpu_ctx*, int* counts2, int* bend_3n, double* restLen_nSeg, double* ks_nSeg, double* kb_nBend, double* restKb_nBend, double* mass_nV);
int ipcgpu_rod_energy(ipcgpu_ctx*, double coef, double* energy);
int ipcgpu_rod_energy_per_elem(ipcgpu_ctx*, double* perSeg_nSeg, double* perBend_nBend);
int ipcgpu_rod_gradient_add(ipcgpu_ctx*, double coef, int projectDBC, double* grad_3nV);
int ipcgpu_rod_hessian_add(ipcgpu_ctx*, double coef, int projectDBC);
/* Attachments (no counterpart in the reference): springs that tie a point A to a point B -- stitches (rest length 0) and tethers (rest length > 0).
 *   Each point is a fixed convex combination of one to three nodes (a node, a point on an edge, a point in a triangle), given as up to three (node, weight)
 *   pairs with weights >= 0 that sum to 1; an unused slot is node id -1 with weight 0.  The nodes may belong to any components, the same one included:
 *   tetrahedral, shell, rod, scripted or obstacle nodes.  A node that appears in both points is merged into one signed coefficient
 *   c_i = weight in A - weight in B (sum c_i = 0, up to 6 distinct nodes); nodes whose coefficient is zero are dropped.
 *   energy      per attachment, stiffness k > 0 (a force per length, the caller's: no material scales it) and rest length L >= 0:
 *               d = sum_i c_i x_i, l = |d|, W = k (l - L)^2 / 2.  Exact gradient grad_i = k (l - L) c_i t, t = d / l.  Hessian blocks H_ij = c_i c_j B,
 *               B = k [t t^T + max(0, 1 - L / l) (I - t t^T)]: the clamp at 0 is the exact eigenvalue projection of the full Hessian (c c^T) (x) B_full
 *               (spectrum |c|^2 times k, k (1 - L / l) twice).  L == 0: W = k |d|^2 / 2, grad_i = k c_i d, B = k I, without a square root or a
 *               division, well defined at d = 0.  L > 0 and l == 0: the energy k L^2 / 2, no force and no block.  Never NaN.
 *   Rows, columns and gradient entries of projected Dirichlet nodes are dropped: a point tied to a scripted collider follows it.
 *   Contact is NOT changed: attached bodies still form contact pairs, so a zero-length stitch between two different surfaces settles at a gap below dHat
 *   with the barrier active.  A caller who wants none of that masks the pair of bodies with ipcgpu_set_contact_groups or gives the attachment a rest length.
 * Not modelled: breaking or plastic stitches; damping of the spring beyond the stiffness-proportional damping every elastic term shares; any exemption
 * from contact.
 * ipcgpu_set_attachments: nodesA_3n / weightsA_3n / nodesB_3n / weightsB_3n attachment-major (slot s of attachment i at 3 i + s); k_n, L_n per attachment.
 * After ipcgpu_set_mesh, before ipcgpu_opt_init (else IPCGPU_ERR_STATE) and before ipcgpu_linsys_set_pattern: every node pair of an attachment joins
 * vNeighbor (a node pattern that exists already is rebuilt by this call, without extra pairs).  It changes no mass and marks no node.  IPCGPU_ERR_ARG: a node
 * id out of range, a point with no node, a weight that is negative or not finite (or != 0 in an unused slot), weights of a point that do not sum to 1 within
 * 1e-12, k <= 0, L < 0 or either not finite, an attachment whose two points are the same.  n == 0 removes the attachments (no-op without any), a second
 * call replaces them.  Sharded context: IPCGPU_ERR_UNSUPPORTED (both ways: ipcgpu_ctx_set_shard refuses a context with attachments).  ipcgpu_set_mesh
 * drops them.
 * With attachments set their term enters the stepper and the building blocks wherever the shell, rod and tetrahedral elastic terms do, with the same
 * coefficient; ipcgpu_opt_system_report returns IPCGPU_ERR_UNSUPPORTED (the energy belongs to no single component).  Without any no attachment kernel is
 * ever launched.
 * ipcgpu_attach_get: *count = n; counts_n the distinct nodes per attachment (2 to 6); nodes_6n / coefs_6n slot-major (slot s of attachment i at s n + i):
 * the merged ids and signed coefficients, the slots behind counts_n[i] repeat slot 0 with coefficient 0; k_n, L_n; restDist_n the distance |d| of the two
 * points at the rest positions (which stitches are pre-stretched).  Any pointer may be null.
 * ipcgpu_attach_energy / _energy_per_elem / _gradient_add / _hessian_add: the semantics of their ipcgpu_rod_* namesakes (the energy after ipcgpu_opt_init;
 * per-attachment terms unscaled; projected Dirichlet entries dropped; a block the pattern lacks: IPCGPU_ERR_STATE; fp64 atomics).
 * ipcgpu_attach_state: per attachment the current length l and the signed force k (l - L) (positive: in tension); either pointer may be null.
 * Without attachments all of them return IPCGPU_OK and do nothing. */
int ipcgpu_set_attachments(ipcgpu_ctx*, int n, const int* nodesA_3n, const double* weightsA_3n, const int* nodesB_3n, const double* weightsB_3n, const double* k_n,
    const double* L_n);
int ipcgpu_attach_get(ipcgpu_ctx*, int* count, int* counts_n, int* nodes_6n, double* coefs_6n, double* k_n, double* L_n, double* restDist_n);
int ipcgpu_attach_energy(ipcgpu_ctx*, double coef, double* energy);
int ipcgpu_attach_energy_per_elem(ipcgpu_ctx*, double* perAttach_n);
int ipcgpu_attach_gradient_add(ipcgpu_ctx*, double coef, int projectDBC, double* grad_3nV);
int ipcgpu_attach_hessian_add(ipcgpu_ctx*, double coef, int projectDBC);
int ipcgpu_attach_state(ipcgpu_ctx*, double* length_n, double* force_n);
/* Pressure chambers: a gas pressure inside closed surfaces, constant or following the ideal-gas law (a balloon, a cushion, a hollow body under outside pressure).  A project extension: the
 * reference has none.  A pressure load is a follower load -- its direction and size move with the surface --, which ipcgpu_opt_add_neumann (a constant
 * acceleration) cannot stand in for.
 *   A chamber is a closed, consistently oriented set of triangles (outward normals by the right-hand rule) over any nodes of the mesh: shell nodes, surface
 *   nodes of tetrahedral components, scripted nodes.  It may consist of several closed pieces.  Chamber c holds the constant gauge pressure p_c: positive
 *   pushes outward, negative is suction or an outside hydrostatic pressure.
 *   energy      with a reference point r_c that is constant during any one evaluation and y_i = x_i - r_c:  V_c = 1/6 sum_t y0 . (y1 x y2) over the
 *               chamber's triangles, W_c = -p_c V_c, per triangle W_t = -(p_c / 6) y0 . (y1 x y2).  Exact gradient dW_t/dx0 = -(p/6) y1 x y2,
 *               dW_t/dx1 = -(p/6) y2 x y0, dW_t/dx2 = -(p/6) y0 x y1.  The 9 x 9 Hessian of a triangle has zero diagonal blocks and H01 = (p/6) [y2]x,
 *               H02 = -(p/6) [y1]x, H12 = (p/6) [y0]x; it is indefinite and is projected to PSD per triangle (a Jacobi eigen-iteration on 9 x 9).
 *   r_c         For a closed surface V_c and its gradient do not depend on r_c in exact arithmetic; the per-triangle Hessian does (its entries grow with
 *               |y|), so a projection about the world origin would add a spurious stiffness proportional to the body's distance from the origin.  r_c is
 *               the mean of the centroids of the chamber's triangles: ipcgpu_set_chambers computes it at the rest positions, ipcgpu_opt_begin_timestep
 *               refreshes it on the device from the positions the step starts from, and it stays fixed through that step's Newton iterations and line
 *               searches (every energy comparison inside a step uses one r_c).  ipcgpu_set_positions does not move it.
 *   Rows, columns and gradient entries of projected Dirichlet nodes are dropped.  The term is no stiffness: it does not enter the lagged stiffness damping
 *   (ipcgpu_opt_set_damping), whose matrix is to the bit what it is without chambers.  Contact is NOT changed.
 * The gas law (ipcgpu_chamber_set_gas).  A chamber is either constant (above, the default) or GAS: an ideal gas with the ambient absolute pressure
 *   p_amb >= 0, the exponent gamma >= 1 (1 isothermal, 1.4 adiabatic air) and the fill volume V0 > 0 (default: the rest volume).  The chamber's pressure p_c
 *   then is the gauge pressure the gas has at V0, P0 = p_amb + p_c > 0, and ipcgpu_chamber_set_pressure between steps pumps gas in or out.  With V the
 *   enclosed volume about r_c:
 *     P(V) = P0 (V0 / V)^gamma,  gauge(V) = P(V) - p_amb
 *     W = -P0 V0 ln(V / V0) + p_amb (V - V0)  (gamma == 1),   W = P0 V0 / (gamma - 1) ((V0 / V)^(gamma - 1) - 1) + p_amb (V - V0)  (gamma > 1),
 *     W = +infinity for V <= 0 (the line search backs off)
 *     dW/dx = -gauge(V) gradV,   d2W/dx2 = -gauge(V) d2V/dx2 + beta gradV gradV^T,  beta = gamma P(V) / V > 0
 *   The first Hessian term is the constant chamber's per-triangle block with p = gauge(V) at the current positions, projected as above.  The second is PSD,
 *   rank one and dense; it never enters the matrix.  The stepper applies it as a rank-k correction around the factor (Woodbury; k gas chambers, k <= 8):
 *   y = A^-1 r, z_c = A^-1 u_c (u_c = gradV_c), C = diag(1 / (coef beta_c)) + U^T Z, C w = U^T y, d = y - Z w.  Where the factorisation reports a bad pivot
 *   the diagonal fallback runs as without it and ignores the term.  Exact solvers only: with a gas chamber IPCGPU_SOLVER_PCG is IPCGPU_ERR_UNSUPPORTED, both
 *   ways round.  Like the constant chamber the term stays out of the stiffness damping, the sparse part and the rank-one part both.
 *   V_c, gauge_c, beta_c and W_c come from a deterministic two-pass reduction on the device (no floating-point atomic, no host read-back): the same state
 *   gives the same bits, between calls and between contexts.
 * Not modelled: open chambers closed by a plane; the mass, the temperature and any leakage of the enclosed gas; the gas law under the iterative solver or on
 * a sharded context.
 * ipcgpu_set_chambers: chamber c owns the triangles [triEnd_nCh[c - 1], triEnd_nCh[c]) (from 0 for c = 0) of tri_colmajor (nTri x 3, nTri = triEnd_nCh[nCh - 1]);
 * pressure_nCh per chamber.  After ipcgpu_set_mesh, before ipcgpu_opt_init (else IPCGPU_ERR_STATE) and before ipcgpu_linsys_set_pattern: the three edges
 * of every triangle join vNeighbor (a node pattern that exists already is rebuilt by this call, without extra pairs).  It changes no mass and marks no
 * node.  IPCGPU_ERR_ARG, with a message that names the chamber and the triangle or edge: a node id out of range, a triangle that repeats a node, an edge of a
 * chamber that is not used by exactly two of that chamber's triangles (an open surface), two triangles that traverse a shared edge in the same direction,
 * an empty chamber, triEnd not ascending, a pressure that is not finite, a rest volume <= 0 (the chamber is oriented inward).  nCh == 0 removes the
 * chambers (no-op without any), a second call replaces them.  Sharded context: IPCGPU_ERR_UNSUPPORTED (both ways: ipcgpu_ctx_set_shard refuses a context
 * with chambers).  ipcgpu_set_mesh drops them.  Pressures are not part of the status file.
 * With chambers set their term enters the stepper and the building blocks wherever the shell, rod and tetrahedral elastic terms do, with the same
 * coefficient; ipcgpu_opt_system_report returns IPCGPU_ERR_UNSUPPORTED.  Without any no chamber kernel is ever launched.
 * ipcgpu_chamber_set_pressure: new pressures, at any time, also between time steps; checks that they are finite and that a gas chamber keeps
 * p_amb + p_c > 0 (IPCGPU_ERR_ARG) and needs chambers (IPCGPU_ERR_STATE without).
 * ipcgpu_chamber_set_gas: per chamber isGas (0: constant), ambient, gamma and fillVolume (a null pointer or a value <= 0: the rest volume); the values of a
 * chamber with isGas == 0 are not looked at.  After ipcgpu_set_chambers (IPCGPU_ERR_STATE without chambers), at any time, also between time steps.
 * IPCGPU_ERR_ARG, naming the chamber: a value that is not finite, ambient < 0, gamma < 1, ambient + p_c <= 0, more than 8 gas chambers.  All isGas == 0
 * restores the constant chambers exactly (the launches and the bits of a context that never called it).  ipcgpu_set_chambers drops the gas law.  Gas
 * parameters are not part of the status file.
 * ipcgpu_chamber_gas_get: what ipcgpu_chamber_set_gas set (a constant chamber: 0, 0, 1, its rest volume).  Any pointer may be null.
 * ipcgpu_chamber_gas_state: per chamber at the current positions V, gauge(V) and beta (a constant chamber: its volume, p_c and 0; V <= 0 of a gas chamber:
 * gauge = beta = 0).  Any pointer may be null.
 * ipcgpu_chamber_volume_gradient: u = gradV of one chamber (gas or constant) at the current positions, 3 nV doubles, xyz interleaved; with projectDBC the
 * entries of projected Dirichlet nodes are dropped, as in the gradient.
 * ipcgpu_chamber_gas_solve: x = (A + coef sum_c beta_c u_c u_c^T)^-1 rhs, A the matrix as last assembled and factorised (exact solvers), the sum over the gas
 * chambers with beta and u (Dirichlet entries projected) at the current positions: the routine the stepper wraps its own solve in.  Without a gas chamber:
 * ipcgpu_linsys_solve.
 * With a gas chamber the building blocks follow the gas energy: ipcgpu_chamber_energy returns W; _gradient_add uses gauge(V); _hessian_add and
 * ipcgpu_assemble_newton add ONLY THE SPARSE PART, -gauge(V) d2V/dx2 projected -- the rank-one part exists in ipcgpu_chamber_gas_solve and the stepper alone;
 * _energy_per_elem gives a gas chamber's triangle the share W_c V_t / V_c.
 * ipcgpu_chamber_get: counts2 = {nCh, nTri}; the lists as given; restVolume_nCh the volume at the rest positions; the current pressures.  Any pointer may be null.
 * ipcgpu_chamber_state: per chamber, at the current positions, the enclosed volume and the surface area (a deterministic segmented reduction; the volume is
 * taken about the centroid mean of the current positions), and refPoint_3nCh, the r_c the evaluations use now.  Any pointer may be null.
 * ipcgpu_chamber_energy / _energy_per_elem / _gradient_add / _hessian_add: the semantics of their ipcgpu_attach_* namesakes (the energy after ipcgpu_opt_init;
 * per-triangle terms unscaled; projected Dirichlet entries dropped; a block the pattern lacks: IPCGPU_ERR_STATE; fp64 atomics; a chamber with p == 0 adds nothing).
 * Without chambers every query returns IPCGPU_OK and does nothing. */
int ipcgpu_set_chambers(ipcgpu_ctx*, int nCh, const int* triEnd_nCh, const int* tri_colmajor, const double* pressure_nCh);
int ipcgpu_chamber_set_pressure(ipcgpu_ctx*, const double* pressure_nCh);
int ipcgpu_chamber_get(ipcgpu_ctx*, int* counts2, int* triEnd_nCh, int* tri_colmajor, double* restVolume_nCh, double* pressure_nCh);
int ipcgpu_chamber_state(ipcgpu_ctx*, double* volume_nCh, double* area_nCh, double* refPoint_3nCh);
int ipcgpu_chamber_energy(ipcgpu_ctx*, double coef, double* energy);
int ipcgpu_chamber_energy_per_elem(ipcgpu_ctx*, double* perTri_nTri);
int ipcgpu_chamber_gradient_add(ipcgpu_ctx*, double coef, int projectDBC, double* grad_3nV);
int ipcgpu_chamber_hessian_add(ipcgpu_ctx*, double coef, int projectDBC);
int ipcgpu_chamber_set_gas(ipcgpu_ctx*, const int* isGas_nCh, const double* ambient_nCh, const double* gamma_nCh, const double* fillVolume_nCh /*nullable or <= 0: rest volume*/);
int ipcgpu_chamber_gas_get(ipcgpu_ctx*, int* isGas_nCh, double* ambient_nCh, double* gamma_nCh, double* fillVolume_nCh);
int ipcgpu_chamber_gas_state(ipcgpu_ctx*, double* volume_nCh, double* gauge_nCh, double* beta_nCh);
int ipcgpu_chamber_volume_gradient(ipcgpu_ctx*, int chamber, int projectDBC, double* u_3nV);
int ipcgpu_chamber_gas_solve(ipcgpu_ctx*, double coef, const double* rhs_3nV, double* x_3nV);
/* Wind and air drag on shells and body surfaces: a load that depends on how a surface faces the air and how fast it moves through it (a sheet that sinks
 * instead of dropping, a flag, a parachute, a balloon that slows down).  A project extension: the reference has none, and gravity or ipcgpu_opt_add_neumann
 * (a constant acceleration) cannot stand in for it.
 *   An aerodynamic surface is a list of triangles over any nodes of the mesh -- shell triangles, boundary faces of tetrahedral components --; it need not be
 *   closed.  Surface s has a normal coefficient Cn >= 0, a tangential coefficient Ct >= 0 and a flag oneSided; globally there is a wind velocity w, uniform
 *   in space, and an air density rho_a > 0 (defaults: still air, 1.225).
 *   lagging     Per triangle the unit normal n (right-hand rule), the area A and the centroid c^n are taken at the positions the time step starts from:
 *               ipcgpu_set_aero computes them at the rest positions, ipcgpu_opt_begin_timestep refreshes them on the device before any scripted move, and
 *               they stay fixed through that step's Newton iterations and line searches.  ipcgpu_set_positions does not move them.
 *   energy      at positions x, with c = (x0 + x1 + x2) / 3:  u = (c - c^n) / dt - w,  u_n = u . n,  u_t = u - u_n n,  s_n = u_n (two-sided) or
 *               max(0, u_n) (one-sided: only the face that pushes into the air is loaded);  the dissipative potential
 *               D_t = dt (rho_a A / 6) (Cn |s_n|^3 + Ct |u_t|^3);  the force on the centroid -dD_t/dc = -(rho_a A / 2) (Cn |s_n| s_n n + Ct |u_t| u_t), a
 *               third of it on each node;  the exact Hessian K = (rho_a A / (2 dt)) (2 Cn |s_n| n n^T + Ct (|u_t| (I - n n^T) + u_t u_t^T / |u_t|)), PSD as it
 *               stands (no projection), K / 9 in each of the nine nodal blocks.  At |u_t| = 0 the tangential part is exactly zero, at s_n = 0 the normal
 *               part, a triangle of zero lagged area contributes nothing; nothing is written for a part that vanishes, and no NaN or Inf is produced.
 *   D enters the stepper and the building blocks (ipcgpu_assemble_newton, ipcgpu_incremental_potential, ipcgpu_gradient) wherever the elastic
 *   codimensional terms do, with the same coefficient.  Under Newmark the velocity the term sees is still (x - x^n) / dt, as the lagged friction's: the load
 *   is then first order in time.  Rows, columns and gradient entries of projected Dirichlet nodes are dropped; their motion still counts in c.  The term is no
 *   stiffness: it does not enter the lagged stiffness damping (ipcgpu_opt_set_damping), whose matrix is to the bit what it is without surfaces.  Contact is
 *   NOT changed.  Both exact solvers and the iterative solver work (the term is sparse).
 * Not modelled: lift other than the normal component of flat-plate drag; shading of one surface by another; wind that varies in space; rods; sharded
 * contexts (IPCGPU_ERR_UNSUPPORTED, both ways: ipcgpu_ctx_set_shard refuses a context with surfaces); ipcgpu_opt_system_report returns
 * IPCGPU_ERR_UNSUPPORTED while surfaces are set.
 * ipcgpu_set_aero: surface s owns the triangles [triEnd_nSurf[s - 1], triEnd_nSurf[s]) (from 0 for s = 0) of tri_colmajor (nTri x 3, nTri =
 * triEnd_nSurf[nSurf - 1]); cn, ct, oneSided per surface.  After ipcgpu_set_mesh, before ipcgpu_opt_init (else IPCGPU_ERR_STATE) and before
 * ipcgpu_linsys_set_pattern: the three edges of every triangle join vNeighbor (a node pattern that exists already is rebuilt by this call).  It changes no
 * mass and marks no node.  IPCGPU_ERR_ARG, with a message that names the surface and the triangle: a node id out of range, a triangle that repeats a node,
 * zero rest area, a triangle listed twice (in one surface or in two, in any rotation or orientation), a coefficient that is negative or not finite, an
 * empty surface, triEnd not ascending.  nSurf == 0 removes the surfaces (no-op without any; wind and density return to their defaults), a second call
 * replaces them (wind and density stay).  ipcgpu_set_mesh drops them.  Without a surface no aero kernel is ever launched.
 * ipcgpu_aero_set_wind: the wind velocity and the air density, at any time, also between time steps: the next step sees them.  IPCGPU_ERR_ARG for a wind
 * that is not finite or a density that is not positive and finite.
 * ipcgpu_aero_get: counts2 = {nSurf, nTri}; the lists and coefficients as given; the wind and the density.  Any pointer may be null.
 * ipcgpu_aero_state: at the current positions the force -dD_t/dc on every triangle (force_3nTri, xyz interleaved); lagged_8nTri, the records the
 * evaluations use now (n, A, c^n, 0 per triangle); total5 = the total force (3), the dissipated power sum -f . u (>= 0) and the loaded area (the lagged area
 * of the triangles that carry a force).  The totals are summed in two passes in a fixed order on the device: bit-reproducible.  Any pointer may be null;
 * force and total5 need ipcgpu_opt_init (it supplies dt).
 * ipcgpu_aero_energy / _energy_per_elem / _gradient_add / _hessian_add: the semantics of their ipcgpu_chamber_* namesakes (per-triangle terms unscaled;
 * projected Dirichlet entries dropped; a block the pattern lacks: IPCGPU_ERR_STATE; fp64 atomics), all after ipcgpu_opt_init (IPCGPU_ERR_STATE before).
 * Without a surface every one of these calls returns IPCGPU_OK and does nothing. */
int ipcgpu_set_aero(ipcgpu_ctx*, int nSurf, const int* triEnd_nSurf, const int* tri_colmajor, const double* cn_nSurf, const double* ct_nSurf, const int* oneSided_nSurf);
int ipcgpu_aero_set_wind(ipcgpu_ctx*, const double* wind3, double density);
int ipcgpu_aero_get(ipcgpu_ctx*, int* counts2, int* triEnd_nSurf, int* tri_colmajor, double* cn_nSurf, double* ct_nSurf, int* oneSided_nSurf, double* wind3, double* density);
int ipcgpu_aero_state(ipcgpu_ctx*, double* force_3nTri, double* lagged_8nTri, double* total5);
int ipcgpu_aero_energy(ipcgpu_ctx*, double coef, double* energy);
int ipcgpu_aero_energy_per_elem(ipcgpu_ctx*, double* perTri_nTri);
int ipcgpu_aero_gradient_add(ipcgpu_ctx*, double coef, int projectDBC, double* grad_3nV);
int ipcgpu_aero_hessian_add(ipcgpu_ctx*, double coef, int projectDBC);
/* ---- Fibre reinforcement and active contraction of tetrahedral elements.  No counterpart in the reference (every body of it is isotropic).  The model, its
 * degenerate states and what is not modelled are stated in ipc_amd/csrc/fiber_kernels.h.  Per fibred element with rest volume vol, unit rest direction a and
 * b = restTriInv a: d = b1 (x1 - x0) + b2 (x2 - x0) + b3 (x3 - x0) = F a, l = |d| the fibre stretch, W = vol psi(l); the Hessian blocks are the closed-form
 * PSD projection.  The term is one of the codimensional energies of the stepper (it enters the lagged stiffness damping) and adds no pair to the pattern.
 * ipcgpu_set_fibers: elements [tetBegin, tetEnd) get one fibre family; ranges as in ipcgpu_set_component_material, a later call overwrites, k == 0 removes.
 *   dir: 3 doubles in the frame of the rest positions (dirPerElement != 0: 3 per element of the range, element-major); normalised by the call.
 *   law 0 (spring): psi = k (l - l0)^2 / 2 with l0 = 1 - act(group); tensionOnly != 0: psi = 0 for l <= l0.  law 1 (exp): psi = k / (2 k2) (exp(k2 (l^2 - 1)^2) - 1)
 *   for l > 1, 0 otherwise; k2 is read under law 1 alone.  k is a stress (Pa), the caller's: no material scales it.  group: 0 .. 63.
 *   IPCGPU_ERR_ARG, and nothing is changed: a range outside [0, nT), a null, zero or non-finite direction, k < 0 or not finite, an unknown law, law 1 with
 *   k2 <= 0, a group outside [0, 64), law 1 on a group whose activation is not 0.  IPCGPU_ERR_UNSUPPORTED: an element of the range is plastic
 *   (ipcgpu_set_plasticity on a fibred element returns the same), or the context is sharded (ipcgpu_ctx_set_shard with world > 1 on a context with fibres
 *   returns the same).  Allowed any time after ipcgpu_set_mesh, before or after ipcgpu_opt_init, between time steps.  With no fibred element the stepper
 *   launches nothing and every result is bit-identical to a context that never called this.  ipcgpu_set_mesh_features with a restTriInv or a volume
 *   recomputes b and vol k; ipcgpu_set_mesh drops the fibres.
 * ipcgpu_fiber_set_activation: act < 1 of one group (0: passive; 0.3: the fibres want to be 30 % shorter); uploads 64 doubles and nothing per element.
 *   IPCGPU_ERR_ARG: act >= 1 or not finite, a group out of range, act != 0 on a group that holds a law-1 element.  IPCGPU_ERR_STATE before ipcgpu_set_fibers.
 * ipcgpu_fiber_get: the number of fibred elements, per element k, k2, the law, tension-only (1 under law 1), the group and the unit direction (nT x 3,
 *   element-major; zeros without a fibre), and the 64 activations.  Any pointer may be NULL.
 * ipcgpu_fiber_energy / _energy_per_elem (nT, 0 without a fibre) / _gradient_add / _hessian_add: as the ipcgpu_attach_* calls of the same names.
 * ipcgpu_fiber_state: read-only.  perElem (nullable, column-major nT x 5): l, the tension psi'(l) (a stress), the current direction t; an element without
 *   fibres gets 1, 0 and 0 0 0.  totals3 (nullable): min l and max l over the fibred elements (1 and 1 without any) and the sum of W.  Deterministic.
 * ipcgpu_opt_save_status appends a section `fiber <nT> 7 64` (the activations, then k, k2, flag word, group and direction per element) when an element is
 *   fibred -- the file is otherwise byte for byte what it was; ipcgpu_opt_load_status reads it and replaces the context's fibres with it. */
int ipcgpu_set_fibers(ipcgpu_ctx*, int tetBegin, int tetEnd, const double* dir, int dirPerElement, double k, int law, double k2, int tensionOnly, int group);
int ipcgpu_fiber_set_activation(ipcgpu_ctx*, int group, double act);
int ipcgpu_fiber_get(ipcgpu_ctx*, int* nFibred, double* k_nT, double* k2_nT, int* law_nT, int* tensionOnly_nT, int* group_nT, double* dir_3nT, double* act_64);
int ipcgpu_fiber_energy(ipcgpu_ctx*, double coef, double* energy);
int ipcgpu_fiber_energy_per_elem(ipcgpu_ctx*, double* perTet_nT);
int ipcgpu_fiber_gradient_add(ipcgpu_ctx*, double coef, int projectDBC, double* grad_3nV);
int ipcgpu_fiber_hessian_add(ipcgpu_ctx*, double coef, int projectDBC);
int ipcgpu_fiber_state(ipcgpu_ctx*, double* perElem_nTx5, double* totals3);
/* ---- Plastic flow of tetrahedral elements: yield, creep, isotropic hardening.  No counterpart in the reference (every body of it is elastic).
 * The model is stated in ipc_amd/csrc/plastic_kernels.h.  Per element with a finite yield strain, at the end of every time step (after the BE / Newmark
 * update, before the lagged damping matrix): F = Ds(x) restTriInv = U diag(s) V^T; skipped and counted where s2 <= 0; e = ln s, d = e - mean(e), n = |d|;
 * y = yield + harden alpha; where n > y: Delta = -expm1(-creep dt) (n - y) / (1 + harden), restTriInv <- restTriInv V diag(exp(-Delta d_i / n)) V^T,
 * alpha += Delta.  Isochoric (volumes and masses do not change).  For small strains the von Mises stress of ipcgpu_elastic_stress is sqrt(6) mu n, so a yield
 * stress sigma_y corresponds to yield = sigma_y / (sqrt(6) mu).
 * ipcgpu_set_plasticity (no counterpart in the reference): elements [tetBegin, tetEnd) get (yield, creep, harden); ranges as in ipcgpu_set_component_material,
 *   later calls overwrite.  yield >= 0 or +inf (+inf switches the range off), creep > 0 or +inf (+inf: the rate-independent return onto the yield
 *   surface), harden >= 0 and finite, nothing NaN: IPCGPU_ERR_ARG otherwise, and nothing is changed.  Touches neither the pattern nor the masses: allowed any
 *   time after ipcgpu_set_mesh, before or after ipcgpu_opt_init, between time steps.  The first call keeps a copy A0 of the current restTriInv.  With no
 *   element switched on the stepper launches nothing and every result is bit-identical to a context that never called this.  IPCGPU_ERR_UNSUPPORTED on a
 *   sharded context; ipcgpu_ctx_set_shard with world > 1 on a context with plastic elements returns the same.
 * ipcgpu_plastic_get (no counterpart): the parameters, the accumulated plastic strain alpha and A0 (layout of ipcgpu_get_features); any pointer may be NULL.
 * ipcgpu_plastic_update (no counterpart): ONE flow at the held positions with the given dt, outside the stepper -- the kernel's test entry, like the
 *   *_hessian_add calls.  nYielded / nSkipped (nullable): elements rewritten / found flat or inverted.
 * ipcgpu_plastic_state (no counterpart): read-only.  perElem (nullable, column-major nT x 3): n, the current y, alpha; n = NaN for an element the flow would
 *   skip, y = +inf where plasticity is off.  totals4 (nullable): yielded and skipped in the last flow, max alpha, sum of rest volume times alpha.
 *   Deterministic: fixed summation order, no floating-point atomics.
 * ipcgpu_plastic_set_state (no counterpart): restTriInv (layout of ipcgpu_get_features) and / or alpha from the caller (either may be NULL); needs
 *   ipcgpu_set_plasticity first.  ipcgpu_plastic_reset (no counterpart): restTriInv = A0, alpha = 0.
 * ipcgpu_opt_save_status appends a section `plastic <nT> 10` (nine entries of restTriInv, then alpha, per element) when an element is plastic -- the file is
 * otherwise byte for byte what it was, and the reference's reader skips the tokens; ipcgpu_opt_load_status reads it (a file without it leaves both untouched). */
int ipcgpu_set_plasticity(ipcgpu_ctx*, int tetBegin, int tetEnd, double yield, double creep, double harden);
int ipcgpu_plastic_get(ipcgpu_ctx*, double* yield_nT, double* creep_nT, double* harden_nT, double* alpha_nT, double* restTriInv0_9nT);
int ipcgpu_plastic_update(ipcgpu_ctx*, double dt, int* nYielded, int* nSkipped);
int ipcgpu_plastic_state(ipcgpu_ctx*, double* perElem_nTx3, double* totals4);
int ipcgpu_plastic_set_state(ipcgpu_ctx*, const double* restTriInv_9nT, const double* alpha_nT);
int ipcgpu_plastic_reset(ipcgpu_ctx*);
/* SelfCollisionHandler::computeConstraintSet (SelfCollisionHandler.cpp:2149-2478) at the current positions:
 * MMActiveSet (PP / PE duplicates merged, multiplicity in slot 3), paraEEMMCVIDSet + paraEEeIeJSet, and the
 * candidate list for the partial CCD.  counts3 = {nActive, nParaEE, nCandidates}. */
int ipcgpu_contact_build(ipcgpu_ctx*, double dHat, int* counts3);
/* the sizes of the sets the library holds since the last ipcgpu_contact_build / _set, counts3 as above (an adapter checks with it that the candidate list it is
 * handed -- MMActiveSet_CCD of Optimizer.cpp:1926 -- is the one the library will sweep in ipcgpu_ccd_partial) */
int ipcgpu_contact_counts(ipcgpu_ctx*, int* counts3);
int ipcgpu_contact_get(ipcgpu_ctx*, int* active_4n, int* paraEE_4n, int* paraEEeIeJ_2n, int* csPTEE_2n /*nullable*/);
/* hand an active set in (adapters that keep the reference's own constraint-set code; tests) */
int ipcgpu_contact_set(ipcgpu_ctx*, int nActive, const int* active_4n, int nParaEE, const int* paraEE_4n, const int* paraEEeIeJ_2n);
/* kappa * (sum mult b(d) + sum e(c) b(d))  -- the barrier part of computeEnergyVal (Optimizer.cpp:3252-3353) */
int ipcgpu_contact_energy(ipcgpu_ctx*, double dHat, double kappa, double* energy);
/* The reference's PER-CONSTRAINT interface, on caller-held MMCVID tuples at the positions of ipcgpu_set_positions (round 5: what the compiled collision-handler
 * adapter include/adapters/HipSelfCollisionHandler.hpp forwards to when the reference's own Optimizer.cpp drives the loop):
 * evaluateConstraints (SelfCollisionHandler.cpp:37-81): val[i] = squared distance of tuple i;
 * leftMultiplyConstraintJacobianT (:84-148): out += coef * multiplicity_i * input[i] * grad d_i (multiplicity = -MMCVID[3] of a PP / PE tuple, 1 otherwise). */
int ipcgpu_contact_evaluate(ipcgpu_ctx*, int n, const int* mmcvid_4n, double* val_n);
int ipcgpu_contact_jt_multiply(ipcgpu_ctx*, int n, const int* mmcvid_4n, const double* input_n, double coef, double* out_3nV_inout);
/* grad += kappa J^T b'  (leftMultiplyConstraintJacobianT + augmentParaEEGradient, SelfCollisionHandler.cpp:84-148,
 * 2990-3036), then rows of projected Dirichlet nodes zeroed (Optimizer.cpp:3512-3516) */
int ipcgpu_contact_gradient_add(ipcgpu_ctx*, double dHat, double kappa, int projectDBC, double* grad_3nV_inout);
/* The contact report: what happens BETWEEN bodies (it extends the reference's `min distance^2` log of a converged solve, Optimizer.cpp:2402-2442, and the
 * per-object counts of outputCollStats, :3070-3087), reduced on the device.  It evaluates the sets the context HOLDS at the positions it holds -- the
 * active and the mollified set of the last ipcgpu_contact_build / _set or of the stepper's last build, every half-space's vertex set, the lagged
 * self-friction set of ipcgpu_friction_update or of the stepper -- in buffers of its own and CHANGES NO STATE.  Components: ipcgpu_opt_set_components
 * (default: one).
 * A row is one unordered pair with at least one contributing tuple: two components (a, b), a <= b, or component a and half-space h, written
 * (a, -1 - h).  Rows ascend by (a, b), the half-space rows of a behind its component rows, ascending in h.
 * Sides: primitive 1 of a decoded tuple is node 0 (PP, PE, PT) or nodes 0 and 1 (EE), primitive 2 the other nodes; of a mollified tuple the primitives
 * are the edges eI and eJ of paraEEeIeJ, whose four nodes all carry force.  A primitive's component is that of its first node.  Side A is the primitive
 * whose component is a (primitive 1 when a == b).  A half-space row has side A only.
 * Barrier part, over the tuples with d < dHat at the current positions (a held tuple at or beyond dHat contributes nothing and is not counted); the
 * force on node k is minus the node's term of ipcgpu_contact_gradient_add(projectDBC = 0) resp. ipcgpu_halfspace_gradient_add, Dirichlet rows kept:
 *   active      f_k = -kappa mult b'(d) grad_k d        mollified   f_k = -kappa (b e' grad_k c + e b' grad_k d)
 * rowsI[8 r ..]: a, b, nPP, nPE, nPT, nEE (active tuples by kind -- tuples, not multiplicities; the vertex count of a half-space row goes into nPP),
 *   nMollified, argmin (index into the list active | mollified, resp. the node id in a half-space row, of the first tuple in list order that attains
 *   minD2; -1 in a row without barrier tuples).
 * rowsD[20 r ..]: minD2 (the squared distance as ipcgpu_contact_evaluate returns it), FA[3], FB[3] (sum of f_k over the nodes of side A / B), TA[3],
 *   TB[3] (sum of x_k x f_k), RA[3], RB[3], W.
 * Friction part, only with Vt != NULL, coef > 0 and a non-empty lagged self-contact set: per lagged tuple the force on node k is minus what
 * ipcgpu_friction_gradient_add(Vt, eps2, coef) adds (self / obstacle scales included), summed by side into RA / RB; W = sum_k f_k . (x_k - Vt_k), the
 * work of the lagged friction forces over the step (<= 0 up to round-off).  A row that exists through friction alone has zero counts and minD2 = +inf.
 * After ipcgpu_opt_solve_timestep the lagged set is the one ipcgpu_opt_next_subproblem took at the CONVERGED positions (the lag is renewed before the
 * stepper decides whether another friction sub-problem follows): the friction columns then are the forces of that fresh lag over the step's motion, not
 * the friction terms the step's last Newton solve balanced.
 * HALF-SPACE FRICTION IS NOT REPORTED (no entry point exposes its per-node terms): the friction columns of half-space rows are 0.
 * capacity < number of rows: IPCGPU_ERR_ARG with *nRows set (capacity = 0 with null arrays asks for the size); no row: *nRows = 0, IPCGPU_OK.  Before
 * ipcgpu_set_surface: IPCGPU_ERR_STATE.  Sharded context: IPCGPU_ERR_UNSUPPORTED; so are more than 2^22 keys nComp (nComp + 1) / 2 + nComp nHalfSpaces
 * (the histogram over the pairs is dense; about 2 890 components).  Cost: linear in the number of held tuples except for the pass that orders a row's
 * records, which compares every record of a row with every other -- quadratic in the LONGEST row (3.4 ms for one row of 22 K tuples on an MI355X; rows of a
 * few hundred thousand tuples, e.g. two large bodies or the default single component of a large scene, take seconds).  fp64, no floating-point atomics, a fixed summation order (records of a row in the
 * order active, mollified, half-spaces by id, friction, then set order): the same state gives the same bits. */
int ipcgpu_contact_report(ipcgpu_ctx*, double dHat, double kappa, const double* Vt_colmajor /*nullable*/, double eps2, double coef, int capacity, int* nRows,
    int* rowsI_8n, double* rowsD_20n);
/* a += PSD-projected barrier Hessians (augmentIPHessian + augmentParaEEHessian, SelfCollisionHandler.cpp:418-561,
 * 3039-3201).  The pattern must already contain the contact connectivity (ipcgpu_contact_connectivity ->
 * ipcgpu_linsys_set_pattern); otherwise IPCGPU_ERR_STATE. */
int ipcgpu_contact_hessian_add(ipcgpu_ctx*, double dHat, double kappa, int projectDBC);
/* augmentConnectivity (SelfCollisionHandler.cpp:330-415): node pairs (a < b) coupled by the barrier Hessians */
int ipcgpu_contact_connectivity(ipcgpu_ctx*, int capacity, int* pairs_2n, int* nPairs);
/* Conservative CCD step bounds (the role of SelfCollisionHandler::largestFeasibleStepSize, :564-686, on the candidate
 * list of the last contact_build, and of largestFeasibleStepSize_CCD, :982-1366, on every pair whose swept boxes
 * overlap).  Contract (CTCD itself is un-vendored): the returned step keeps every tested pair at
 * >= (1 - slackness) of its current distance.  pair2 = limiting pair, (-svI-1, sfI) or (eI, eJ); (0,0) if none. */
int ipcgpu_ccd_partial(ipcgpu_ctx*, const double* searchDir_3nV, double slackness, double* stepSize_inout, int* pair2);
int ipcgpu_ccd_full(ipcgpu_ctx*, const double* searchDir_3nV, double slackness, double* stepSize_inout, int* pair2, int* nCandidates);
/* The full sweep exactly as the reference runs it (largestFeasibleStepSize_CCD, SelfCollisionHandler.cpp:982-1366, over the swept
 * SpatialHash::build, SpatialHash.hpp:589-832, whose step-size argument is a reference): (1) the hash caps the step so that the mean
 * |component| of the search direction over the surface nodes, times the step, stays below its cell size avgEdgeLen / 3 -- returned in
 * alphaCapped; (2) a surface vertex is swept against the surface vertices (svJ > svI), the edges and the triangles that share a cell
 * with it, an edge against the edges (eJ > eI) that share a cell and whose swept boxes overlap; (3) each pair with the safety
 * distance (1 - slackness) * its own current distance, asked again without it when it reports t < 1e-6.  The per-pair query is the
 * conservative advancement of ipcgpu_ccd_full (CTCD is un-vendored).  arg3 = limiting pair (kind, i, j): 0 (svI, svJ), 1 (svI, eI),
 * 2 (svI, sfI), 3 (eI, eJ); (-1,-1,-1) if none.  This is what the time stepper uses (ipcgpu_set_ccd_mode 1, the default);
 * mode 0 keeps the swept-box sweep over point-triangle / edge-edge pairs of ipcgpu_ccd_full. */
int ipcgpu_ccd_full_reference(ipcgpu_ctx*, const double* searchDir_3nV, double slackness, double* stepSize_inout, double* alphaCapped, int* arg3,
    int* nCandidates);
int ipcgpu_set_ccd_mode(ipcgpu_ctx*, int mode);
/* isIntersected / checkEdgeTriIntersectionIfAny (Optimizer.cpp:2626-2659, SelfCollisionHandler.cpp:3255-3300) */
int ipcgpu_is_intersected(ipcgpu_ctx*, int* flag);

/* ---- Optimizer<3>: the time stepper itself, state resident on the GPU --------------- */
/* Optimizer ctor + setTime (Optimizer.cpp:97-115, 418-430).  Uses the mesh of this context. */
int ipcgpu_opt_init(ipcgpu_ctx*, double dt, int withGravity);
int ipcgpu_opt_set_rel_tol(ipcgpu_ctx*, double relTol); /* setRelGL2Tol, Optimizer.cpp:390-396 */
/* `script twist` (AnimScripter.cpp:555-572, 1674-1684): two handle sets rotating about x */
int ipcgpu_opt_set_twist(ipcgpu_ctx*, int nLeft, const int* left, int nRight, const int* right, double angVel);
/* `selfCollisionOn` with the interior-point solver (Config.cpp:41-45, Optimizer.cpp:1534-1550): needs ipcgpu_set_surface;
 * dHat = dHatEps^2 * bboxDiag^2 (`dHat` keyword, default 1e-3).  From then on the stepper builds constraint sets, adds the
 * barrier terms, adapts kappa and bounds every step by CCD exactly as fullyImplicit_IP / solveSub_IP do. */
int ipcgpu_opt_enable_self_collision(ipcgpu_ctx*, double dHatEps);
/* Look-ahead of the contact pattern (no counterpart in the reference, which rebuilds pattern + symbolic analysis whenever the contact graph changes,
 * Optimizer.cpp:3570-3592; here the pattern only grows and a new analysis is needed when a pair shows up that the pattern lacks): on such a change the new
 * pattern takes the full stencils of the candidate set at `pad` x dHat (squared distances), blocks of pairs that are not active yet hold explicit zeros.
 * pad < 1: exactly the live pairs; 1: full stencils of the current candidates; > 1: fewer analyses, more fill in the factor.  Default (never called): 4 (twice
 * the distance) for meshes up to 150 K nodes, 2.25 beyond -- measured on the bench's contact workloads, profiles/r06_pattern_lookahead_ab.txt.
 * The Newton iterates do not depend on it (explicit zeros); what it trades is host-side analyses against factorisation flops. */
int ipcgpu_opt_set_pattern_lookahead(ipcgpu_ctx*, double pad);
/* analytic half-space obstacle (`ground` / `halfSpace` keywords, Config.cpp:306-345; HalfSpace.cpp:41-85): points with
 * normal.(x - origin) > 0 are free.  Needs ipcgpu_set_surface.  Returns its index in *id.  The stepper then builds its
 * vertex constraint set (CollisionObject.h:323-351), adds barrier energy / gradient / diagonal Hessian blocks
 * (HalfSpace.cpp:106-214) and bounds each step by the ray test with slackness 0.9 (HalfSpace.cpp:242-269). */
int ipcgpu_opt_add_half_space(ipcgpu_ctx*, const double* origin3, const double* normal3, double dHatEps, int* id);
/* the same pieces one by one (adapter for a HalfSpace<3> subclass).  verts = activeSet[coI], ascending surface order. */
int ipcgpu_halfspace_build(ipcgpu_ctx*, int id, double dHat, int cap, int* verts, int* n);
int ipcgpu_halfspace_set(ipcgpu_ctx*, int id, int n, const int* verts);
int ipcgpu_halfspace_energy(ipcgpu_ctx*, int id, double dHat, double kappa, double* E);
int ipcgpu_halfspace_gradient_add(ipcgpu_ctx*, int id, double dHat, double kappa, double* grad_3nV_inout);
int ipcgpu_halfspace_hessian_add(ipcgpu_ctx*, int id, double dHat, double kappa, int projectDBC);
/* HalfSpace::move (HalfSpace.cpp:389-416), what the ACO* scripts of AnimScripter call before a time step (AnimScripter.cpp:1832-1890): the plane's
 * origin moves along delta by the largest fraction <= 1 that keeps `slackness` of the distance of every surface node (Dirichlet nodes included);
 * stepSizeLeft = 1 - that fraction. */
int ipcgpu_halfspace_move(ipcgpu_ctx*, int id, const double* delta3, double slackness, double* stepSizeLeft);
int ipcgpu_halfspace_step_bound(ipcgpu_ctx*, int id, const double* searchDir_3nV, double slackness, double* stepSize_inout);

/* ---- round colliders: analytic spheres and capsules beside the half-space (a project extension; model in ipc_amd/csrc/round_collider_kernels.h) ----
 * A round collider is the segment [p0, p1] with radius R > 0: a sphere where p0 == p1 (exactly), a capsule otherwise.  hollow = 1 (spheres only):
 * the bodies live inside, as in a bowl; it needs R^2 > dHat.  With q the closest point of the segment, r = |x - q|, the signed distance is
 * s = side (r - R), side = +1 / -1 (solid / hollow); the barrier is kappa b(s^2, dHat) on the surface vertices with dbc == 0 and s^2 < dHat.  The
 * Hessian touches only the diagonal 3 x 3 block of a node, so the matrix pattern never changes.  Needs ipcgpu_set_surface; shares the context's one
 * dHatEps; refused with IPCGPU_ERR_UNSUPPORTED on a sharded context, and IPCGPU_ERR_STATE where a node with dbc == 0 lies on or inside the collider
 * at the current positions (ipcgpu_opt_begin_timestep asks again).  Returns its index in *id (round colliders count separately from half-spaces).
 * The stepper visits the round colliders right after the half-spaces: constraint set, barrier energy / gradient / Hessian, step bound with slackness
 * 0.9, intersection check, kappa adaptation, lagged friction.  ipcgpu_opt_system_report is refused while one is set, and ipcgpu_contact_report does
 * not list them: ipcgpu_round_state serves that purpose. */
int ipcgpu_opt_add_round_collider(ipcgpu_ctx*, const double* p0_3, const double* p1_3, double R, int hollow, double dHatEps, int* id);
/* the same pieces one by one, as the ipcgpu_halfspace_* list.  verts: the active set in ascending surface order. */
int ipcgpu_round_build(ipcgpu_ctx*, int id, double dHat, int cap, int* verts, int* n);
int ipcgpu_round_set(ipcgpu_ctx*, int id, int n, const int* verts);
int ipcgpu_round_energy(ipcgpu_ctx*, int id, double dHat, double kappa, double* E);
int ipcgpu_round_gradient_add(ipcgpu_ctx*, int id, double dHat, double kappa, double* grad_3nV_inout);
int ipcgpu_round_hessian_add(ipcgpu_ctx*, int id, double dHat, double kappa, int projectDBC);
/* the first t in (0, *stepSize_inout] at which some surface vertex with dbc == 0 has s(x + t p) = (1 - slackness) s(x); unchanged where no ray gets there */
int ipcgpu_round_step_bound(ipcgpu_ctx*, int id, const double* searchDir_3nV, double slackness, double* stepSize_inout);
/* translate the collider by the largest fraction <= 1 of delta that keeps `slackness` of every surface node's gap (Dirichlet nodes included);
 * stepSizeLeft = 1 - that fraction, like ipcgpu_halfspace_move */
int ipcgpu_round_move(ipcgpu_ctx*, int id, const double* delta3, double slackness, double* stepSizeLeft);
int ipcgpu_round_get(ipcgpu_ctx*, int id, double* p0_3, double* p1_3, double* R, int* hollow); /* any pointer may be null */
/* lagged friction piece by piece: lambda and the unit normal of every entry of the current set are stored (the lagged tangent plane); energy,
 * gradient and Hessian are the half-space's with that per-entry normal, Vt = x^t (3 nV), eps2 = the squared velocity threshold times h^2 */
int ipcgpu_round_lag_update(ipcgpu_ctx*, int id, double dHat, double kappa, int* nLagged);
int ipcgpu_round_friction_energy(ipcgpu_ctx*, int id, const double* Vt, double eps2, double* E);
int ipcgpu_round_friction_gradient_add(ipcgpu_ctx*, int id, const double* Vt, double eps2, double* grad_3nV_inout);
int ipcgpu_round_friction_hessian_add(ipcgpu_ctx*, int id, const double* Vt, double eps2, int projectDBC);
/* State of one collider at the current positions and set.  *nSet: the set size.  out10[0]: the smallest s over the surface nodes (Dirichlet nodes
 * included; +infinity without a surface node); out10[1..3]: the total barrier force on the bodies (minus the barrier gradient over the set);
 * out10[4..6]: its torque about p0; out10[7..9]: the total lagged friction force (zero while nothing is lagged), with x^t and the velocity threshold
 * of the stepper.  dHat, kappa <= 0: the stepper's current values.  Summed in a fixed order: two calls on one state agree to the bit. */
int ipcgpu_round_state(ipcgpu_ctx*, int id, double dHat, double kappa, int* nSet, double* out10);
/* ---- lagged smoothed Coulomb friction (FrictionUtils.hpp, SelfCollisionHandler.cpp:2481-2988, HalfSpace.cpp:272-381)
 * `selfFric mu` / `fricIterAmt n` / eps_v = tuning[4] (Config.cpp:482-488, 550-551, 45).  Self friction needs self collision. */
/* NOTE on eps_v: the smoothing distance the friction terms use is eps_v^2 * h^2 * (bounding-box diagonal)^2 with h = 0.025 -- the step size of the
 * setTime(10.0, 0.025) inside the reference's Optimizer constructor (Optimizer.cpp:116, 290-303) -- NOT the dt of ipcgpu_opt_init: the reference sets
 * the scene's dt afterwards (main.cpp:1398) without recomputing it, and this library follows the reference (CN_MBC of :268 likewise). */
int ipcgpu_opt_set_friction(ipcgpu_ctx*, double selfFric, int fricIterAmt, double epsV);
/* eps_v homotopy: `tuning`'s sixth entry (Config.cpp:41-45, Optimizer.cpp:296-303).  The smoothing distance of the friction terms starts every
   time step at eps_v (fifth entry) and is halved down -- or clamped up -- to eps_v_target between the friction-lag passes (:1776-1781); the
   tangent-space convergence test runs only once it has arrived (:1717).  <= 0: the target is eps_v itself (what the `epsv` keyword sets). */
int ipcgpu_opt_set_friction_target(ipcgpu_ctx*, double eps_v_target);
/* The step size h inside eps_v^2 h^2 (fricDHat0 / fricDHatTarget) and CN_MBC.  In the reference these are evaluated in the Optimizer constructor right after its
   setTime(10.0, 0.025) (Optimizer.cpp:116, 268, 290-303) and never again when main.cpp:1398 sets the scene's dt: they carry h = 0.025 whatever `time` says.  That
   is the default here; pass the scene's dt for the paper's semantics.  Call before ipcgpu_opt_init / ipcgpu_opt_precompute. */
int ipcgpu_opt_set_constructor_dt(ipcgpu_ctx*, double h);
/* The three remaining knobs of the scene file behind the interior-point lengths (Config.cpp:553-558, Config.hpp:138-139):
 *   useAbsParameters   dHat, its homotopy target, dTol, eps_v (and its target) and the Newton tolerance are ABSOLUTE lengths instead of fractions
 *                      of the rest-shape bounding-box diagonal (Optimizer.cpp:107-109, 279-302, 1535-1537, 2941-2945); suggestKappa's
 *                      distances and CN_MBC stay relative there too (:268, 2228-2233)
 *   dTolRel            tuning[3] (1e-9): below dTol = dTolRel^2 (x diagonal^2) a converged distance ends the homotopy / the close-pair
 *                      bookkeeping counts a stencil (:102-109, 1710, 1744, 2409-2434)
 *   kappaMinMultiplier 1e11 (`kappaMinMultiplier` / `minBarrierStiffnessScale`): numerator of suggestKappa and, x 100, of upperBoundKappa
 * Call it after the collision objects are registered or before -- the derived lengths are recomputed. */
int ipcgpu_opt_set_parameter_scaling(ipcgpu_ctx*, int useAbsParameters, double dTolRel, double kappaMinMultiplier);
/* MeshCO::friction (Config.cpp:459-474, MeshCO.cpp) beside Config::selfFric: a kinematic mesh obstacle carries its own friction
 * coefficient for the pairs that involve it.  Pass the larger coefficient to ipcgpu_opt_set_friction and the ratios here: the lagged
 * normal forces (MMLambda_lastH) of stencils without / with an obstacle node are multiplied by scaleSelf / scaleObstacle. */
int ipcgpu_opt_set_friction_scales(ipcgpu_ctx*, double scaleSelf, double scaleObstacle);
/* Optimizer.cpp:146-166: solveFric is also true when a mesh collision object carries a friction coefficient, although no friction
 * term is ever evaluated for its pairs (:3357-3376, 3473-3510, 3676-3705): the lagging loop with its tangent-space convergence solve
 * then runs after every converged sub-problem.  on != 0 switches that loop on without any frictional pair. */
int ipcgpu_opt_force_friction_loop(ipcgpu_ctx*, int on);
int ipcgpu_opt_set_half_space_friction(ipcgpu_ctx*, int id, double mu); /* CollisionObject::friction of half-space `id` */
int ipcgpu_opt_set_round_collider_friction(ipcgpu_ctx*, int id, double mu); /* the same for round collider `id` */
/* Lagged stiffness-proportional damping: `dampingStiff s` (Config.cpp:141-147; `dampingRatio r` is s = r * dt^3 * 3 / 4, :148-157,
 * 614-616).  The damping matrix is the PSD-projected elastic Hessian at the end of the last time step times s / dt
 * (Optimizer.cpp:593-595, 3723-3735); 1/2 dx^T D dx joins the energy (:3381-3400), D dx the gradient (:3519-3540), D the Hessian
 * (:3707-3709).  Call before ipcgpu_opt_precompute; 0 switches it off. */
int ipcgpu_opt_set_damping(ipcgpu_ctx*, double dampingStiff);
/* `tuning` entry 0 (Config.cpp:41-45, 533-541): the barrier stiffness every time step starts from, bounded from above by
 * upperBoundKappa and still raised by initKappa / the adaptive updates (Optimizer.cpp:1540-1550, 2216-2225); 0 = suggestKappa. */
int ipcgpu_opt_set_kappa(ipcgpu_ctx*, double kappa);
/* `tuning` entry 2 (relative, like dHat): the dHat homotopy of fullyImplicit_IP.  Every time step starts at dHat; after a converged
 * sub-problem whose largest active distance is not below the target, ipcgpu_opt_next_subproblem halves dHat (not below the
 * target), rebuilds the constraint sets and re-initialises kappa (Optimizer.cpp:283-289, 1706-1713, 1763-1774).  <= 0: target =
 * dHat, no homotopy (the default, and what `dHat x` / a 6-entry `tuning` with equal entries 1 and 2 mean). */
int ipcgpu_opt_set_dhat_target(ipcgpu_ctx*, double dHatTargetEps);
/* After ipcgpu_opt_newton_iter reported convergence: the tail of the fullyImplicit_IP loop body (Optimizer.cpp:1617-1790) --
 * refresh the lagged multipliers / tangent bases, test tangent-space convergence.  *more = 1: another solveSub_IP pass has
 * started (keep calling newton_iter); 0: the time step is done.  Without friction it returns 0 and changes nothing. */
int ipcgpu_opt_next_subproblem(ipcgpu_ctx*, int* more);
/* scalars4 = {fricDHat (eps_v^2 h^2, < 0: off), #lagged self-contact constraints, friction iteration, #lagged half-space
 * vertices}; lambda (nullable) receives MMLambda_lastH */
int ipcgpu_opt_get_friction_state(ipcgpu_ctx*, double* scalars4, double* lambda);
/* building blocks over the lagged self-contact set.  friction_update lags the CURRENT constraint set (ipcgpu_contact_build /
 * _set) at the current positions: multipliers (Optimizer.cpp:1586-1591), computeDistCoordAndTanBasis (:2481-2527).
 * Vt_colmajor = positions at the beginning of the time step (result.V_prev). */
int ipcgpu_friction_update(ipcgpu_ctx*, double dHat, double kappa, int* nLagged);
int ipcgpu_friction_get(ipcgpu_ctx*, double* lambda_n, double* coord_2n, double* basis_6n);
int ipcgpu_friction_energy(ipcgpu_ctx*, const double* Vt_colmajor, double eps2, double coef, double* energy);
int ipcgpu_friction_gradient_add(ipcgpu_ctx*, const double* Vt_colmajor, double eps2, double coef, double* grad_3nV_inout);
int ipcgpu_friction_hessian_add(ipcgpu_ctx*, const double* Vt_colmajor, double eps2, double coef, int projectDBC);
/* overwrite Optimizer::velocity (xyz-interleaved) and recompute xTilta (computeXTilta, Optimizer.cpp:1236-1257): the
 * `initVel` script keyword (Config.cpp:247-262) */
int ipcgpu_opt_set_velocity(ipcgpu_ctx*, const double* vel_3nV);
/* Config `timeIntegration BE | NM beta gamma` (src/Config.cpp:112-118, defaults beta = 0.25, gamma = 0.5 src/Config.hpp:96):
 * type 0 = backward Euler, 1 = Newmark.  Newmark scales the elastic terms by dt^2 beta (Optimizer.cpp:3216-3224, 3427-3434,
 * 3627-3631), predicts xTilta with the stored acceleration (:1259-1277) and updates velocity / acceleration at the end of the
 * time step (:582-590).  Call after ipcgpu_opt_init, before ipcgpu_opt_precompute; the acceleration starts at zero (:177). */
int ipcgpu_opt_set_time_integration(ipcgpu_ctx*, int type, double beta, double gamma);
/* Config `warmStart n` -> Optimizer::initX(n) (Optimizer.cpp:925-1215): first iterate of every time step.  0 = the last
   configuration (default), 1 explicit Euler, 2 xHat, 3 symplectic Euler, 4 uniformly accelerated motion, 5 the Jacobi guess -g_i / H_ii
   (gradient with projected, matrix with unprojected Dirichlet rows, :1082-1110); the step is cut by the
   inversion filter, the half-space bounds and a full CCD pass, then halved while the mesh is inverted or intersecting.
   *last_step (nullable) receives the fraction of the predicted displacement the last begin_timestep could take. */
int ipcgpu_opt_set_warm_start(ipcgpu_ctx*, int option);
int ipcgpu_opt_get_warm_step(ipcgpu_ctx*, double* last_step);
/* One Mesh::DirichletBCs entry (src/Mesh.hpp:23-39; `DBC bboxMin bboxMax linVel angVel [t0 t1]` on a shape line,
 * src/Config.cpp:246-263, vertices picked by IglUtils::Init_Dirichlet) or the scripted linear / angular velocity of a whole
 * component (`linearVelocity` / `angularVelocity`, componentLVels / componentAVels -- how kinematic mesh obstacles move):
 * while t0 <= stepStartTime < t1 the vertices are Dirichlet nodes (ZERO if both velocities vanish, else NONZERO,
 * AnimScripter.cpp:58-110) and every time step moves them by R (x - c) + c + linVel dt - x with R = Rx Ry Rz of ang_vel dt and
 * c the centre of their current bounding box (AnimScripter.cpp:1413-1462).  ang_vel in rad/s (the script gives deg/s).
 * Call after ipcgpu_opt_init and after the static ipcgpu_set_dbc / ipcgpu_opt_set_twist calls. */
int ipcgpu_opt_add_dirichlet(ipcgpu_ctx*, int n, const int* vert_ids, const double* lin_vel3, const double* ang_vel3, double t0, double t1);
/* Ends group `group` (0-based, in the order of the ipcgpu_opt_add_dirichlet calls) at time t_end: from the time step that starts at
 * t_end on its vertices are free again.  This is what the state-dependent scripts do with mesh.resetDBCVertices() inside
 * AnimScripter::stepAnimScript -- e.g. `script dragright` lets go of the handle once the body has been pulled past the
 * obstacles (AnimScripter.cpp:1619-1632); the condition is the caller's. */
int ipcgpu_opt_end_dirichlet(ipcgpu_ctx*, int group, double t_end);
/* The hard-coded scripted motions of AnimScripter::stepAnimScript that move whole components by a rule evaluated on the current state
 * (`script DCOSquash / DCOSquash6 / DCOSqueezeOut / DCORotCylinders / DCOVerschoorRoller`, AnimScripter.cpp:1060-1300 set-up, :1961-2135
 * per step): the caller evaluates the rule before a time step and hands the group's motion for that step over.  center3 != NULL: the
 * rotation turns about this fixed point (MCORotCenter, the component's bounding-box centre at set-up) instead of the centre of the
 * group's current bounding box; force_nonzero: the nodes are NONZERO Dirichlet nodes even while their velocity is zero, as those
 * scripts type them (it decides whether they are released with the others when a scripted move is cut short, Optimizer.cpp:2168-2203). */
int ipcgpu_opt_set_dirichlet_motion(ipcgpu_ctx*, int group, const double* lin_vel3, const double* ang_vel3, const double* center3 /*nullable*/,
    int force_nonzero);
/* Mesh-sequence motion of a Dirichlet group (`meshSeq <folder>` behind a shape, Config.cpp:284-289; AnimScripter.cpp:1465-1532): before
   every time step the reference reads <folder>/<step>.{msh,obj,seg,pt} and makes `file position - current position` the move of the
   component's nodes, overriding its velocities; the move is then bounded by CCD and the intersection check like any scripted motion
   (:2162-2250).  targets_3n = the file's positions (node order of the group, xyz interleaved), handed over before each step; NULL ends
   the sequence.  The nodes keep the type their velocities give them (ZERO for a codimensional component that only follows a sequence). */
int ipcgpu_opt_set_dirichlet_targets(ipcgpu_ctx*, int group, int n, const double* targets_3n);
/* One Mesh::NeumannBCs entry (src/Mesh.hpp:47-56; `NBC bboxMin bboxMax force [t0 t1]` on a shape line, src/Config.cpp:264-280):
 * while t0 <= stepStartTime < t1 every listed vertex that is not a Dirichlet node feels the acceleration `accel3` -- the
 * incremental potential gets -dt^2 m_v accel . x_v, the gradient -dt^2 m_v accel (Optimizer.cpp:3241-3250, 3452-3461). */
int ipcgpu_opt_add_neumann(ipcgpu_ctx*, int n, const int* vert_ids, const double* accel3, double t0, double t1);
/* State of the augmented-Lagrangian Dirichlet fallback (Optimizer.cpp:1826-1828, 2168-2203; AnimScripter.cpp:2280-2350): when
 * the scripted motion of a time step is cut short (element inversion, CCD, intersection), the NONZERO Dirichlet nodes are
 * released and pulled to their targets by a penalty rho_DBC / 2 m |x - target|^2 with multipliers until the completed step
 * size exceeds 1 - 1e-3.  out4 = {completed step size, rho_DBC, m_projectDBC, number of target positions}. */
int ipcgpu_opt_get_dbc_state(ipcgpu_ctx*, double* out4);
/* Optimizer::velocity (xyz-interleaved), acceleration and dx_Elastic = V - xTilta of the last finished time step
 * (Optimizer.cpp:574-586); any pointer may be null */
int ipcgpu_opt_get_kinematics(ipcgpu_ctx*, double* vel_3nV, double* acc_3nV, double* dx_elastic_3nV);
/* The system report, Optimizer::computeSystemEnergy (Optimizer.cpp:3746-3778; written to sysE.txt / sysM.txt / sysL.txt after precompute, :488-506, and
 * after every time step, :1497-1512, 1801-1816), reduced on the device.  Per mesh component c with nodes [v0, v1) and elements [t0, t1):
 *   sysE[c] = sum_t vol_t psi(F_t) + sum_v m_v (|x_v - xprev_v|^2 / (2 dt^2) - g . x_v)
 *   sysM[c] = sum_v p_v,  p_v = m_v (x_v - xprev_v) / dt          sysL[c] = sum_v x_v x p_v
 * psi: the configured energy (the per-element values of ipcgpu_elastic_energy_per_elem), m_v: the lumped mass (ipcgpu_get_features), g: the gravity of
 * ipcgpu_opt_init, xprev: the positions the last finished time step started from (result.V_prev at the reference's call sites; equal to x after
 * ipcgpu_opt_init / ipcgpu_opt_precompute / ipcgpu_opt_load_status, where the kinetic part and the momenta are exactly zero).  Every node of a range
 * counts (Dirichlet, obstacle and codimensional nodes too).  fp64, no atomics, a fixed summation order: the same state gives the same bits.
 * ipcgpu_opt_set_components: the accumulated ends of the components as the reference keeps them (compVAccSize / compFAccSize, main.cpp:91-92,
 * 1111-1112): non-decreasing, the last ones equal to nV / nT (else IPCGPU_ERR_ARG); empty ranges are legal.  Call after ipcgpu_set_mesh (which goes
 * back to the default: one component, the whole mesh).
 * ipcgpu_opt_system_report: sysE[nComp], sysM / sysL[3 nComp] component-major, xyz interleaved; any pointer may be null.  After ipcgpu_opt_init
 * (before: IPCGPU_ERR_STATE); changes no state.  On a sharded context (ipcgpu_ctx_set_shard, world > 1): IPCGPU_ERR_UNSUPPORTED. */
int ipcgpu_opt_set_components(ipcgpu_ctx*, int nComp, const int* nodeEnd_nComp, const int* tetEnd_nComp);
int ipcgpu_opt_system_report(ipcgpu_ctx*, double* sysE_nComp, double* sysM_3nComp, double* sysL_3nComp);
/* Optimizer::saveStatus (Optimizer.cpp:2964-3011) and the `restart <status file>` branch of the Optimizer constructor
 * (Optimizer.cpp:179-248, Config.cpp:513-516): the reference's text checkpoint (timestep / position / velocity / acceleration /
 * dx_Elastic), written with 20 significant digits so that doubles round-trip; files are interchangeable with the reference's.
 * Load after ipcgpu_opt_init (and ipcgpu_opt_set_time_integration), before ipcgpu_opt_precompute. */
int ipcgpu_opt_save_status(ipcgpu_ctx*, const char* path);
int ipcgpu_opt_load_status(ipcgpu_ctx*, const char* path);
/* counts6 = {#active, #paraEE, #CCD candidates, #half-space constraints, #full CCD passes, #pattern changes}; pair2 = limiting CCD pair of the
 * last iteration ((-svI-1, sfI) or (eI, eJ), (0,0) if none) */
int ipcgpu_opt_get_contact_state(ipcgpu_ctx*, int* counts6, int* pair2);
int ipcgpu_opt_precompute(ipcgpu_ctx*); /* precompute, Optimizer.cpp:457-507 */
int ipcgpu_opt_begin_timestep(ipcgpu_ctx*); /* solve(): stepAnimScript + fullyImplicit_IP head */
/* one pass of the solveSub_IP loop (Optimizer.cpp:1829-2204) == one "Newton iteration" of the
 * metric; *converged = 1 when the convergence test fired before any work was done */
int ipcgpu_opt_newton_iter(ipcgpu_ctx*, int* converged);
int ipcgpu_opt_end_timestep(ipcgpu_ctx*); /* BE velocity + xTilta update, Optimizer.cpp:570-580 */
int ipcgpu_opt_solve_timestep(ipcgpu_ctx*, int maxIter, int* nIter); /* Optimizer::solve(1) */
/* state readers (any pointer may be NULL); scalars8 = {lastEnergyVal, lastStepSize, targetGRes,
 * innerIterAmt, timestep, alphaFeasible, kappa, dHat} */
int ipcgpu_opt_get_state(ipcgpu_ctx*, double* V_colmajor, double* searchDir_3nV, double* gradient_3nV, double* scalars8);
/* timer_step buckets in seconds (src/main.cpp:1326-1340): 0 matrixComputation .. 14 computeConstraintSets */
int ipcgpu_opt_get_timers(ipcgpu_ctx*, double* t16);
/* multi-GPU: the caller-supplied reduction hook used by the optimizer for sharded assembly.
 * fn(user, buf_dev, count, op) must all-reduce `count` doubles in device memory in place
 * (op 0 = sum, 1 = min).  bench.py binds it to torch.distributed (RCCL). */
typedef int (*ipcgpu_allreduce_fn)(void* user, void* buf_dev, long long count, int op);
int ipcgpu_opt_set_allreduce(ipcgpu_ctx*, ipcgpu_allreduce_fn fn, void* user);
/* Stream-ordered variant, and the one a C / C++ caller uses: fn enqueues the all-reduce on the HIP stream it is handed (the
 * context's own) and returns -- `ncclAllReduce(buf, buf, count, ncclDouble, op ? ncclMin : ncclSum, comm, stream)` is the whole body.
 * The library then never synchronises with the host around a collective.  include/adapters/ipcgpu_rccl.cpp is that hook on RCCL
 * (libipcgpu_rccl.so: ipcgpu_rccl_unique_id / ipcgpu_rccl_attach); takes precedence over ipcgpu_opt_set_allreduce. */
typedef int (*ipcgpu_allreduce_stream_fn)(void* user, void* buf_dev, long long count, int op, void* hip_stream);
int ipcgpu_opt_set_allreduce_stream(ipcgpu_ctx*, ipcgpu_allreduce_stream_fn fn, void* user);
/* Point-to-point exchange of the sharded direct solver (round 5; ipcgpu_linsys_set_shard).  A front above the cut of the assembly tree is executed by
 * ONE rank; the packed update matrix of a child that another rank computed (factorisation), its update vector (forward sweep) and the solution entries
 * of an ancestor (backward sweep) go from the rank that has them to exactly the ranks that need them.  One call = ONE group of operations between which
 * no order may be assumed (ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd; torch.distributed.batch_isend_irecv): op i moves `count` doubles of the
 * device buffer `buf_dev` to (send = 1) or from (send = 0) rank `peer`; several operations between one pair of ranks match in the order given.
 * Host-ordered variant: the library drains its stream before the call and expects the data in place when it returns.  Stream variant: the hook
 * enqueues on the stream it is handed (include/adapters/ipcgpu_rccl.cpp); takes precedence.  Set one of them before ipcgpu_linsys_set_shard with
 * world_size > 1.  (The all-reduce hooks above stay in use for scalars, the nodal gradient, the pivot flag and the solution vector.) */
typedef struct ipcgpu_p2p_op {
    void* buf_dev;
    long long count;
    int peer;
    int send;
} ipcgpu_p2p_op;
typedef int (*ipcgpu_exchange_fn)(void* user, int n_ops, const ipcgpu_p2p_op* ops);
typedef int (*ipcgpu_exchange_stream_fn)(void* user, int n_ops, const ipcgpu_p2p_op* ops, void* hip_stream);
int ipcgpu_opt_set_exchange(ipcgpu_ctx*, ipcgpu_exchange_fn fn, void* user);
int ipcgpu_opt_set_exchange_stream(ipcgpu_ctx*, ipcgpu_exchange_stream_fn fn, void* user);
int ipcgpu_ctx_get_stream(ipcgpu_ctx*, void** hip_stream);

/* ---- measurement -------------------------------------------------------------------- */
/* Launch the fused element-assembly kernel `reps` times on the context stream and return the
 * average duration per launch measured with HIP events on that stream, plus the algorithmic
 * bytes of one launch (112 nT + 84 nV + 8 nnz). */
int ipcgpu_bench_assembly(ipcgpu_ctx*, double dtSq, int reps, double* avg_ms, double* algorithmic_bytes);
/* same for one numeric factorisation + solve */
int ipcgpu_bench_factor_solve(ipcgpu_ctx*, int reps, double* factor_ms, double* solve_ms);
/* device streaming copy bandwidth (GB/s) measured here, the "STREAM" figure quoted beside the
 * nominal 8 TB/s */
/* average time of one launch of the iterative solver's product (ipcgpu_linsys_multiply_sym) on device-resident vectors and its algorithmic bytes:
 * 8 nnz values + 4 nnz columns + the two vectors, each once */
int ipcgpu_bench_multiply_sym(ipcgpu_ctx*, int reps, double* avg_ms, double* algorithmic_bytes);
int ipcgpu_bench_stream(ipcgpu_ctx*, long long bytes, int reps, double* gbps);

#ifdef __cplusplus
}
#endif
#endif
