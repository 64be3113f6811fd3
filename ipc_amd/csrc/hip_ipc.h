// Host-side mirror of the three reference interfaces on the hot path, with their state resident in HBM:
//   HipMesh          <- Mesh<3>                       (src/Mesh.hpp:58-171)
//   HipLinSysSolver  <- LinSysSolver<VectorXi,VectorXd> (src/LinSysSolver/LinSysSolver.hpp:31-467)
//   HipNeoHookean    <- Energy<3>/NeoHookeanEnergy<3>  (src/Energy/Energy.hpp:27-138)
//   HipOptimizer     <- Optimizer<3>                   (src/TimeStepper/Optimizer.hpp:28-283)
// Method names and argument meaning follow the reference so that the adapters in INTEGRATION.md are
// one-line forwards.  Everything here is reached through the C ABI of include/ipcgpu.h.
#pragma once
#include "common.h"
#include "aero_kernels.h"
#include "aero_plan.h"
#include "attach_kernels.h"
#include "attach_plan.h"
#include "chamber_kernels.h"
#include "chamber_plan.h"
#include "contact_pattern.h"
#include "fiber_kernels.h"
#include "fiber_plan.h"
#include "mf_numeric.h"
#include "mf_symbolic.h"
#include "nh_kernels.h"
#include "patch_assembly.h"
#include "hip_contact.h"
#include "hip_halfspace.h"
#include "round_collider_kernels.h"
#include "pcg.h"
#include "pcg_coarse.h"
#include "plastic_kernels.h"
#include "plastic_plan.h"
#include "report_plan.h"
#include "rod_kernels.h"
#include "rod_plan.h"
#include "scalar_slots.h"
#include "shell_kernels.h"
#include "shell_limit_kernels.h"
#include "shell_limit_plan.h"
#include "shell_plan.h"
#include "shell_plastic_kernels.h"
#include "shell_plastic_plan.h"
#include "shell_rubber_kernels.h"
#include "shell_rubber_plan.h"
#include "shell_weave_kernels.h"
#include "shell_weave_plan.h"
#include "stress_plan.h"
#include <map>
#include <memory>
#include <string>

struct ipcgpu_ctx; // opaque C handle
typedef int (*ipcgpu_allreduce_fn_t)(void* user, void* buf_dev, long long count, int op);
typedef int (*ipcgpu_allreduce_stream_fn_t)(void* user, void* buf_dev, long long count, int op, void* hipStream);

namespace ipcgpu {

// Plastic flow of the shell (ipcgpu_shell_set_plasticity; shell_plastic_kernels.h): the host plan and the device state.  plan.nTri == 0: never set, and then
// nothing below is allocated or read.  on(): some triangle has a finite yield strain or some hinge flows -- only then does the stepper launch a flow and
// does saveStatus write the section.  While allocated, rows 0-3 of d_triConst and row 0 of d_hingeConst (HipShell) are the truth about the rest shape.
struct HipShellPlastic {
    ShellPlasticPlan plan;
    DevBuf<double> d_yield, d_creep, d_harden, d_alpha; // nTri
    DevBuf<double> d_hYield, d_hCreep, d_hHarden, d_hG, d_alphaB; // nHinge
    DevBuf<double> d_hA; // nTri rest volumes h A
    DevBuf<double> d_B0, d_thetaBar0; // SoA [4][nTri], nHinge: the records as they were at the first call (ipcgpu_shell_plastic_reset puts them back)
    DevBuf<int> d_count; // SPC_COUNT (scalar_slots.h)
    DevBuf<double> d_totals, d_partial, d_stateTri, d_stateHinge; // SPT_COUNT; ipcgpu_shell_plastic_state's scratch
    bool allocated() const { return plan.nTri > 0; }
    bool on() const { return plan.nOn > 0 || plan.nHingeOn > 0; }
    void drop() { plan = ShellPlasticPlan(); }
};

// Elastic shell of the mesh (ipcgpu_set_shell): the host plan and its device copy.  nTri() == 0: no shell, and then nothing below is ever read.
struct HipShell {
    ShellPlan plan;
    double bendScale = 1.0;
    // what the shell replaced, put back when it is removed or replaced: the masses its nodes had before (codimensional area masses, or 0) and avgEdgeLen
    std::vector<double> massBefore;
    double avgEdgeLenBefore = 0.0;
    DevBuf<int> d_tri;
    DevBuf<int4> d_hinge;
    DevBuf<double> d_triConst, d_hingeConst;
    int nTri() const { return plan.nTri; }
    int nHinge() const { return plan.nHinge; }
    // strain limit (ipcgpu_shell_set_strain_limit; shell_limit_plan.h): arrays of its own beside the shell's.  nLimited() == 0: no limit, and then none of
    // the limit kernels is launched.  unchecked: set where the stepper cannot know from its last energy whether the state is feasible (a new limit,
    // positions written from outside): the next time step then asks the device once
    ShellLimitPlan limit;
    DevBuf<int> d_limTri;
    DevBuf<double> d_limConst, d_triLimit, d_stretchPartial, d_stretchOut;
    bool limitUnchecked = false;
    int nLimited() const { return limit.nLimited; }
    // rubber membrane (ipcgpu_shell_set_membrane; shell_rubber_plan.h): arrays of its own beside the shell's.  nRubber() == 0: every triangle is StVK, none of
    // the rubber kernels is launched and d_triConst is the plan's triConst; otherwise d_triConst holds zeros for the two StVK constants of the rubber
    // triangles.  unchecked: as limitUnchecked, for "a rubber triangle is degenerate" (its energy is +infinity)
    ShellRubberPlan rubber;
    DevBuf<int> d_rubTri;
    DevBuf<double> d_rubConst, d_rubCount;
    bool rubberUnchecked = false;
    int nRubber() const { return rubber.nRubber; }
    // woven cloth (ipcgpu_shell_set_weave; shell_weave_plan.h): arrays of its own beside the shell's.  nWoven() == 0: no triangle is woven, none of the weave
    // kernels is launched, d_triConst holds no zeros of this term and row 1 of d_hingeConst is the plan's bendScale k_b w_e; otherwise d_triConst holds zeros
    // for the two StVK constants of the woven triangles and row 1 of d_hingeConst carries the plan's hinge factors
    ShellWeavePlan weave;
    DevBuf<int> d_wovTri;
    DevBuf<double> d_wovConst;
    int nWoven() const { return weave.nWoven; }
    HipShellPlastic plastic; // (its own struct above)
};

// Elastic rod of the mesh (ipcgpu_set_rod): the host plan and its device copy.  nSeg() == 0: no rod, and then nothing below is ever read.
struct HipRod {
    RodPlan plan;
    double bendScale = 1.0;
    // what the rod replaced, put back when it is removed or replaced: the masses its nodes had before (the reference's segment masses, or 0) and avgEdgeLen
    std::vector<double> massBefore;
    double avgEdgeLenBefore = 0.0;
    bool ownsAvgEdgeLen = false;
    DevBuf<int2> d_seg;
    DevBuf<int> d_bend;
    DevBuf<double> d_segConst, d_bendConst;
    int nSeg() const { return plan.nSeg; }
    int nBend() const { return plan.nBend; }
    int nBendActive() const { return bendScale > 0.0 ? plan.nBend : 0; } // `bend 0` switches bending off: no triple reaches the kernels
};

// Attachments of the mesh (ipcgpu_set_attachments): the host plan and its device copy.  n() == 0: none, and then nothing below is ever read.
struct HipAttach {
    AttachPlan plan;
    DevBuf<int> d_node;
    DevBuf<double> d_coef, d_kL;
    // vNeighbor as it was before this set's pairs joined it, and HipMesh::nbVersion right after they did (setAttachments)
    std::vector<int> nbPtrBefore, nbBefore;
    unsigned nbVersionAfter = 0;
    int n() const { return plan.n; }
};

// Pressure chambers of the mesh (ipcgpu_set_chambers): the host plan and its device copy.  n() == 0: none, and then nothing below is ever read.
struct HipChamber {
    ChamberPlan plan; // plan.pressure is the host copy of the pressures (ipcgpu_chamber_set_pressure keeps it current)
    DevBuf<int> d_tri, d_chamberOf, d_triEnd;
    DevBuf<double> d_pressure, d_ref; // d_ref: r_c, the rest value until the first time step refreshes it (chamber_kernels.h)
    // vNeighbor as it was before this set's pairs joined it, and HipMesh::nbVersion right after they did (setChambers)
    std::vector<int> nbPtrBefore, nbBefore;
    unsigned nbVersionAfter = 0;
    int n() const { return plan.n; }
    int nTri() const { return plan.nTri; }
    // The gas law (ipcgpu_chamber_set_gas; chamber_kernels.h).  nGas() == 0: every chamber is constant, nothing below is allocated or read, and the launches
    // are those of a context that never heard of the gas law.  Otherwise the kernels read TWO pressure arrays in place of d_pressure (which keeps p_c):
    //   d_pConst  p_c of the constant chambers and 0 for the gas chambers: what the per-triangle energy kernel multiplies the volume with
    //   d_pEff    the effective pressure the assemble kernel reads: p_c of the constant chambers, gauge(V_c) of the gas chambers as the last gas update left it
    ChamberGas gas;
    DevBuf<int> d_sliceBegin, d_sliceEnd, d_sliceOff, d_gasChamber, d_isGas;
    DevBuf<double> d_pConst, d_pEff, d_gasParam, d_slicePartial, d_gasState, d_gasSelect; // d_gasSelect: nGas rows of n doubles, row g is 1 at gasChamber[g]
    int nGas() const { return gas.nGas; }
    ChamberGasView gasView() const
    {
        return ChamberGasView{ gas.nGas, gas.nSlice(), d_sliceBegin.p, d_sliceEnd.p, d_sliceOff.p, d_gasChamber.p, d_gasParam.p, d_pressure.p, d_slicePartial.p, d_pEff.p, d_gasState.p };
    }
};

// Aerodynamic surfaces of the mesh (ipcgpu_set_aero): the host plan and its device copy.  n() == 0: none, and then nothing below is ever read.
struct HipAero {
    AeroPlan plan;
    DevBuf<int> d_tri, d_surfOf;
    DevBuf<double> d_coef, d_lagged; // d_lagged: the lagged records, the rest values until the first time step refreshes them (aero_kernels.h)
    DevBuf<double> d_statePartial, d_stateOut, d_force; // ipcgpu_aero_state
    double wind[3] = { 0.0, 0.0, 0.0 }, density = 1.225; // ipcgpu_aero_set_wind; back to these defaults when the surfaces are removed
    // vNeighbor as it was before this set's pairs joined it, and HipMesh::nbVersion right after they did (setAero)
    std::vector<int> nbPtrBefore, nbBefore;
    unsigned nbVersionAfter = 0;
    int n() const { return plan.n; }
    int nTri() const { return plan.nTri; }
    void drop()
    {
        plan = AeroPlan();
        wind[0] = wind[1] = wind[2] = 0.0;
        density = 1.225;
    }
};

// Plastic flow of the tetrahedral elements (ipcgpu_set_plasticity; plastic_kernels.h): the host plan and the device state.  plan.nT == 0: never set, and
// then nothing below is allocated or read.  on(): some element has a finite yield strain -- only then does the stepper launch the flow and does
// saveStatus write the section.  While allocated, d_A (HipMesh) is the truth and the host copy HipMesh::restTriInv may be stale.
struct HipPlastic {
    PlasticPlan plan;
    DevBuf<double> d_yield, d_creep, d_harden, d_alpha;
    DevBuf<double> d_A0; // restTriInv as it was when plasticity was first set (ipcgpu_plastic_reset puts it back), SoA [9][nT]
    DevBuf<int> d_count; // PC_COUNT (scalar_slots.h)
    DevBuf<double> d_totals, d_partial, d_state; // PT_COUNT; ipcgpu_plastic_state's scratch
    bool allocated() const { return plan.nT > 0; }
    bool on() const { return plan.nOn > 0; }
    void drop() { plan = PlasticPlan(); }
};

// Fibre reinforcement of the tetrahedral elements (ipcgpu_set_fibers; fiber_kernels.h): the host plan and its device copy.  n() == 0: no fibred element,
// and then nothing below is ever read and the stepper launches nothing.
struct HipFiber {
    FiberPlan plan;
    DevBuf<int> d_fibTet, d_flags, d_groupOf;
    DevBuf<double> d_b, d_volK, d_k2, d_l0;
    DevBuf<double> d_state, d_partial, d_totals; // ipcgpu_fiber_state's scratch
    int n() const { return plan.nF; }
    void drop() { plan = FiberPlan(); }
};

class HipMesh {
public:
    int nV = 0, nT = 0;
    int nElemNodes = 0; // nodes referenced by at least one element (mean nodal mass, bounding box)
    std::vector<double> V_rest; // column-major nV x 3
    std::vector<int> F; // column-major nT x 4
    std::vector<double> restTriInv; // SoA [9][nT]
    std::vector<double> triArea, mass, mu, lam;
    std::vector<int> dbcType;
    std::vector<int> nbPtr, nb; // vNeighbor as sorted CSR adjacency (Mesh.cpp:470-493)
    unsigned nbVersion = 0; // bumped by everything that rebuilds or extends vNeighbor
    double avgEdgeLen = 0, bboxDiag2 = 0, bboxLo[3] = { 0, 0, 0 }, bboxHi[3] = { 0, 0, 0 };
    // device
    DevBuf<double> d_x, d_xTilde, d_mass, d_A, d_vol, d_mu, d_lam;
    DevBuf<int> d_dbc;
    DevBuf<int4> d_tet;

    // Mesh::computeFeatures + computeMassMatrix + setLameParam (Mesh.cpp:414-527, 246-266, 399-401, 660-671)
    unsigned featuresVersion = 0; // bumped by every computeFeatures: host-side caches of mesh topology key on it
    void computeFeatures(int nV, int nT, const double* Vrest, const int* F, double YM, double PR, double density, hipStream_t s);
    // surface-only nodes that belong to the mesh (triangle meshes under `shapes`, componentCoDim 2): they count in the bounding box
    // and the mean nodal mass and carry the given lumped masses (Mesh.cpp:310-345)
    std::vector<char> inMesh; // per node: referenced by an element (the components of codimension 3)
    void addSurfaceEdges(int nSF, const int* SF_colmajor, int nCE = 0, const int* CE_pairs = nullptr);
    void setCodimNodes(int n, const int* ids, const double* nodeMass, hipStream_t s);
    // Elastic shell on triangle components (shell_plan.h): validates, sets the lumped masses of the shell nodes, marks them as element nodes (bounding box,
    // mean nodal mass), adds the plan's node pairs to vNeighbor and uploads the constants.  nTri = 0 removes the shell, a second call replaces it: the nodes
    // of the old shell get back the masses they had before it (ipcgpu_set_codim_nodes' or 0) and lose the mark; the neighbour pairs stay.  With no tetrahedron
    // in the mesh avgEdgeLen is the mean side of the shell triangles while a shell is set.
    HipShell shell;
    void setShell(int nTri, const int* tri_colmajor, const double* thickness, const double* YM, const double* PR, const double* rho, double bendScale, hipStream_t s);
    // Strain limit of the shell (shell_limit_plan.h): validates and uploads the compact list and the constants.  All limits zero (or null) removes it;
    // setShell and computeFeatures drop it.  Changes no mass and adds no neighbour pair (the blocks are the membrane's).
    void setShellStrainLimit(const double* limit, const double* onset, const double* stiff, hipStream_t s);
    // Membrane model of the shell's triangles (shell_rubber_plan.h): validates, uploads the compact list of the rubber triangles with their constants, and the
    // shell's triConst with the StVK constants of those triangles zeroed (the plan's own where none is rubber).  All models zero (or null) removes the term;
    // setShell and computeFeatures drop it.  Changes no mass and adds no neighbour pair (the blocks are the membrane's).
    void setShellMembrane(const int* model, const double* alpha, hipStream_t s);
    // Woven cloth of the shell's triangles (shell_weave_plan.h): validates, uploads the compact list of the woven triangles with their constants, the shell's
    // triConst with the StVK constants of those triangles zeroed, and row 1 of hingeConst times the plan's hinge factors (both the shell plan's own once no
    // triangle is woven).  All selectors zero (or null) removes the term; setShell and computeFeatures drop it.  Changes no mass and adds no neighbour pair.
    void setShellWeave(const int* woven, const double* dir, const double* E1, const double* E2, const double* G12, const double* nu12, const double* bendWarp,
        const double* bendWeft, hipStream_t s);
    void uploadShellTriConst(hipStream_t s); // rows 4 and 5 of d_triConst from the shell plan, zeroed where the rubber or the weave plan says so; rows 0-3 kept where they may have flowed
    // Plastic flow of the shell (shell_plastic_plan.h): validates, uploads the parameter arrays; the first call allocates alpha = alphaB = 0 and keeps the
    // copies B0 and thetaBar0 of the device records.  Touches no mass, no neighbour pair and no pattern; setShell and computeFeatures drop it.
    void setShellPlasticity(int triBegin, int triEnd, double yield, double bendYield, double creep, double harden, hipStream_t s);
    void ensureShellPlastic(hipStream_t s); // the state arrays with everything elastic, unless they exist (loadStatus of a file with a shellplastic section)
    void uploadShellPlasticParams(hipStream_t s);
    // Elastic rod on segment components (rod_plan.h): as setShell -- validates, sets the lumped masses of the rod nodes, marks them as element nodes, adds
    // the plan's node pairs to vNeighbor and uploads the constants.  nSeg = 0 removes the rod, a second call replaces it: the nodes of the old rod get back
    // the masses they had before it and lose the mark; the neighbour pairs stay.  With neither a tetrahedron nor a shell in the mesh avgEdgeLen is the mean
    // rest length of the segments while a rod is set.  A rod node may belong to no tetrahedron and no shell triangle (setShell checks the converse).
    HipRod rod;
    // set to 1 by a codimensional Hessian kernel that finds no block for a node pair in the pattern (csr_scatter_device.h); allocated and zeroed
    // with the first shell, rod or attachment set.  The C entry points *_hessian_add read and clear it after their launch; the stepper builds its own pattern and never reads it
    DevBuf<int> d_codimErr;
    // what setShell and setRod share: the nodes of the body that is replaced or removed (null: none) get back massBefore and lose the inMesh mark, massBefore
    // becomes a snapshot of the masses, the new body's nodes take newMass and the mark
    void replaceBodyMasses(const std::vector<char>* oldNodes, std::vector<double>& massBefore, const std::vector<char>& newNodes, const std::vector<double>& newMass);
    void addNeighbourPairs(const std::vector<int>& pairs); // (lo, hi) pairs into vNeighbor, both directions, sorted and unique
    void setRod(int nSeg, const int* seg_colmajor, const double* radius, const double* YM, const double* rho, double bendScale, hipStream_t s);
    // Attachments (attach_plan.h): validates, adds the plan's node pairs to vNeighbor and uploads the stencils.  n = 0 removes them, a second call replaces
    // them (their neighbour pairs leave vNeighbor again unless something else has extended it since); computeFeatures drops them.  Touches no mass and no inMesh mark: an attachment is no body.
    HipAttach attach;
    void setAttachments(int n, const int* nodesA, const double* weightsA, const int* nodesB, const double* weightsB, const double* k, const double* L, hipStream_t s);
    // Pressure chambers (chamber_plan.h): validates, adds the plan's node pairs to vNeighbor and uploads the lists, the pressures and the rest reference
    // points.  nCh = 0 removes them, a second call replaces them (their neighbour pairs leave vNeighbor again unless something else has extended it since);
    // computeFeatures drops them.  Touches no mass and no inMesh mark: a chamber is no body.
    HipChamber chamber;
    void setChambers(int nCh, const int* triEnd, const int* tri_colmajor, const double* pressure, hipStream_t s);
    void setChamberPressure(const double* pressure, hipStream_t s); // finite values only; needs chambers; a gas chamber keeps ambient + pressure > 0
    // The gas law (chamber_plan.h: buildChamberGas): validates, uploads the parameters, the slices and the two pressure arrays.  All isGas == 0 drops it
    // again.  setChambers and computeFeatures drop it too.
    void setChamberGas(const int* isGas, const double* ambient, const double* gamma, const double* fillVolume, hipStream_t s);
    void uploadChamberGasPressures(hipStream_t s); // d_pConst and d_pEff from plan.pressure
    // Aerodynamic surfaces (aero_plan.h): validates, adds the plan's node pairs to vNeighbor and uploads the lists, the coefficients and the rest records.
    // nSurf = 0 removes them, a second call replaces them (their neighbour pairs leave vNeighbor again unless something else has extended it since);
    // computeFeatures drops them.  Touches no mass and no inMesh mark: a load is no body.  Wind and density survive a replacement, not a removal.
    HipAero aero;
    void setAero(int nSurf, const int* triEnd, const int* tri_colmajor, const double* cn, const double* ct, const int* oneSided, hipStream_t s);
    void setAeroWind(const double* wind3, double density); // finite wind, finite density > 0; nothing without surfaces
    // Plastic flow (plastic_plan.h): validates, uploads the three parameter arrays; the first call allocates alpha = 0 and keeps the copy A0 of d_A.
    // Touches no mass, no neighbour pair and no pattern; computeFeatures drops it.
    HipPlastic plastic;
    void setPlasticity(int tetBegin, int tetEnd, double yield, double creep, double harden, hipStream_t s);
    void ensurePlastic(hipStream_t s); // the state arrays with every element elastic, unless they exist (loadStatus of a file with a plastic section)
    void resetPlasticHistory(hipStream_t s); // A0 = the current d_A, alpha = 0 (ipcgpu_set_mesh_features with a restTriInv)
    // Fibre reinforcement (fiber_plan.h): validates, merges the range into the specification, rebuilds the compact lists from the current restTriInv and
    // rest volumes and uploads them.  Refuses a range that holds a plastic element.  Touches no mass, no neighbour pair and no pattern (the six node
    // pairs of a tetrahedron are in every pattern); computeFeatures drops it.
    HipFiber fiber;
    void setFibers(int tetBegin, int tetEnd, const double* dir, bool dirPerElement, double k, int law, double k2, bool tensionOnly, int group, hipStream_t s);
    void setFiberActivation(int group, double act, hipStream_t s); // uploads l0 (FIBER_MAX_GROUPS doubles) and nothing per element
    void uploadFibers(hipStream_t s); // the compact lists again from the current restTriInv and volumes (ipcgpu_set_mesh_features, loadStatus)
    void meshBBox(); // bounding box and node count over inMesh (Mesh::matSpaceBBoxSize2(dim) / avgNodeMass(dim): tetrahedral components only)
    void uploadDBC(hipStream_t s);
    int energyType = 0; // Config `energy NH|FCR` (Config.cpp:23-24): 0 neo-Hookean, 1 fixed corotated; 2 stable neo-Hookean (no counterpart in the reference)
    // Energy::getNeedElemInvSafeGuard(): only NH has a barrier at J = 0; the step filter and the inversion checks of the stepper serve it alone
    bool needElemInvSafeGuard() const { return energyType == 0; }
    double density = 0; // global density handed to computeFeatures (component overrides rescale the nodal mass by rho / density)
    void setComponentMaterial(int nodeBegin, int nodeEnd, int tetBegin, int tetEnd, double rho, double YM, double PR, hipStream_t s);
    bool isDBCVertex(int v) const { return dbcType[v] != 0; }
    bool isProjectDBCVertex(int v, bool projectDBC) const { return dbcType[v] == 1 || (dbcType[v] == 2 && projectDBC); }
};

class HipLinSysSolver {
public:
    explicit HipLinSysSolver(hipStream_t s);
    ~HipLinSysSolver();
    int numRows = 0;
    std::vector<int> ia, ja; // 0-based symmetric-upper CSR (host copy, get_ia / get_ja)
    DevBuf<int> d_ia, d_ja;
    DevBuf<double> d_a;
    DevBuf<double> hostDelta, hostSetVal; // staging of ipcgpu_linsys_apply_host_updates
    DevBuf<unsigned char> hostSetMask;
    // per-node row geometry + per-tet edge slots used by the element kernels
    std::vector<int> rowBase, rowLen;
    DevBuf<int> d_rowBase, d_rowLen, d_edgeP0;
    int solverType = 0;
    int patternVersion = 0; // bumped by every set_pattern*: consumers (patch plan) rebuild lazily
    hipStream_t stream;

    // set_pattern(vNeighbor, fixedVert) (LinSysSolver.hpp:46-150); extra = contact connectivity
    void set_pattern(const HipMesh& mesh, int nExtra, const int* extraPairs);
    void set_pattern_csr(int nRows, const int* ia, const int* ja);
    void buildElementMap(const HipMesh& mesh); // tet edge -> CSR slot
    void setZero();
    int findEntry(int row, int col) const;
    void analyze_pattern(const HipMesh* meshForCoords);
    bool factorize();
    bool solve(const double* rhs_dev, double* x_dev); // false: the iterative solver met p.Ap <= 0 (the exact solvers always return true)
    // factorize + solve, forward sweep overlapped with the factorisation.  negateRhs (multifrontal solver only, solverType 0): solves A x = -rhs, the sign
    // taken in the solver's own pass over the right-hand side
    bool factorizeSolve(const double* rhs_dev, double* x_dev, bool wait = true, bool negateRhs = false);
    bool lastPivotsOk() const; // after factorizeSolve(..., wait = false) and a synchronisation of the stream
    int devicePivotFlag() const { return num_.devicePivotFlag(); } // tests: the multifrontal solver's flag read from device memory (synchronises)
    bool lastSyncOk_ = true;
    void multiply(const double* x_dev, double* y_dev);
    void precondition_diag(const double* in_dev, double* out_dev);
    // Solver type 2: preconditioned CG (the reference's iterative choice, AMGCLSolver.cpp:24-25, 173-241).  precond 0: 3x3 block Jacobi, no symbolic
    // analysis at all; 1: the multifrontal factor of an earlier matrix, kept for up to maxFactorAge factorize() calls; 2: block Jacobi plus the exact solve
    // of a coarse matrix of six rigid-body modes per node aggregate (pcg_coarse.h), rebuilt and factorised by every factorize() (maxFactorAge is ignored).
    double pcgRelTol = 1e-5; // solver.tol, AMGCLSolver.cpp:24
    int pcgMaxIter = 1000; // solver.maxiter, :25
    int pcgPrecond = 0, pcgMaxFactorAge = 1; // (the best of 1, 2, 4, 8, 16 on the headline workload: profiles/pcg_bench.json)
    void setIterative(double relTol, int maxIter, int precond, int maxFactorAge);
    void iterStats(double* out6) const;
    // two-level preconditioner, after analyze_pattern: { aggregates, coarse rows, coarse nnz, coarse factorisations so far, factorize() calls whose coarse
    // matrix was not positive definite (those matrices were served by block Jacobi alone) }
    void coarseStats(double* out5) const;
    bool coarseDims(int* nAgg, int* rows, int* nnz) const; // false: there is no coarse level (another preconditioner, or before analyze_pattern)
    void coarseGet(int* aggOfNode, int* cia, int* cja, double* ca); // the hierarchy as the last analyze_pattern / factorize left it
    void multiplySym(const double* x_dev, double* y_dev); // the atomic-free product of the iterative solver (any solver type)
    int getNumRows() const { return numRows; }
    int getNumNonzeros() const { return (int)ja.size(); }
    const MfSymbolic& symbolic() const { return sym_; }
    // subtree-sharded factorisation / solves over `world` ranks (MfNumeric::setShard); takes effect at the next analyze_pattern
    void setShard(int rank, int world, ipcgpu_allreduce_fn_t fn, void* user, ipcgpu_allreduce_stream_fn_t sfn = nullptr, void* streamUser = nullptr)
    {
        num_.setShard(rank, world, fn, user, sfn, streamUser);
        analyzed_ = false;
    }
    void setHooks(ipcgpu_allreduce_fn_t fn, void* user, ipcgpu_allreduce_stream_fn_t sfn, void* streamUser) { num_.setHooks(fn, user, sfn, streamUser); }
    void setExchangeHooks(MfNumeric::ExchangeFn fn, void* user, MfNumeric::ExchangeStreamFn sfn, void* streamUser) { num_.setExchangeHooks(fn, user, sfn, streamUser); }
    bool hasExchangeHook() const { return num_.hasExchangeHook(); }
    int solverWorld() const { return num_.world(); }
    void setBulkTuning(double minMB, int block) { num_.setBulkTuning(minMB, block); }
    void entryDestinations(long long* out) const { num_.entryDestinations(out, ja.size()); }
    void nodeOwners(std::vector<int>& o) const { num_.nodeOwners(o); }
    long long exchangedBytes() const { return num_.exchangedBytes(); }
    long long exchangeCalls() const { return num_.exchangeCalls(); }
    long long sentBytes() const { return num_.sentBytes(); }
    long long receivedBytes() const { return num_.receivedBytes(); }
    double exchangeWaitMs() { return num_.exchangeWaitMs(); }
    void criticalPath(double* out5) const { num_.criticalPath(out5); }
    int analysisVersion = 0; // bumped by every analyze_pattern (the owner-computes plan of the assembly follows the solver's cut)
    double sharedFlopFraction() const { return num_.sharedFlopFraction(); }
    bool analyzed() const { return analyzed_; }
    void invalidateAnalysis() { analyzed_ = false; } // the solver type changed: what one back end set up is not what another needs

private:
    MfSymbolic sym_;
    MfNumeric num_;
    bool analyzed_ = false;
    std::unique_ptr<struct RocsolverCsrrf> rs_;
    // solver type 2
    PcgPattern pcgPat_;
    PcgWork pcgWork_;
    int pcgPatVersion_ = -1;
    void ensurePcgPattern();
    int runPcg(const double* rhs_dev, double* x_dev, PcgState& out);
    bool haveFactor_ = false, lastConverged_ = true;
    int factorAge_ = 0; // factorize() calls since the factor was computed
    long long nFactorizations_ = 0;
    // two-level preconditioner: the aggregation (rebuilt when the pattern changes), its device copy, and a second solver (multifrontal, same stream) for Ac
    PcgCoarse coarseHost_;
    PcgCoarseDev coarseDev_;
    std::unique_ptr<HipLinSysSolver> coarse_;
    const HipMesh* coarseMesh_ = nullptr; // positions and Dirichlet types are read from it at every factorize()
    int coarseVersion_ = -1;
    bool coarseBuilt_ = false, coarseOk_ = false; // Ac assembled for the current values; its factorisation succeeded
    long long nCoarseFactorizations_ = 0, nCoarseFallbacks_ = 0;
    struct {
        int iterations = 0, syncs = 0, factorAge = 0;
        double residual = 0.0;
        bool converged = false;
    } pcgLast_;
    friend struct RocsolverCsrrf;
};

class HipOptimizer {
public:
    HipOptimizer(HipMesh& mesh, HipLinSysSolver& lin, hipStream_t s);
    void init(double dt, bool withGravity);
    void setRelGL2Tol(double relTol);
    void setParameterScaling(bool absolute, double dTolRel, double kappaMinMultiplier); // useAbsParameters / tuning[3] / kappaMinMultiplier
    void setTwist(int nL, const int* left, int nR, const int* right, double angVel);
    void precompute();
    void beginTimestep();
    bool newtonIter(); // true = converged before doing work
    void endTimestep();
    int solveTimestep(int maxIter);

    // building blocks (virtuals of Optimizer.hpp:229-283)
    double computeEnergyVal();
    void computeGradient(bool projectDBC);
    void penaltyGradientAdd(bool projectDBC);
    void computePrecondMtr(bool projectDBC, bool withGradient); // its three steps follow
    bool patternCoversContact(); // does the solver's pattern hold every block of the current contact sets
    void growPattern(const std::function<void(const char*)>& lap); // new pattern + analysis where ContactPattern asks for them (lap: IPCGPU_PATTERN_TIMES)
    void assembleSystem(bool projectDBC, bool withGradient); // matrix (and gradient) on the current pattern, one sequence for every sharding scheme
    // lagged stiffness-proportional damping (Optimizer.cpp:3381-3400, 3519-3540, 3707-3709, 3723-3735; Config.cpp:141-157, 614-616):
    // D = projected elastic Hessian at the state the last time step ended in, times dampingStiff / dt, on the solver's pattern
    double dampingStiff = 0.0;
    double ctorDt = 0.025; // the step size inside eps_v^2 h^2 and CN_MBC: the reference's constructor leaves its setTime(10, 0.025) in them (hip_optimizer.cpp, top)
    double dHatTargetEps = -1.0; // tuning[2] (Optimizer.cpp:283-289): every time step starts at dHat and halves it down to this; < 0: no homotopy
    double kappaConfig = 0.0; // tuning[0] (Config.cpp:41-45): the barrier stiffness a time step starts from, 0 = suggestKappa
    void setDamping(double stiff);
    void computeDampingMtr(); // at the current positions (precompute, end of a time step)
    void assembleDampingMtr(); // (re)builds the values at the remembered positions on the current pattern
    double dampingEnergy();
    void dampingGradientAdd(bool projectDBC, double* grad_dev);
    void computeSearchDir();
    void enqueueDirNorm();
    void lineSearch(double& stepSize);
    void stepForward(const double* x0_dev, double alpha);
    void stepFeasible(double& stepSize);
    double filterStepSize(const double* p_dev, double stepSize);
    double fullCcd(double slackness, double stepSize); // the full sweep of the search direction in the mode of the contact handler
    bool checkInversion(bool meshQuery = false); // true: no element has det < 0; without meshQuery also whenever the energy has no inversion safeguard
    ElemView view() const;
    // The codimensional terms (shell_kernels.h, shell_rubber_kernels.h, shell_weave_kernels.h, shell_limit_kernels.h, rod_kernels.h, attach_kernels.h, chamber_kernels.h, aero_kernels.h) enter wherever the tetrahedral elastic term does, with the same
    // coefficient, through the two members below and nowhere else.  Both walk the terms in the fixed order shell, rubber, weave, limit, rod, attachments, chambers, air drag (the energy sum
    // is ((((((((E + shell) + rubber) + weave) + limit) + rod) + attach) + chamber) + aero) + fiber) and launch a term only where the mesh has it (nTri(), nRubber(), nWoven(), nLimited(), nSeg(), attach.n(), chamber.nTri(), aero.nTri(), fiber.n()); none of them is ever sharded.
    // CODIM_STIFFNESS: the terms that enter the lagged stiffness damping -- a pressure load is no stiffness, and neither is air drag; the fibre term is one.
    enum : unsigned {
        CODIM_SHELL = 1, CODIM_SHELL_LIMIT = 2, CODIM_ROD = 4, CODIM_ATTACH = 8, CODIM_CHAMBER = 16, CODIM_SHELL_RUBBER = 32, CODIM_AERO = 64, CODIM_FIBER = 128, CODIM_SHELL_WEAVE = 256, CODIM_ALL = 511,
        CODIM_STIFFNESS = CODIM_ALL & ~CODIM_CHAMBER & ~CODIM_AERO
    };
    CodimBase codimBase(const double* x_dev) const;
    ShellView shellView(const double* x_dev) const;
    ShellLimitView shellLimitView(const double* x_dev) const;
    ShellRubberView shellRubberView(const double* x_dev) const;
    ShellWeaveView shellWeaveView(const double* x_dev) const;
    RodView rodView(const double* x_dev) const;
    AttachView attachView(const double* x_dev) const;
    FiberView fiberView(const double* x_dev) const;
    // pressure: which array the kernels read as the pressure -- d_pressure without a gas chamber, whatever is asked; with one, the effective pressure
    // (CHAMBER_P_EFFECTIVE, what the assembly wants) or the constant chambers' alone (CHAMBER_P_CONSTANT, what the per-triangle energy wants)
    enum { CHAMBER_P_EFFECTIVE = 0, CHAMBER_P_CONSTANT = 1 };
    ChamberView chamberView(const double* x_dev, int pressure = CHAMBER_P_EFFECTIVE) const;
    void refreshChamberRef(); // r_c of every chamber from the current positions, on the device (beginTimestep)
    AeroView aeroView(const double* x_dev) const; // (with the wind, the density and dt as they are now)
    PlasticView plasticView(const double* x_dev, double dt_) const;
    void plasticFlow(const double* x_dev, double dt_); // zeroes the two counters and launches one flow on the stream: no synchronisation
    ShellPlasticView shellPlasticView(const double* x_dev, double dt_) const;
    void shellPlasticFlow(const double* x_dev, double dt_); // zeroes the four counters and launches the flows that are on: no synchronisation
    void refreshAeroLagged(); // n, A and c^n of every aerodynamic triangle from the current positions, on the device (beginTimestep)
    // The gas chambers' dense rank-k Hessian term, coef sum_c beta_c u_c u_c^T, as a correction around the solver's retained factor (chamber_kernels.h):
    // y_dev holds A^-1 r on entry and (A + coef sum beta_c u_c u_c^T)^-1 r on return, with beta and u at the mesh's current positions.  k further solves,
    // everything on the stream, no synchronisation.  Nothing without a gas chamber.  The stepper (computeSearchDir) and ipcgpu_chamber_gas_solve both call it.
    void chamberGasCorrect(double coef, bool projectDBC, double* y_dev);
    void chamberVolumeGradient(int gasIndex, bool projectDBC, double* u_dev); // u_c of the gasIndex-th gas chamber at the current positions
    DevBuf<double> d_gasU, d_gasZ, d_gasDots, d_gasW;
    size_t codimPartials() const; // doubles of d_partial the largest energy launch needs
    // *out_dev (+)= coef * energy of the chosen terms at x_dev; accumulate == false: the first term launched overwrites *out_dev, the later ones add.  The
    // limit's energy is +infinity with a stretch at or over its limit, which every comparison of the line search rejects like the fold of a rod node
    void codimEnergyAdd(const double* x_dev, double coef, double* out_dev, bool accumulate, unsigned which = CODIM_ALL);
    // grad_dev (nullable) += coef * gradient, a_dev (nullable) += coef * PSD Hessian blocks, at x_dev (null: the mesh's positions)
    void codimAssembleAdd(double coef, bool projectDBC, double* grad_dev, double* a_dev, const double* x_dev = nullptr, unsigned which = CODIM_ALL);
    void enqueueElasticEnergy(bool ownerRank, double* out_dev); // launch_energy (elasticity + inertia) and the codimensional energies on top
    // sigma1, sigma2 per triangle (host, 2 nTri, nullable), the maximum of sigma1 / limit and the number of triangles at or over their limit (synchronises)
    void shellStretch(double* sigma_host, double* maxRatio, int* nOver, const double* x_dev = nullptr);
    bool shellLimitFeasible(); // true without a limit; else one stretch query at the current positions
    void requireShellLimitFeasible(); // StateError naming the number of triangles over their limit
    int shellRubberDegenerate(); // the number of rubber triangles whose energy is +infinity at the current positions (0 without rubber; synchronises)
    bool shellRubberFeasible() { return !mesh.shell.nRubber() || shellRubberDegenerate() == 0; }
    void requireShellRubberFeasible(); // StateError naming the number of degenerate rubber triangles
    // a mesh without tetrahedra has no patch plan: the node pass initialises the gradient / the matrix diagonal in its place (only with a shell or a rod
    // set: shells only, rods only, or both)
    bool shellOnly() const { return mesh.nT == 0 && (mesh.shell.nTri() > 0 || mesh.rod.nSeg() > 0); }

    HipMesh& mesh;
    HipLinSysSolver& lin;
    hipStream_t stream;
    double dt = 0.025, dtSq = 0, gravity[3] = { 0, 0, 0 };
    double relGL2Tol = 1e-8, targetGRes = 0;
    // Config `timeIntegration BE | NM beta gamma` (Config.hpp:96, Config.cpp:112-118): 0 backward Euler, 1 Newmark
    int timeIntegration = 0;
    int warmStart = 0; // Config `warmStart`: initX option 0..4 (Optimizer.cpp:925-1080)
    double warmStepSize = 0.0; // step the last warm start could take
    double betaNM = 0.25, gammaNM = 0.5;
    DevBuf<double> d_acc, d_dxElastic; // acceleration, dx_Elastic = x - xTilta of the finished step (Optimizer.cpp:176-177, 574-586)
    double elasticCoef() const { return timeIntegration == 1 ? dtSq * betaNM : dtSq; } // Optimizer.cpp:3205-3224, 3416-3434, 3618-3632
    void setTimeIntegration(int type, double beta, double gamma);
    void getKinematics(double* vel, double* acc, double* dxElastic);
    void getDbcState(double* out4) const;
    // Optimizer::computeSystemEnergy (Optimizer.cpp:3746-3778): per component the energy, the linear and the angular momentum, reduced on the device.
    // d_xStepStart is result.V_prev as the reference's call sites see it (:1497, 1801 run BEFORE V_prev = V of :578 / :588): the positions the last
    // finished time step started from -- endTimestep swaps it with d_xPrev instead of overwriting x^t in place.  Without setComponents: one component.
    std::vector<int> compNodeEnd, compTetEnd; // accumulated ends (compVAccSize / compFAccSize, main.cpp:1111-1112)
    DevBuf<double> d_xStepStart, d_reportRec;
    DevBuf<int> d_reportSlices, d_reportNodeStart, d_reportTetStart;
    PinnedBuf<double> h_report;
    bool reportPlanValid = false;
    int nReportNodeSlices = 0, nReportSlices = 0;
    void setComponents(int nComp, const int* nodeEnd, const int* tetEnd);
    void ensureReportPlan();
    void systemReport(double* sysE, double* sysM_3, double* sysL_3); // any pointer may be null; changes no state
    void saveStatus(const std::string& path); // Optimizer::saveStatus, Optimizer.cpp:2964-3011
    void loadStatus(const std::string& path); // restart, Optimizer.cpp:179-248
    DevBuf<double> d_vel, d_xPrev, d_searchDir, d_gradient, d_minusG, d_x0, d_partial, d_scalar;
    DevBuf<double> d_damp, d_xDamp, d_zeroMass, d_dampDx, d_dampAdx;
    unsigned long long dampPatternVersion = ~0ULL;
    DevBuf<int> d_flag, d_handleIds;
    DevBuf<double> d_handleAng;
    int nHandles = 0;
    // Mesh::DirichletBCs (Mesh.hpp:23-39) and scripted component velocities (AnimScripter.cpp:1413-1435)
    struct DbcGroup {
        std::vector<int> ids;
        DevBuf<int> d_ids;
        DevBuf<double> d_pos;
        double lin[3], ang[3], t0, t1;
        // the hard-coded scripts of AnimScripter.cpp:1961-2135 (DCOSquash6, DCOSqueezeOut, DCORotCylinders, ...): every node of the group is a
        // NONZERO Dirichlet node whatever its velocity currently is, and rotations turn about a centre fixed at set-up time
        bool forceNonzero = false, hasCenter = false;
        double center[3] = { 0, 0, 0 };
        // mesh-sequence motion (`meshSeq <folder>`, AnimScripter.cpp:1465-1528): the positions the nodes are to reach in the next time step,
        // handed over before every step; the velocities above are then ignored
        bool hasTargets = false;
        DevBuf<double> d_targets;
        bool isZero() const { return !forceNonzero && lin[0] == 0 && lin[1] == 0 && lin[2] == 0 && ang[0] == 0 && ang[1] == 0 && ang[2] == 0; }
    };
    std::vector<std::unique_ptr<DbcGroup>> dbcGroups;
    // Mesh::NeumannBCs (Mesh.hpp:47-56): a mass-weighted acceleration on a vertex set while t0 <= stepStartTime < t1
    struct NbcGroup {
        int n = 0;
        DevBuf<int> d_ids;
        double a[3], t0, t1;
    };
    std::vector<std::unique_ptr<NbcGroup>> nbcGroups;
    void addNeumannBC(int n, const int* ids, const double* accel3, double t0, double t1);
    void neumannGradientAdd(double* grad_dev); // Optimizer.cpp:3452-3461
    double neumannEnergy(); // :3241-3250
    std::vector<int> baseDbcType;
    double stepStartTime = 0, stepEndTime = 0; // AnimScripter.cpp:1406-1407
    // augmented-Lagrangian Dirichlet fallback (AnimScripter.cpp:2150-2157, 2280-2350; Optimizer.cpp:1826-1828, 2168-2203)
    std::vector<int> tpIds, tpIdsOnDevice; // targetPos keys = the Dirichlet nodes, ascending (and the list d_tpIds currently holds)
    DevBuf<int> d_tpIds;
    DevBuf<double> d_tpPos, d_tpLam, d_tpStage;
    double dist2Tol = 0, completedStep = 1.0, lastMove = 1.0, rhoDBC = 0.0, CN_MBC = 0.0;
    bool projDBC = true; // m_projectDBC
    MdbcView mdbc() const { return MdbcView{ (int)tpIds.size(), d_tpIds.p, d_tpPos.p, d_tpLam.p, mesh.d_mass.p }; }
    void buildTargetPositions(bool deferTolerance = false); // after the scripted search direction is known, before it is applied
    void finishTolerance(); // dist2Tol from the scripted directions buildTargetPositions(true) left in pinned host memory (behind a synchronisation)
    PinnedBuf<double> h_tpStage;
    bool tolPending = false;
    void initSubProblem(); // head of solveSub_IP (Optimizer.cpp:1826-1828)
    double computeCompletedStepSize(); // AnimScripter.cpp:2286-2300
    void dirichletPenaltyUpdate(); // Optimizer.cpp:2168-2203
    void addDirichletBC(int n, const int* ids, const double* lin3, const double* angRad3, double t0, double t1);
    void setDBCVertices(); // AnimScripter::setDBCVertices, AnimScripter.cpp:58-110
    bool dbcGroupMotion(); // adds the active groups' motion to d_searchDir; true if any
    double rotCenter[3] = { 0, 0, 0 };
    // the scalar board (scalar_slots.h): d_scalar holds one double per ScalarSlot, h_scalar.p[S] is the published copy of d_scalar.p[S] and nothing else
    PinnedBuf<double> h_scalar;
    double* slot(ScalarSlot s) const { return d_scalar.p + s; }
    double* slotMapped(ScalarSlot s) const { return h_scalar.dev + s; } // the slot's place in the mirror as kernels address it
    double published(ScalarSlot s) const { return h_scalar.p[s]; } // valid behind a publish of s and a synchronisation
    void publish(ScalarSlot first, int count = 1); // slots [first, first + count) to their places in the mirror: one launch, no synchronisation
    double readScalar(ScalarSlot s); // publish(s), synchronise, published(s)
    PinnedBuf<int> h_flag;
    int innerIterAmt = 0, globalIterNum = 0, k = 0;
    double lastEnergyVal = 0, lastStepSize = 0, lastAlphaFeasible = 0;
    double timers[16] = { 0 };
    bool initialised = false;
    int rank = 0, worldSize = 1;
    int tetBegin = 0, tetEnd = 0;
    ipcgpu_allreduce_fn_t allreduce = nullptr;
    ipcgpu_allreduce_stream_fn_t allreduceStream = nullptr; // takes precedence: enqueued on `stream`, no host synchronisation
    void hookReduce(double* dev, long long n, int op);
    // Contact-free single-rank iterations (the matTwist bench): the scalars the host branches on come back in batches -- one read after the
    // solve (|p|_inf for the next convergence test, the inversion step filter, E at the current iterate), one after the trial step (inversion
    // flag + E at the trial point) -- instead of one host synchronisation per scalar; the assembly bucket is timed with HIP events.
    bool fastPath() const;
    bool cachedDistValid = false, cachedE0Valid = false;
    double cachedDist = 0, cachedE0 = 0, cachedFilter = 0;
    // ... and, second step: the first trial of the line search is taken on the device behind the solve
    // as well -- its step size, inversion flag and energy arrive with the same synchronisation, ONE per Newton iteration
    bool cachedTrialValid = false, cachedTrialInverted = false;
    double cachedTrialE = 0, cachedAlpha = 1.0;
    // ... and, round 4: the NEXT iteration's fused assembly (gradient + Hessian at the trial point) is enqueued behind the trial kernels, before that one
    // synchronisation -- into buffers of its own, swapped in when the trial is accepted and the next pass asks for exactly this assembly.  The host's
    // read-back, its decisions and the way back through the caller's loop (45 us per iteration on the bench) then run beside a kernel instead of in front of it.
    // Nothing is skipped and nothing observable moves: d_gradient and the solver's values keep describing the iterate the search direction came from
    // until the swap; a rejected trial, a converged pass (one assembly per time step goes unused), a bad pivot or a time-step call drop the buffers' content.
    DevBuf<double> d_aSpec, d_gradSpec;
    bool specAsmValid = false;
    void speculativeAssembly();
    hipEvent_t evAsm0 = nullptr, evAsm1 = nullptr, evTail = nullptr;
    bool evAsmPending = false;
    int evAsmWeight = 1;
    unsigned asmLaunches = 0;
    void resolveEventTimers();
    DevBuf<double> d_contactG; // this rank's share of the barrier forces before their all-reduce (contact-pair lists sharded)
    void* allreduceUser = nullptr;
    void* allreduceStreamUser = nullptr; // separate slots: the two hooks can be set in any order
    void reduceSum(double* dev, long long n);
    void reduceMin(double* dev, long long n);
    PatchPlan patch; // atomic-free assembly plan for the current pattern
    int patchVersion = -1;
    void ensurePatchPlan();
    void patchShard(int& pb, int& pe) const;
    // Owner-computes sharding (round 4; SURVEY.md 8e as north_star states it): with the assembly AND the solver sharded, a rank assembles exactly the CSR rows
    // its fronts read -- the rows of the nodes its subtrees eliminate plus the rows of the separator nodes above the cut, which every rank repeats -- by running
    // the patches that hold such a node (elements and contact stencils on a cut are evaluated by both sides, like the halo of a patch).  NO matrix value crosses
    // ranks; the gradient does (one all-reduce of 3 nV doubles in which every node is contributed by one designated rank), scalars, and what the solver
    // exchanges above its cut (update matrices / vectors of the subtree roots, the solution).
    bool ownerMode() const;
    void ensureOwnerPlan();
    int ownerPlanPatch = -1, ownerPlanAnalysis = -1;
    int nOwnerPatches = 0;
    DevBuf<int> d_ownerPatches; // the patches this rank runs
    DevBuf<unsigned char> d_need, d_mine; // per node: rows needed on this rank / this rank is the node's designated contributor to all-reduced nodal vectors
    long long ownerNeededNodes = 0;
    bool matrixComplete = true; // false after an owner-mode assembly: a[] holds this rank's rows only
    void maskAndReduceGradient(double* g);
    void ownerGradientTail(bool projectDBC); // stencils part 1, the exchange, Neumann, part 2, penalty: what computeGradient and assembleSystem share
    void completeMatrix(); // sum of the designated rows over the ranks: for the consumers of the WHOLE matrix on a sharded context (diagonal fallback, get_a)
    long long commBytes = 0, commCalls = 0; // all-reduced through the hook by the optimizer itself (the solver counts its own: HipLinSysSolver::exchangedBytes)
    // self-contact, interior point (fullyImplicit_IP with isSelfCollision, Optimizer.cpp:1518-1819)
    HipContact* contact = nullptr;
    bool selfCollision = false;
    double dHatEps = 1.0e-3, dHat = 0, kappa = 0, dTol = 0;
    bool absParameters = false; // useAbsParameters: lengths of `tuning` and the tolerance are absolute (Config.cpp:553-555)
    double dTolRel = 1.0e-9, kappaMinMultiplier = 1.0e11; // tuning[3] (Optimizer.cpp:102-106), Config.hpp:139
    double lenScale2() const { return absParameters ? 1.0 : mesh.bboxDiag2; }
    ContactPattern contactPattern; // contact connectivity inside the current pattern (vNeighbor_IP)
    std::vector<std::array<int, 4>> closeID; // closeMConstraintID / Val (Optimizer.cpp:2396-2440)
    std::vector<double> closeVal;
    int lastCCDPair[2] = { 0, 0 }, nFullCCD = 0, nPatternChanges = 0, dbcIncomplete = 0;
    // "does the pattern cover the contact sets" as answered at the end of the last iteration, stamped with the versions of sets and pattern it was asked for
    unsigned long long coverSets = ~0ull;
    int coverPattern = -1;
    bool coverAnswer = false;
    // look-ahead of the contact pattern in units of dHat (ipcgpu_opt_set_pattern_lookahead; < 1 = exact pattern).  Negative = by mesh size (lookahead()): what it
    // trades is host-side analyses against fill in the factor, and the two scale differently -- measured (profiles/r06_pattern_lookahead_ab.txt): 40 K nodes, ms per
    // Newton iteration at pad 1 / 2.25 / 4: 22.6 / 11.4 / 9.9 (27 / 7 / 4 analyses of ~14 ms); 375 K nodes: 461 / 258 / 357 (an analysis costs ~130 ms, but the
    // factorisation 139 / 243 / 341 ms -- 3.7 / 7.2 / 10.7 TFLOP)
    double patternPad = -1.0;
    double lookahead() const { return patternPad >= 0.0 ? patternPad : (mesh.nV > 150000 ? 2.25 : 4.0); }
    // analytic half-space obstacles (animConfig.collisionObjects) and their close-constraint list (Optimizer.cpp:2364-2374)
    std::vector<std::unique_ptr<HipHalfSpace>> planes;
    // analytic round colliders (spheres, capsules: round_collider_kernels.h)
    std::vector<std::unique_ptr<HipRoundCollider>> rounds;
    // THE walk over the analytic obstacles: all planes in registration order, then all rounds in registration order, whatever the order of the add calls
    // (the energy sums and the object index of closeHS are positions in it).  listColliders() after every change of `planes` or `rounds`.
    std::vector<HipVertexCollider*> colliders;
    void listColliders();
    std::vector<std::pair<int, int>> closeHS; // (object, vertex): the object's position in `colliders`
    std::vector<double> closeHSVal;
    // lagged friction: Optimizer.cpp:286-304, 1525-1600, 1615-1790; the lagged sets live in HipContact /
    // HipHalfSpace, x^t is d_xPrev
    double selfFric = 0.0, epsV = 1.0e-3, fricDHat0 = 0, fricDHat = -1.0;
    // eps_v homotopy (tuning[5], Optimizer.cpp:296-303, 1717, 1776-1781): fricDHat is halved down (or clamped UP) to this target between the
    // friction-lag passes, the tangent-space convergence test runs only once it is there; < 0: the same as the start value (no homotopy)
    double epsVTarget = -1.0, fricDHatTarget = 0;
    int fricIterAmt = 1, fricIterI = 0;
    bool fricLoopForced = false; // a mesh collision object with a friction coefficient: the lagging loop runs, no pair carries friction (Optimizer.cpp:156-161)
    bool solveFric() const;
    void updateFrictionLag();
    bool nextSubproblem(); // tail of the fullyImplicit_IP loop body after a converged solveSub_IP; true = run another one
    bool ipOn() const { return selfCollision || !colliders.empty(); }
    size_t nConstraints() const;
    int addHalfSpace(HipContact* c, const double* origin3, const double* normal3, double dHatEps);
    int addRoundCollider(HipContact* c, const double* p0, const double* p1, double R, int hollow, double dHatEps);
    void requireRoundsFeasible(); // throws where dHat has outgrown a hollow sphere, or a node with dbc == 0 lies on or inside a collider
    bool anyIntersection();
    void elasticInertiaGradient(bool projectDBC, bool finish = true); // finish = false: owner-computes callers that exchange the sum themselves
    void barrierGradientAdd(bool projectDBC, double kappa, bool activeOnly, double* grad_dev, int part = 0);
    void enableSelfCollision(HipContact* c, double dHatEps);
    void setVelocity(const double* vel3nV);
    void computeConstraintSets();
    double kappaFloor() const;
    void initKappa();
    void postLineSearch();
    bool isIntersected();
    void computeXTilta();
};

// Buffers of ipcgpu_elastic_stress: the incidence list of the current mesh (built at the first call that asks for nodal values, dropped with the
// mesh), the two record arrays, and the count of invalid elements with its mapped host copy
struct StressFields {
    bool planValid = false;
    DevBuf<int> d_ptr, d_elems, d_invalid;
    DevBuf<double> d_elem, d_node;
    PinnedBuf<int> h_invalid;
};

} // namespace ipcgpu

struct ipcgpu_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::unique_ptr<ipcgpu::HipMesh> mesh;
    std::unique_ptr<ipcgpu::HipLinSysSolver> lin;
    std::unique_ptr<ipcgpu::HipOptimizer> opt;
    std::unique_ptr<ipcgpu::HipContact> contact;
    std::unique_ptr<ipcgpu::StressFields> stress;
    int rank = 0, worldSize = 1;
    // point-to-point exchange hooks of the sharded solver (ipcgpu_opt_set_exchange[_stream]); stored here as opaque pointers of the C ABI's types
    void* exchange = nullptr;
    void* exchangeUser = nullptr;
    void* exchangeStream = nullptr;
    void* exchangeStreamUser = nullptr;
};
