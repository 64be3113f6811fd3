// HipContact: the self-collision handler of the hot path (SelfCollisionHandler<3> statics,
// src/CollisionObject/SelfCollisionHandler.hpp:21-250) with its state in HBM.
//   computeConstraintSet      SelfCollisionHandler.cpp:2149-2478  -> buildConstraintSet (grid broad phase, typing and the merge of
//                                                                   duplicate tuples on the GPU, in the order of the reference's std::map)
//   evaluateConstraints + b   :38-81, Optimizer.cpp:3252-3353     -> energy
//   leftMultiplyConstraintJacobianT / augmentParaEEGradient  :84-148, 2990-3036   -> gradientAdd
//   augmentIPHessian / augmentParaEEHessian   :418-561, 3039-3201 -> hessianAdd
//   augmentConnectivity       :330-415                            -> connectivity
//   largestFeasibleStepSize[_CCD]  :564-686, 982-1366             -> ccdPartial / ccdFull / ccdFullReference (conservative additive CCD)
#pragma once
#include <cstddef>
#include <cstdlib>
#include "common.h"
#include "contact_groups.h"
#include <array>
#include <utility>
#include <functional>
#include <vector>

namespace ipcgpu {

class HipMesh;
class HipLinSysSolver;

// uniform grid of the broad phase (cell_of, hip_contact.hip): laid out on the host, taken by value by the kernels
struct Grid {
    double lo[3], h;
    int dim[3];
};

// counters_ (HipContact): C_COUNT ints of device memory, zeroed at the head of every pass that counts.  One pass uses the block at a time; each pass has
// its own enum for what the first entries mean.  The kernels take the address of the entry they count into, or the block's base and these indices.
constexpr int C_COUNT = 16;
enum BuildCounter : int { C_PT = 0, C_EE = 1, C_STALE = 2 }; // buildConstraintSet: point-triangle records, edge-edge records, "the positions have left the grid" (k_bbox_final).  isIntersected: C_PT is its flag
enum HessianCounter : int { C_MISS = 0, C_SWEEPS = 1, C_BIN0 = 4 }; // hessianAdd, patternCovers: a node pair outside the CSR pattern, Jacobi sweeps of the projections, the first of the NBINS stencil-kind bin counts (k_bin_stencils)
enum CcdCounter : int { C_QUERIED = 0, C_HITS = 1 }; // ccdFull, ccdFullReference: queried pairs, pairs that returned a time inside the step (the hit list)
enum CloseCounter : int { C_CLOSE = 0, C_CLOSE_MISS = 2, C_CLOSE_END = 4 }; // closeStencils: stencils closer than dTol, the pattern check's miss flag riding along; [0, C_CLOSE_END) come back
// ccdOut_ (HipContact): the 64-bit words a step-bound pass leaves its result in, set by k_step_bounds_init at its head; non-negative doubles as bits, which order like integers
enum CcdSlot : int {
    CCD_MIN = 0, // the smallest time a pair returned; all ones: none
    CCD_ARG = 1, // the smallest order key (pair_key, ref_key) among the pairs that attain it; all ones: none
    CCD_AUX = 2, // stepBounds, maxSurfaceSpeed, makeGrid: the largest |p| (k_max_speed).  ccdFullReference: the bound the vertex sweeps left
    CCD_STEP = 3, // the step the pass is bounded by (stepBounds: cut by the inversion filter's root)
    CCD_SLOTS = 4
};

// what the host needs between the stages of a build, written to mapped host memory by one thread (three blits of 12, 4 and 48 bytes before)
struct BuildReadback {
    int cnt[4]; // point-triangle records, edge-edge records, stale-grid flag, total number of cell entries
    double box[6];
    unsigned long long totals; // category totals of the candidate list (k_bucket_rank_classify's flags, scanned)
    int nUnique, pad;
};
// Everything the host reads from the contact kernels through mapped memory: HipContact::readback_ is one of these.  Every member but hessError is
// written and read inside ONE call of the handler, between a launch and the synchronisation behind it, and the handler's calls do not overlap on its
// stream: those members are never live together.  hessError is live from hessianAdd(deferCheck) to takeHessianError(), across whatever the stepper
// calls in between (energy, stepBounds, both CCDs, builds): no other member may share its bytes.
struct ContactReadback {
    BuildReadback build; // buildConstraintSet (k_publish_narrow, then k_dup_emit: totals, nUnique), isIntersected (k_publish_narrow)
    unsigned long long stepBounds[CCD_SLOTS]; // stepBounds, maxSurfaceSpeed: ccdOut_, by CcdSlot
    double energy; // energy(): the barrier energy behind energyEnqueue
    double refBox[7]; // ccdFullReference, first wait: the capped step, lower and upper corner of the hash (k_ref_box_final)
    unsigned long long refCcd[2]; // ccdFull, ccdFullReference, last wait: ccdOut_[CCD_MIN], [CCD_ARG] ...
    int refCount[2]; // ... and C_QUERIED, C_HITS
    int refItems; // ccdFull, ccdFullReference, second wait: total number of cell entries
    int hessError; // C_MISS of a hessianAdd(deferCheck): see above
    int close[C_CLOSE_END]; // closeStencils: counters [0, C_CLOSE_END)
    double sweptBox[7]; // ccdFull, first wait: lower and upper corner of the positions' box, the largest |p| (makeGrid)
};
static_assert(sizeof(BuildReadback) == 80 && offsetof(BuildReadback, box) % 8 == 0 && offsetof(BuildReadback, totals) % 8 == 0, "k_publish_narrow and k_dup_emit write this record");
static_assert(offsetof(ContactReadback, build) == 0 && offsetof(ContactReadback, stepBounds) % 8 == 0 && offsetof(ContactReadback, energy) % 8 == 0
        && offsetof(ContactReadback, refBox) % 8 == 0 && offsetof(ContactReadback, refCcd) % 8 == 0 && offsetof(ContactReadback, sweptBox) % 8 == 0,
    "the kernels store the 8-byte members whole");
static_assert(sizeof(ContactReadback) == 280, "members are added at the end; every publish stays inside its own member");

class HipContact {
public:
    explicit HipContact(hipStream_t s) : stream(s)
    {
    }
    hipStream_t stream;
    // surface (Mesh::SF, SVI, SFEdges; Mesh.cpp:495-515, 890-930)
    int nSF = 0, nSVI = 0, nSFE = 0;
    std::vector<int> SF; // column-major nSF x 3
    std::vector<int> SVI;
    std::vector<std::pair<int, int>> SFEdges;
    DevBuf<int> d_SF, d_SVI, d_SFE; // d_SF: int[3 nSF] (t0 t1 t2 per triangle), d_SFE: int[2 nSFE]
    DevBuf<double> d_xRest; // rest positions xyz-interleaved (eps_x needs rest edge lengths)
    // sets
    // The sets live in HBM (d_active ... d_csPTEE with the counts below); the host vectors are mirrors that syncHost() fills
    // when somebody needs the tuples on the host (tests, the connectivity of a pattern change, friction lagging).
    std::vector<std::array<int, 4>> active, para;
    std::vector<std::array<int, 2>> paraEIEJ, csPTEE;
    DevBuf<int> d_active, d_para, d_paraEIEJ, d_csPTEE;
    int nActive() const { return nActive_; }
    int nPara() const { return nPara_; }
    int nCand() const { return nCand_; }
    void syncHost() const;
    bool surfaceSet = false;

    // CE: codimensional segments (`.seg` shapes, Mesh::CE) as node pairs; nodes without any neighbour in the mesh are codimensional points
    // (`.pt` shapes): both join SVI, the segments SFEdges (Mesh.cpp:490-515, 912-927)
    void setSurface(const HipMesh& mesh, int nSF, const int* SF_colmajor, int nCE = 0, const int* CE_pairs = nullptr);
    std::vector<int> codimPoints;
    bool exactPredicates = false; // the intersection checks as a USE_PREDICATES build of the reference makes them (IglUtils.hpp:222-233, 280-294)
    // kinematic obstacle nodes (the reference's MeshCO riding along as a surface-only component, MeshCO.cpp) and, for scenes with
    // `selfCollisionOff`, the filter that keeps only primitive pairs involving an obstacle
    void setObstacle(int nV, int n, const int* ids, bool obstacleOnly);
    bool hasObstacle = false, obstacleOnly = false;
    DevBuf<int> d_obst, d_pairFlags;
    const int* pairFlags(int nV, const int* dbc_dev);
    // contact groups (ipcgpu_set_contact_groups; contact_groups.h): per node the group of its component and the group's row of the collide matrix, OR-ed
    // into the pair flags, and the 16 x 16 friction scales k_friction_lag multiplies the lagged normal forces with.  Empty words: the default (one group)
    void setGroups(int nV, const std::vector<int>& words, const std::vector<double>& scale16, int nGroups);
    bool hasGroups = false;
    int nGroups = 1;
    std::vector<int> groupWord;
    DevBuf<int> d_groupWord;
    DevBuf<double> d_groupScale;
    void setSets(int nA, const int* a4, int nP, const int* p4, const int* pe2);
    void uploadSets();
    // returns #active
    int buildConstraintSet(const HipMesh& mesh, const double* x_dev, const int* dbc_dev, double dHat);
    // Multi-GPU ("contact pairs assigned to the owner of ..."): the constraint SETS are the same on every rank (integer outputs every rank
    // needs for the pattern), their EVALUATION is split.  energy(): rank r takes the stencils [n r / W, n (r + 1) / W) of the two lists and all-reduces its
    // scalar through `shardReduce`.  gradientAdd / hessianAdd (round 4): the CALLER hands in a node mask -- a stencil is evaluated where one of its nodes owns
    // rows (HipOptimizer's owner-computes plan); with a null mask they evaluate the whole lists, whatever the context's shard (the C entry points do).
    int shardRank = 0, shardWorld = 1;
    std::function<void(double*, long long)> shardReduce;
    void shardRange(int n, int& b, int& e) const
    {
        b = (int)((long long)n * shardRank / shardWorld);
        e = (int)((long long)n * (shardRank + 1) / shardWorld);
    }
    double energy(const double* x_dev, double dHat, double kappa, DevBuf<double>& partial, double* scalar_dev);
    // the same without the read-back: the value is left in *scalar_dev on the stream (false: empty sets, nothing enqueued, the value is 0) -- the time stepper
    // reads it together with the elastic energy, one synchronisation for both
    // pubCount > 0: the reduction's own launch also copies pubCount doubles pubSrc -> pubDst (mapped host memory; at most one wave of 32-bit words);
    // publishedByEnergy() says whether it did
    bool energyEnqueue(const double* x_dev, double dHat, double kappa, DevBuf<double>& partial, double* scalar_dev, const double* pubSrc = nullptr,
        double* pubDst = nullptr, int pubCount = 0);
    bool publishedByEnergy() const { return publishedByEnergy_; }
    bool publishedByEnergy_ = false;
    // useActive / usePara: initKappa leaves the mollified set out (Optimizer.cpp:2262-2270)
    void gradientAdd(const double* x_dev, const int* dbc_dev, int nV, double dHat, double kappa, int projectDBC, double* grad_dev, bool useActive = true,
        bool usePara = true, const unsigned char* need_dev = nullptr);
    // deferCheck: the "pair outside the pattern" flag is not waited for; the caller calls takeHessianError() behind its next synchronisation of the stream
    void hessianAdd(const double* x_dev, const int* dbc_dev, const HipLinSysSolver& lin, double dHat, double kappa, int projectDBC,
        double* a_dev, const unsigned char* need_dev = nullptr, bool deferCheck = false);
    void takeHessianError(); // throws what hessianAdd(..., deferCheck = true) would have thrown
    // the reference's per-constraint interface on host arrays of MMCVID tuples (SelfCollisionHandler.cpp:37-148; ipcgpu_contact_evaluate / _jt_multiply):
    // val[i] = squared distance of tuple i;  out += coef * multiplicity_i * input[i] * grad d_i
    void evaluateTuples(const double* x_dev, int n, const int* tuples4, double* val);
    void jtMultiplyTuples(const double* x_dev, int nV, int n, const int* tuples4, const double* input, double coef, double* out_3nV);
    DevBuf<int> tupleBuf_;
    DevBuf<double> tupleVal_, tupleOut_;
    void connectivity(std::vector<std::pair<int, int>>& pairs) const;
    bool patternCovers(const HipLinSysSolver& lin); // every node pair of the current sets has its block in lin's pattern (one small kernel)
    void candidateConnectivity(std::vector<std::pair<int, int>>& pairs) const; // appends; all node pairs of the candidate list
    void candidateConnectivitySorted(std::vector<std::pair<int, int>>& pairs); // the same, sorted and unique, formed on the device
    // conservative CCD step bounds; pair2 receives the limiting pair ((-svI-1, sfI) or (eI, eJ)); returns the new bound
    double ccdPartial(const double* x_dev, const double* p_dev, double slackness, double stepSize, int* pair2);
    // inversion filter (root already on the device, may be null) -> ccdPartial -> maxSurfaceSpeed with one synchronisation (the time stepper's step-size pipeline)
    void stepBounds(const double* x_dev, const double* p_dev, double slackness, double stepSize, const double* filterDev, double* alphaOut, int* pair2,
        double* pMaxOut);
    double ccdFull(const HipMesh& mesh, const double* x_dev, const double* p_dev, const int* dbc_dev, double slackness, double stepSize, int* pair2,
        int* nCand);
    // the full sweep as the reference runs it (SelfCollisionHandler.cpp:982-1366 over SpatialHash.hpp:589-832): the hash first caps the step
    // (alphaCapped), a surface vertex is swept against vertices / edges / triangles that share a cell with it, an edge against edges;
    // arg3 = (kind, i, j) of the limiting pair: K_PP (svI, svJ), K_PE (svI, eI), K_PT (svI, sfI), K_EE (eI, eJ)
    double ccdFullReference(const HipMesh& mesh, const double* x_dev, const double* p_dev, const int* dbc_dev, double slackness, double stepSize,
        double* alphaCapped, int* arg3, int* nCand);
    int ccdMode = 1; // 1: ccdFullReference in the time stepper; 0: the swept-box sweep of PT / EE pairs (ccdFull)
    bool isIntersected(const HipMesh& mesh, const double* x_dev, const int* dbc_dev);
    void evalStencils(const std::vector<std::array<int, 4>>& ids, const double* x_dev, std::vector<double>& d2);
    // lin != null: *covers = patternCovers(*lin), answered with the same synchronisation
    void closeStencils(const double* x_dev, double dTol, std::vector<std::array<int, 4>>& ids, std::vector<double>& d2, const HipLinSysSolver* lin = nullptr,
        int* covers = nullptr);
    unsigned long long setsVersion = 0; // bumped whenever the sets change (buildConstraintSet, uploadSets): what a cached coverage answer is stamped with
    double maxSurfaceSpeed(const double* p_dev); // max_{v in SVI} |p_v|  (CFL bound, Optimizer.cpp:1947-1953)
    // lagged friction of the self-contact set: MMActiveSet_lastH, MMLambda_lastH, MMDistCoord, MMTanBasis
    std::vector<std::array<int, 4>> fricSet;
    DevBuf<int> d_fricSet;
    DevBuf<double> d_fricLambda, d_fricCoord, d_fricBasis;
    double fricScaleSelf = 1.0, fricScaleObst = 1.0; // MeshCO::friction beside selfFric: factors on the lagged normal forces by stencil kind
    void frictionLagClear();
    void frictionLagUpdate(const double* x_dev, double dHat, double kappa); // lags the current `active` set (Optimizer.cpp:1578-1598)
    void frictionGet(double* lambda, double* coord2, double* basis6);
    double frictionEnergy(const double* x_dev, const double* xt_dev, double eps2, double coef, DevBuf<double>& partial, double* scalar_dev);
    void frictionGradientAdd(const double* x_dev, const double* xt_dev, double eps2, double coef, double* grad_dev);
    void frictionHessianAdd(const double* x_dev, const double* xt_dev, const int* dbc_dev, const HipLinSysSolver& lin, double eps2, double coef,
        int projectDBC, double* a_dev);
    void frictionConnectivity(std::vector<std::pair<int, int>>& pairs) const; // appends
    // Contact report (ipcgpu_contact_report, include/ipcgpu.h): per pair of components, or component and half-space, the smallest squared distance, the
    // constraint counts by kind, the barrier forces and torques on either side, the lagged friction forces and their work.  Evaluates the sets held
    // (active, mollified, every plane's vertex set, the lagged friction set) at x_dev in buffers of its own: no state of the handler changes.
    // compNodeEnd: accumulated node ends of the components; Vt_colmajor null or coef <= 0: no friction part.  Returns the number of rows; rowsI / rowsD
    // are filled when capacity >= that number.
    struct ReportPlane {
        double n[3], D;
        const int* set_dev;
        int count;
    };
    int contactReport(const double* x_dev, int nV, const std::vector<int>& compNodeEnd, const std::vector<ReportPlane>& planes, double dHat, double kappa,
        const double* Vt_colmajor, double eps2, double coef, int capacity, int* rowsI_8n, double* rowsD_20n);

private:
    // contact report: node -> component, the previous positions, the records (key, kind, index, 13 values, SoA), the counting sort of the records by
    // key, the slice list with its partial sums, and the mapped host block the row keys, ends and finished rows come back through
    struct ReportScratch {
        std::vector<int> compNodeEnd;
        DevBuf<int> nodeComp, kind, idx, seg, sorted, slices, sliceStart, sliceI;
        DevBuf<unsigned> key;
        DevBuf<double> xt, val, sliceD;
        ZeroKeptCounters count;
        DevBuf<unsigned long long> start;
        DevBuf<char> scanTmp;
        PinnedBuf<int> hostI;
        PinnedBuf<double> hostD;
    } report_;
    // host side of the grids: the swept grid of ccdFull (over the positions' own box grown by the step's reach, read back with the largest |p| in one wait: box_ is
    // not touched), the grid of a build or check over box_ padded by two cells of size h (grown until the grid has at most 2^26 cells), and the box of the
    // positions measured synchronously (first build or check of a surface)
    Grid makeGrid(const HipMesh& mesh, const double* x_dev, const double* p_dev, double alpha, double minCell, long long& nCells);
    Grid gridOverBox(double h, long long& nCells) const;
    double* enqueueBox(int nV, const double* x_dev); // the box of the positions, six doubles on the device (k_bbox_partial, k_bbox_final without the stale check)
    void measureBox(int nV, const double* x_dev);
    void buildCells(const Grid& g, long long nCells, const double* x_dev, const double* p_dev, double alpha);
    unsigned long long* ccdOutBegin(double stepSize, const double* filterDev = nullptr); // ccdOut_ allocated and set for a pass (k_step_bounds_init)
    void readSweep(); // ccdFull, ccdFullReference: ccdOut_[CCD_MIN], [CCD_ARG], C_QUERIED and C_HITS into readback_ (refCcd, refCount), waited for
    void enqueueMaxSpeed(int n, const int* ids_dev, const double* p_dev, CcdSlot slot); // ccdOut_[slot] = max(itself, largest |p| of the n nodes; ids null: 0 .. n - 1)
    void* scanTmp(size_t bytes); // temporary storage of a hipcub call, grown on demand
    template <class T>
    void exclusiveSum(const T* in, T* out, int count);
    DevBuf<int> d_ids_;
    DevBuf<double> d_vals_;
    DevBuf<unsigned long long> ccdOut_, ccdHits_;
    DevBuf<int> d_codimPoints;
    DevBuf<int> outPT_, outEE_, counters_;
    DevBuf<int> d_v2sv, refVbox_, refStart_, refItems_; // reference-mode sweep: node -> surface index, index boxes, the three cell structures in one
    ZeroKeptCounters refCount_;
    DevBuf<double> bboxPartial_;
    bool haveBox_ = false; // box_: the bounding box the last constraint-set build or intersection check measured (the next grid is laid over it)
    double box_[6] = { 0, 0, 0, 0, 0, 0 };
    // the narrow phase's grids, triangles and edges in one array of 2 nCells + 1 cells (k_grid_insert_both); the intersection check uses nCells + 1 of them,
    // the swept grid of ccdFull 2 (nCells + 1) with bare indices as items (buildCells).  One pass at a time; gridItems_ never shrinks
    ZeroKeptCounters gridCount_;
    DevBuf<int> gridStart_, gridItems_;
    // on-device assembly of the sets (buildConstraintSet)
    int nActive_ = 0, nPara_ = 0, nCand_ = 0;
    mutable bool hostStale_ = false;
    DevBuf<unsigned long long> sortKeyIn_, sortKeyOut_, flags_, flagPos_;
    DevBuf<int> permPT_, dupTuple_, dupSorted_, closeIdx_;
    // counting sorts of the record lists (by first primitive) and of the duplicate candidates (by vertex): counters, bucket starts, bucket contents, runs
    ZeroKeptCounters bucketCount_, dupCount_;
    DevBuf<int> bucketStart_, bucketSeg_, dupStart_, runs_, runPos_;
    void readbackInit();
    bool hessErrPending_ = false;
    PinnedBuf<ContactReadback> readback_; // one record (mapped memory, written by the kernels)
    DevBuf<double> closeVal_;
    DevBuf<char> scanTmp_;
    // deterministic scatter of the barrier / friction terms (hip_contact.hip "Deterministic scatter"): per-stencil slots, keys, bucket counters / starts /
    // contents of the counting sort
    DevBuf<double> detVals_;
    DevBuf<unsigned> detKey_;
    ZeroKeptCounters detCount_;
    DevBuf<int> detStart_, detSeg_, detSorted_, detRow_, hessPerm_; // hessPerm_: the two lists' indices binned by stencil kind (k_bin_stencils)
    void detBegin(size_t nSlots, int valsPerSlot, bool withRow, bool fillKeys, size_t nKeys);
    void detBuckets(size_t nSlots, size_t nKeys, int div);
    void detReduce3(size_t nSlots, size_t nKeys, double* grad_dev);
    void detReduceBlocks(size_t nSlots, size_t nKeys, const int* ia_dev, double* a_dev);
};

} // namespace ipcgpu
