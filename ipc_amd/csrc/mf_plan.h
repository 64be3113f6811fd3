// Launch plan of the GPU multifrontal LL^T: which front takes which kernel, in what order, and every descriptor record the factorisation and the two sweeps
// read.  Pure integer logic on an MfSymbolic, host only (no HIP header: tests/test_mf_plan.py builds it with g++ and reads the records the way the kernels do).
// MfNumeric::setup() uploads the arrays as they stand here.
#pragma once
#include "mf_symbolic.h"
#include <cstddef>
#include <stdexcept>
#include <utility>
#include <vector>

namespace ipcgpu {

// ---- geometry shared by the planner and the kernels (mf_kernels.h adds what only the kernels need)
constexpr int NB = 32; // columns of a panel / of a pivot block
constexpr int ROW_WAVES_B = 3; // row waves per role-B workgroup (1 was measured slower: 3x the workgroups, each repeating the pivot work)
#ifndef MF_ROWS_MT
#define MF_ROWS_MT 2
#endif
constexpr int MT_B = MF_ROWS_MT; // 16-row tiles per row wave of a role-B workgroup
constexpr int ROWS_B = 16 * MT_B * ROW_WAVES_B; // panel rows per role-B workgroup
constexpr int TS = 64; // trailing-update tile
constexpr int TQ = 32; // Schur tile
constexpr int TQ64 = 64; // ... of the levels with many tiles (k_big_schur64, k_big_schur64_ea, k_big_bulk)
constexpr int XCDS = 8; // accelerator complex dies of an MI355X: workgroup b of a launch is observed to run on XCD b % 8
constexpr int MV_ROWS = 32; // rows per workgroup of the forward matrix-vector kernels (k_big_fwd_rect, k_xinv_fwd): 32 rows x 8 column groups
// Host-packed descriptor of a front, 64 ints: everything the kernel would otherwise chase through five rounds of
// dependent loads (front list -> index pointers -> child list -> child pointers -> inverse maps) arrives in one.
//   [0,1] front offset  [2] N  [3] nc  [4,5] first dinv block  [6] aBeg  [7] aEnd  [8] #children in this record  [9] next record of the chain or -1
//   child q at 16 + 6 q: [0,1] front offset  [2] N  [3] nc  [4] offset of its inverse map
// ([4..7] are filled for the fused fronts only, [9] for the chained records of the others.)
constexpr int FD_STRIDE = 64;
constexpr int FUSED_MAX_KIDS = 8;
// Tile records of the two kernels that gather children per 64 x 64 tile (k_extend_add, k_big_schur64_ea): 16 ints = four int4 = one 64-byte line per workgroup,
// so that everything in front of the gathers arrives with the tile's first load:
//   [0] N  [1] nc  [2,3] front offset | [4] ti  [5] tj  [6] #children of the front  [7] first of its records in kidRec
//   child q (0, 1) at 8 + 4 q: [0,1] front offset  [2] N  [3] offset of its row map in childMap   (an absent child: front offset 0, N 0, the map of -1s at offset 0)
// Children 2, 3, ... of a front are read from kidRec (the same four ints each, the front's children in ascending order), one after the other.
// childMap: per (batched front, child) N(parent) + TILE_MAP_PAD ints: parent scalar row I -> scalar row inside the child's front, -1 where the child's structure
// lacks it.  The pad (rows N .. N + 63, all -1) lets a tile that hangs over the front's last row load its indices without a clamp.
constexpr int TILE_REC = 16;
constexpr int TILE_MAP_PAD = 64;

#ifndef MF_BORDER_MAX_NC
#define MF_BORDER_MAX_NC 1536 // (1024 until round 6: the 1 440-column root of the two-sheet contact stack keeps 0.17 ms of doubling rounds behind its factorisation, profiles/r06_border_max_nc_ab.txt)
#endif

struct MfPlanError : std::runtime_error { // a pattern the numeric phase cannot run (MfNumeric reports it as a StateError)
    using std::runtime_error::runtime_error;
};

struct MfRec4 { // one descriptor record: the kernels read it as an int4
    int x, y, z, w;
};

struct MfRange {
    int off = 0, cnt = 0;
};

// Fixed since round 6 (each was an environment switch while it was being measured; the sweeps are profiles/r05_knob_sweep*.txt, r05_two_level_blocking_ab.txt,
// r03r_schur_tile_ab.txt, r04_nd_leaf_size_ab.txt): levels with >= 512 Schur tiles of 32 x 32 take the 64 x 64 kernel (schur64Min); levels whose step launches
// move >= 48 MB of own columns factor them in outer blocks of 256 columns (bulkMinMB, bulkBlock: the only two a caller can set,
// ipcgpu_linsys_set_tuning, because no mesh of the test suite reaches 48 MB and the path has to be forced to be tested; swept at 375 K nodes: 4, 16, 64 MB the
// same, factorisation 17.58 -> 16.9 ms; block 128 the same, 512 half the gain); 64 KB of LDS per fused front.
// The product sets no other field: they are fields so that a CPU test can force every path at a small size.
struct MfPlanTuning {
    size_t fusedLds = 64 * 1024;
    int ntBigN = 200; // levels whose widest fused front has at least this many rows run the fused kernel with 512 threads: one workgroup per CU anyway (LDS)
    int xinvMin = 192; // explicit triangle inverses (see k_xinv_*): fronts of the multi-workgroup path with nc >= xinvMin
    int borderMaxNc = MF_BORDER_MAX_NC; // wider separators (a root of 2 600 columns at 1.12 M tets) keep the recursive doubling: a bordering workgroup is as long as the
                                        // front is wide, and at that width it stretches every step launch (measured at mat433: factorisation 20.0 -> 20.8 ms)
    long long schur64Min = 512; // profiles/r03r_schur_tile_ab.txt
    double bulkMinMB = 48.0; // ipcgpu_linsys_set_tuning "bulk_min_mb"
    int bulkBlock = 256; // width of an outer block; ipcgpu_linsys_set_tuning "bulk_block"
};

struct MfLevelPlan {
    MfRange small; // into smallList
    size_t smallLds = 0, solveLds = 0, triLds = 0, bwdLds = 0;
    int smallThreads = 256; // workgroup size of the fused kernel on this level
    MfRange ea; // extend-add descriptors
    MfRange bigFronts; // into bigList
    std::vector<MfRange> step; // fused factor steps: launch 0 factors panel 0, launch j+1 applies panel j / factors j+1
    std::vector<MfRange> bulk; // per step launch: the bulk updates of the wide fronts that follow it (k_big_bulk; empty ranges elsewhere)
    MfRange schur; // one-pass Schur complement tiles of the big fronts
    int schurTileOff = 0; // fuseEA levels: first of the level's records in schurTile (one per workgroup, in the order of `schur`)
    bool schur64 = false; // ... as 64 x 64 tiles (k_big_schur64) instead of 32 x 32 with the columns split over the waves
    bool stepTop = false; // the level's step launches carry role C, the explicit inverse growing by bordering (k_big_step<true>)
    bool fuseEA = false; // the level's Schur kernel gathers the children of the update block itself (k_big_schur64_ea); the extend-add only writes own columns
    MfRange fwdRect, bwdInit; // descriptors of the row-/column-parallel halves of the big-front solves
    MfRange bigTri; // into triList: big fronts whose triangle is swept by one workgroup (no explicit inverse)
    MfRange xinvFwd, xinvBwd; // into xinvDesc: row / column blocks of the fronts with an explicit inverse
};

struct MfXinvLevel {
    MfRange blocks; // diagonal blocks of the level's inverse fronts (cnt > 0: the level has inverses to form by recursive doubling)
    MfRange init; // into xinvDesc
    std::vector<std::pair<MfRange, MfRange>> rounds; // per doubling: the two GEMM launches (descriptor pairs)
};

struct MfXchgOp { // one send or receive; MfNumeric adds the buffer's base to `off`
    long long off; // in doubles: into the level's staging buffer (opsM, opsW) or into the solution vector (opsX)
    long long count;
    int peer;
    int send;
};
struct MfXchgLevel {
    MfRange pack; // into xchgDesc: (front, staging offset lo, hi, offset of its update vector) of the fronts of this level this rank SENDS to their parent's rank
    MfRange unpack; // ... and of the children (of this level) of fronts this rank executes that it RECEIVES
    std::vector<MfXchgOp> opsM, opsW, opsX; // the level's groups: update matrices (factorisation), update vectors (forward sweep), solution segments (backward sweep)
    long long count = 0; // doubles exchanged after the level's factorisation (update matrices)
    long long countW = 0; // ... and after its forward sweep (update vectors)
};

struct MfPlan {
    int rank = 0, world = 1;
    MfPlanTuning tune;
    // ---- step 1 (mf_plan_fronts)
    std::vector<char> fused; // per front: takes the single-workgroup kernel
    std::vector<MfLevelPlan> level; // (small, bigFronts, schur64, fuseEA after step 1; the rest after step 2)
    std::vector<int> smallList, bigList; // the fronts this rank executes, level after level, in launch order
    std::vector<int> eaTileBase, eaColTiles; // per big front: its first extend-add tile; tiles kept per tile row: min(ti + 1, eaColTiles)
    int nEaTiles = 0;
    std::vector<MfRec4> frontInfo; // per front: (kind: -1 another rank's, 0 single-workgroup, 1 batched; first extend-add tile; tile columns kept per tile row; 0)
    std::vector<int> nodeFront; // per permuted node
    std::vector<long long> dinvOff; // ns + 1: first 32 x 32 inverse block of every front
    // world > 1
    std::vector<int> owner; // per front: owning rank, -1 = above the cut
    std::vector<int> exec; // per front: the rank that factorises and solves it (== owner below the cut)
    std::vector<unsigned long long> group; // per front: ranks that execute a front of its subtree
    double sharedFlops = 0.0;
    std::vector<int> nodeExec; // per permuted node: executing rank
    std::vector<MfRec4> xchgDesc;
    std::vector<MfXchgLevel> xchg;
    long long xchgStaging = 1; // doubles of the largest level's staging area
    // ---- step 2 (mf_plan_launches)
    std::vector<int> aPtr; // ns + 1: entry range of every fused front (the bucket starts of the device sort)
    size_t nFusedA = 0, nBigA = 0; // entries of A of the fused fronts / of the others
    std::vector<int> eaAPtr; // per extend-add tile: first of its entries among the others'
    std::vector<MfRec4> ea; // extend-add tiles (record in bigFd, ti, tj, tile number): the host's list; the kernel reads eaTile
    std::vector<int> bigFd; // packed records of the fronts of the multi-workgroup path (host only since the tile records below: tests read the plan through them)
    // the children of the batched fronts as the tile kernels read them (TILE_REC above): they depend on the pattern alone, like every other array here
    std::vector<int> childMap; // [0, maxN + TILE_MAP_PAD): -1s (the map of an absent child); then the maps, front after front in bigList order, child after child
    std::vector<MfRec4> kidRec; // per (batched front, child): (front offset lo, hi, N, map offset)
    std::vector<int> kidBase; // per front: first of its records in kidRec, -1 for a front that is not batched
    std::vector<int> eaTile; // TILE_REC ints per extend-add tile, in the order of `ea`
    std::vector<int> schurTile; // TILE_REC ints per Schur workgroup of the fuseEA levels
    std::vector<int> fdesc; // packed records of the fused fronts, in launch order
    std::vector<MfRec4> desc; // step, bulk, Schur and sweep descriptors of the big fronts
    std::vector<MfRec4> xinvDesc; // all descriptors of the inverse machinery
    std::vector<MfXinvLevel> xinvLevel;
    std::vector<long long> xinvOff; // per front: offset of X = L11^-1, -1 when it has none
    long long xTot = 0;
    std::vector<int> triList;
    size_t maxSmallLds = 0, maxSolveLds = 0, maxBwdLds = 0, maxTriLds = 0, xinvLds = 8; // dynamic LDS of the widest launch of every kind

    bool mine(int s) const { return world == 1 || exec[s] == rank; }
    bool hasXinv(const MfSymbolic& sym, int s) const { return !fused[s] && sym.nc(s) >= tune.xinvMin; }
    // the inverse grows by bordering inside the step launches (step_border); otherwise by recursive doubling on the side stream (profiles/r05_permlane_and_border_ab.txt)
    bool hasBorder(const MfSymbolic& sym, int s) const { return hasXinv(sym, s) && sym.nc(s) <= tune.borderMaxNc; }
    int eaTileOf(int s, int ti, int tj) const // index of tile (ti, tj) of front s among the extend-add tiles
    {
        const int c = eaColTiles[s];
        return eaTileBase[s] + (ti <= c ? ti * (ti + 1) / 2 : c * (c + 1) / 2 + (ti - c) * c) + tj;
    }
};

// Step 1: classification, per-level order, extend-add tile numbering, frontInfo / nodeFront (what the device sort of A's entries needs), and for world > 1 the
// cut of the tree and the exchange lists.  plan.rank / world / tune are inputs.
void mf_plan_fronts(const MfSymbolic& sym, MfPlan& plan);
// Step 2: everything else.  bucketStart: ns + nEaTiles + 1 exclusive starts of the entries of A sorted by bucket (fused front s: bucket s; the others:
// ns + extend-add tile), as k_entry_dst / k_scan_exclusive leave them.
void mf_plan_launches(const MfSymbolic& sym, const int* bucketStart, MfPlan& plan);

} // namespace ipcgpu
