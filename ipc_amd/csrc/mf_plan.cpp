// Launch plan of the GPU multifrontal LL^T (see mf_plan.h).  Host only.
#include "mf_plan.h"
#include <algorithm>
#include <climits>
#include <cstring>

namespace ipcgpu {

namespace {

int kidsOf(const MfSymbolic& sym, int s) { return sym.childPtr[s + 1] - sym.childPtr[s]; }

// what the fused kernel keeps in LDS: the nc own columns plus the index maps of the children
size_t ldsOf(const MfSymbolic& sym, int s)
{
    return ((size_t)sym.nc(s) * sym.N(s) + 64) * sizeof(double) + (size_t)kidsOf(sym, s) * sym.N(s) * sizeof(int);
}

// (N, nc, front offset lo, hi): the second record of every two-record descriptor
MfRec4 geometryRec(const MfSymbolic& sym, int s)
{
    const long long foff = sym.frontOff[s];
    return MfRec4{ sym.N(s), sym.nc(s), (int)(unsigned)(foff & 0xffffffffll), (int)(unsigned)(foff >> 32) };
}

// one 64-int record of front s with its children k0 .. k0 + nk (layout: FD_STRIDE in mf_plan.h); the caller fills [4..7] and [9]
int* frontRecord(const MfSymbolic& sym, int s, int k0, int nk, int* d)
{
    const long long off = sym.frontOff[s];
    std::memcpy(d, &off, 8);
    d[2] = sym.N(s);
    d[3] = sym.nc(s);
    d[8] = std::max(nk, 0);
    for (int q = 0; q < nk; ++q) {
        const int c = sym.child[sym.childPtr[s] + k0 + q];
        int* k = d + 16 + 6 * q;
        const long long coff = sym.frontOff[c];
        std::memcpy(k, &coff, 8);
        k[2] = sym.N(c);
        k[3] = sym.nc(c);
        k[4] = sym.invPtr[c];
    }
    return d;
}

const int* bigBegin(const MfPlan& plan, int l) { return plan.bigList.data() + plan.level[l].bigFronts.off; }
const int* bigEnd(const MfPlan& plan, int l) { return bigBegin(plan, l) + plan.level[l].bigFronts.cnt; }
struct BigFronts { // the fronts of the multi-workgroup path of one level, in launch order
    const int *b, *e;
    BigFronts(const MfPlan& plan, int l) : b(bigBegin(plan, l)), e(bigEnd(plan, l)) {}
    const int* begin() const { return b; }
    const int* end() const { return e; }
    bool empty() const { return b == e; }
};

// A front whose nc own columns (plus the index maps of its children) fit into LDS takes the fused single-workgroup path;
// the others go through the level-batched multi-workgroup kernels.
// ... unless its level has fronts of the second kind anyway and only a few of the first (round 5): the single-workgroup kernel of such a level is a launch of
// its own IN FRONT of the level's batched kernels -- 57 us for the 93 widest fused fronts of level 4 of a 45 K-node sheet, one workgroup each at the limit of
// what LDS holds -- while as members of the batched launches the same fronts cost next to nothing (those launches are latency-bound and far from full).
// (profiles/r05_mixed_levels_ab_and_p2p_bytes.txt)
void classifyFronts(const MfSymbolic& sym, MfPlan& plan)
{
    const int nLevels = (int)sym.levelPtr.size() - 1;
    plan.fused.assign(sym.ns, 0);
    std::vector<int> nFit(nLevels, 0), nBigL(nLevels, 0);
    for (int s = 0; s < sym.ns; ++s) {
        plan.fused[s] = kidsOf(sym, s) <= FUSED_MAX_KIDS && ldsOf(sym, s) <= plan.tune.fusedLds;
        (plan.fused[s] ? nFit : nBigL)[sym.level[s]]++;
    }
    for (int s = 0; s < sym.ns; ++s) {
        const int l = sym.level[s];
        if (plan.fused[s] && nBigL[l] > 0 && nFit[l] <= std::max(64, nBigL[l])) plan.fused[s] = 0;
    }
}

// ---- multi-GPU: cut the assembly tree below its top separators (see mf_numeric.h).
// Exchange lists, by level (mf_exchange_plan: fronts whose parent another rank executes, solution segments of the fronts above the cut).  Every
// rank computes the same staging layout; it packs what it sends and unpacks what it receives.
void exchangeLists(const MfSymbolic& sym, MfPlan& plan)
{
    const int nLevels = (int)sym.levelPtr.size() - 1;
    plan.sharedFlops = mf_assign_owners(sym, plan.world, plan.owner);
    mf_assign_executors(sym, plan.owner, plan.exec, plan.group);
    std::vector<MfExchangeLevel> lists;
    mf_exchange_plan(sym, plan.owner, plan.exec, plan.group, plan.rank, plan.world, lists);
    for (const MfExchangeLevel& E : lists) {
        plan.xchgStaging = std::max(plan.xchgStaging, E.count + E.countW);
        // the device descriptor of an update vector carries its offset (matrix area + offW) in ONE 32-bit word (k_xchg_w), the matrices' in two
        if ((long long)E.count + (long long)E.countW > (long long)INT_MAX)
            throw MfPlanError("solver exchange: a level's staging area exceeds 2^31 doubles (the update-vector offsets are 32-bit)");
    }
    plan.xchg.assign(nLevels, MfXchgLevel());
    std::vector<MfRec4>& xd = plan.xchgDesc;
    for (int l = 0; l < nLevels; ++l) {
        MfXchgLevel& X = plan.xchg[l];
        const MfExchangeLevel& E = lists[l];
        X.count = E.count;
        X.countW = E.countW;
        auto emit = [&](const std::vector<MfExchangeItem>& items, MfRange& R, int sendFlag) {
            R.off = (int)xd.size();
            for (const MfExchangeItem& it : items) {
                xd.push_back(MfRec4{ it.front, (int)(unsigned)(it.off & 0xffffffffLL), (int)(it.off >> 32), (int)(E.count + it.offW) }); // vectors sit behind the matrices
                const long long m = sym.N(it.front) - sym.nc(it.front);
                X.opsM.push_back(MfXchgOp{ it.off, m * (m + 1) / 2, it.peer, sendFlag });
                X.opsW.push_back(MfXchgOp{ E.count + it.offW, m, it.peer, sendFlag });
            }
            R.cnt = (int)xd.size() - R.off;
        };
        emit(E.send, X.pack, 1);
        emit(E.recv, X.unpack, 0);
        for (const MfExchangeItem& it : E.xsSend) X.opsX.push_back(MfXchgOp{ 3 * (long long)sym.firstNode[it.front], (long long)sym.nc(it.front), it.peer, 1 });
        for (const MfExchangeItem& it : E.xsRecv) X.opsX.push_back(MfXchgOp{ 3 * (long long)sym.firstNode[it.front], (long long)sym.nc(it.front), it.peer, 0 });
    }
    plan.nodeExec.assign(std::max(sym.nn, 1), 0);
    for (int s = 0; s < sym.ns; ++s)
        for (int v = sym.firstNode[s]; v < sym.firstNode[s + 1]; ++v) plan.nodeExec[v] = plan.exec[s];
}

// The fronts of every level in the order the plans below use them (heaviest first, so that the tail of a level is made of short jobs), the levels whose
// Schur kernel gathers the update block itself (k_big_schur64_ea: their extend-add only writes own columns), and the numbering of the extend-add tiles
// (64 x 64, lower triangle, front after front): the entries of A are sorted by the tile they land in, because the extend-add kernel adds them (round 5).
void orderLevels(const MfSymbolic& sym, MfPlan& plan)
{
    const int nLevels = (int)sym.levelPtr.size() - 1;
    plan.level.assign(nLevels, MfLevelPlan());
    plan.eaTileBase.assign(sym.ns, -1);
    plan.eaColTiles.assign(sym.ns, 0);
    plan.nEaTiles = 0;
    for (int l = 0; l < nLevels; ++l) {
        MfLevelPlan& P = plan.level[l];
        std::vector<int> small, big;
        for (int i = sym.levelPtr[l]; i < sym.levelPtr[l + 1]; ++i) {
            const int s = sym.levelFronts[i];
            if (!plan.mine(s)) continue; // factorised and solved by the rank that executes it
            (plan.fused[s] ? small : big).push_back(s);
        }
        std::sort(small.begin(), small.end(), [&](int a, int b) { return sym.N(a) > sym.N(b) || (sym.N(a) == sym.N(b) && a < b); });
        std::sort(big.begin(), big.end(), [&](int a, int b) { return sym.nc(a) > sym.nc(b) || (sym.nc(a) == sym.nc(b) && a < b); });
        P.small = MfRange{ (int)plan.smallList.size(), (int)small.size() };
        plan.smallList.insert(plan.smallList.end(), small.begin(), small.end());
        P.bigFronts = MfRange{ (int)plan.bigList.size(), (int)big.size() };
        plan.bigList.insert(plan.bigList.end(), big.begin(), big.end());
        long long tiles32 = 0;
        for (int s : big) {
            const long long nt = (sym.N(s) - sym.nc(s) + TQ - 1) / TQ;
            tiles32 += nt * (nt + 1) / 2;
        }
        P.schur64 = P.fuseEA = tiles32 >= plan.tune.schur64Min; // (it thins out the extend-add's tiles and numbers them)
        for (int s : big) {
            const int nt = (sym.N(s) + TS - 1) / TS;
            plan.eaColTiles[s] = P.fuseEA ? (sym.nc(s) + TS - 1) / TS : nt;
            plan.eaTileBase[s] = plan.nEaTiles;
            for (int ti = 0; ti < nt; ++ti) plan.nEaTiles += std::min(ti + 1, plan.eaColTiles[s]);
        }
    }
}

// dynamic LDS and workgroup size of the level's single-workgroup launches
void levelLds(const MfSymbolic& sym, MfPlan& plan, int l)
{
    MfLevelPlan& P = plan.level[l];
    int maxN = 0, maxBelow = 1;
    P.smallLds = 0;
    for (int i = P.small.off; i < P.small.off + P.small.cnt; ++i) {
        const int s = plan.smallList[i];
        maxN = std::max(maxN, sym.N(s));
        P.smallLds = std::max(P.smallLds, ldsOf(sym, s));
    }
    for (int s : BigFronts(plan, l)) maxBelow = std::max(maxBelow, sym.N(s) - sym.nc(s));
    P.smallThreads = maxN >= plan.tune.ntBigN ? 512 : 256; // wide fronts: one workgroup per CU anyway (LDS)
    P.solveLds = (size_t)std::max(maxN, 1) * sizeof(double);
    P.bwdLds = (size_t)maxBelow * sizeof(double);
    plan.maxSmallLds = std::max(plan.maxSmallLds, P.smallLds);
    plan.maxSolveLds = std::max(plan.maxSolveLds, P.solveLds);
    plan.maxBwdLds = std::max(plan.maxBwdLds, P.bwdLds);
}

// packed records of the fronts of the multi-workgroup path: a chain of records of FUSED_MAX_KIDS children each.  Returns front -> its first record.
std::vector<int> packBigFronts(const MfSymbolic& sym, MfPlan& plan)
{
    std::vector<int> recOf(sym.ns, -1);
    std::vector<int>& fd = plan.bigFd;
    for (int s : plan.bigList) {
        recOf[s] = (int)(fd.size() / FD_STRIDE);
        const int nkAll = kidsOf(sym, s);
        for (int k0 = 0; k0 == 0 || k0 < nkAll; k0 += FUSED_MAX_KIDS) {
            const size_t base = fd.size();
            fd.resize(base + FD_STRIDE, 0);
            int* d = frontRecord(sym, s, k0, std::min(FUSED_MAX_KIDS, nkAll - k0), fd.data() + base);
            d[9] = (k0 + FUSED_MAX_KIDS < nkAll) ? (int)(base / FD_STRIDE) + 1 : -1;
        }
    }
    return recOf;
}

// The children of the batched fronts for the tile kernels (TILE_REC in mf_plan.h): per child one map parent scalar row -> child scalar row, which the kernels
// used to derive for every tile from the node map (nc(child) + 3 inv[I / 3] + I % 3), and one record per child.
void childMaps(const MfSymbolic& sym, MfPlan& plan)
{
    int maxN = 0;
    size_t total = 0, kids = 0;
    for (int s : plan.bigList) {
        maxN = std::max(maxN, sym.N(s));
        total += (size_t)kidsOf(sym, s) * (sym.N(s) + TILE_MAP_PAD);
        kids += kidsOf(sym, s);
    }
    total += (size_t)maxN + TILE_MAP_PAD;
    if (total > (size_t)INT_MAX) throw MfPlanError("the child maps of the batched fronts exceed 2^31 entries");
    plan.childMap.assign(total, -1);
    plan.kidRec.clear();
    plan.kidRec.reserve(kids + 1);
    plan.kidBase.assign(sym.ns, -1);
    size_t at = (size_t)maxN + TILE_MAP_PAD;
    for (int s : plan.bigList) {
        plan.kidBase[s] = (int)plan.kidRec.size();
        const int N = sym.N(s);
        for (int q = 0; q < kidsOf(sym, s); ++q) {
            const int c = sym.child[sym.childPtr[s] + q];
            const int* inv = sym.inv.data() + sym.invPtr[c];
            const int ncc = sym.nc(c);
            int* m = plan.childMap.data() + at;
            for (int I = 0; I < N; ++I) {
                const int ic = inv[I / 3];
                if (ic >= 0) m[I] = ncc + 3 * ic + I % 3;
            }
            const long long coff = sym.frontOff[c];
            plan.kidRec.push_back(MfRec4{ (int)(unsigned)(coff & 0xffffffffll), (int)(unsigned)(coff >> 32), sym.N(c), (int)at });
            at += (size_t)N + TILE_MAP_PAD;
        }
    }
    if (plan.kidRec.empty()) plan.kidRec.push_back(MfRec4{ 0, 0, 0, 0 });
}

// the record of tile (ti, tj) of batched front s: the front's geometry and its first two children inline
void pushTileRecord(const MfSymbolic& sym, const MfPlan& plan, int s, int ti, int tj, std::vector<int>& out)
{
    const MfRec4 g = geometryRec(sym, s);
    const int nk = kidsOf(sym, s), base = plan.kidBase[s];
    out.insert(out.end(), { g.x, g.y, g.z, g.w, ti, tj, nk, base });
    for (int q = 0; q < 2; ++q) {
        const MfRec4 k = q < nk ? plan.kidRec[base + q] : MfRec4{ 0, 0, 0, 0 };
        out.insert(out.end(), { k.x, k.y, k.z, k.w });
    }
}

// packed descriptors of the fused fronts, in launch order
void packFusedFronts(const MfSymbolic& sym, MfPlan& plan)
{
    plan.fdesc.assign(std::max<size_t>(plan.smallList.size(), 1) * FD_STRIDE, 0);
    for (size_t i = 0; i < plan.smallList.size(); ++i) {
        const int s = plan.smallList[i];
        int* d = frontRecord(sym, s, 0, kidsOf(sym, s), plan.fdesc.data() + i * FD_STRIDE);
        std::memcpy(d + 4, &plan.dinvOff[s], 8);
        d[6] = plan.aPtr[s];
        d[7] = plan.aPtr[s + 1];
    }
}

// extend-add descriptors: lower-triangular 64 x 64 tiles of the parent, each pointing at the parent's packed record
void extendAddTiles(const MfSymbolic& sym, MfPlan& plan, const std::vector<int>& recOf, int l)
{
    MfLevelPlan& P = plan.level[l];
    std::vector<MfRec4>& ea = plan.ea;
    P.ea.off = (int)ea.size();
    for (int s : BigFronts(plan, l)) { // every lower-triangle tile is written (children sums or zeros): the fronts are never zero-filled
        const int nt = (sym.N(s) + TS - 1) / TS;
        for (int ti = 0; ti < nt; ++ti)
            for (int tj = 0; tj <= ti; ++tj) {
                if (P.fuseEA && TS * tj >= sym.nc(s)) continue; // a tile of the update block alone: the Schur kernel's
                if ((int)ea.size() != plan.eaTileOf(s, ti, tj)) throw MfPlanError("internal: extend-add tiles are not numbered in emission order");
                ea.push_back(MfRec4{ recOf[s], ti, tj, plan.eaTileOf(s, ti, tj) });
                pushTileRecord(sym, plan, s, ti, tj, plan.eaTile);
            }
    }
    P.ea.cnt = (int)ea.size() - P.ea.off;
}

// big-front step descriptors: launch 0 factors panel 0, launch j + 1 applies panel j and factors panel j + 1; behind each the bulk updates it releases
void stepRecords(const MfSymbolic& sym, MfPlan& plan, int l)
{
    MfLevelPlan& P = plan.level[l];
    std::vector<MfRec4>& desc = plan.desc;
    const BigFronts big(plan, l);
    int steps = 0;
    for (int s : big) steps = std::max(steps, (sym.nc(s) + NB - 1) / NB);
    P.step.assign(big.empty() ? 0 : steps + 1, MfRange());
    P.bulk.assign(P.step.size(), MfRange());
    // two-level blocking (k_big_bulk) for the fronts of this level?  What a step launch's rank-32 update reads and writes: the own columns of every front, all rows
    const int OBW = plan.tune.bulkBlock;
    double stepMB = 0.0;
    for (int s : big) stepMB += 8.0e-6 * (double)sym.N(s) * sym.nc(s);
    const bool levelWide = stepMB >= plan.tune.bulkMinMB;
    for (int j = -1; j < steps && !big.empty(); ++j) {
        MfRange& R = P.step[j + 1];
        R.off = (int)desc.size();
        for (int s : big) {
            const int N = sym.N(s), nc = sym.nc(s);
            const int kb = j * NB;
            if (j >= 0 && kb >= nc) continue;
            const int w = (j >= 0) ? std::min(NB, nc - kb) : 0;
            const int kb1 = (j >= 0) ? kb + w : 0;
            const int w1 = (kb1 < nc) ? std::min(NB, nc - kb1) : 0;
            const MfRec4 rec2 = geometryRec(sym, s);
            const int di = (int)plan.dinvOff[s];
            // wide fronts (two-level blocking, k_big_bulk): E = the end of the outer block panel kb belongs to; when the next panel opens a new block, the
            // bulk update launched in front of this step has applied panel kb already
            const bool wide = levelWide && nc >= 2 * OBW;
            const int E = (wide && j >= 0) ? std::min(nc, (kb / OBW + 1) * OBW) : nc;
            const bool applied = wide && j >= 0 && kb1 >= E && kb1 < nc;
            if (w1 > 0)
                for (int r0 = 0; r0 < N - kb1; r0 += ROWS_B) {
                    desc.push_back(MfRec4{ di, j < 0 ? -1 : (applied ? -2 - kb1 : kb), r0, -2 });
                    desc.push_back(rec2);
                }
            if (j >= 0 && plan.hasBorder(sym, s)) { // role C: the rows of panel j of X = L11^-1, one workgroup per column tile up to the diagonal block
                P.stepTop = true;
                // 16-column tiles (32 wide ones made the late steps of the root 20 us long: one CU per tile, k up to nc); c0 == kb: the diagonal block, one copy
                for (int c0 = 0; c0 <= kb; c0 += 16) {
                    desc.push_back(MfRec4{ s, kb, c0, -6 });
                    desc.push_back(rec2);
                }
            }
            if (j >= 0 && !applied) {
                // trailing tiles inside the front's own columns (of a wide front: inside the panel's outer block -- the records carry E in place of nc, which is
                // all role A reads nc for); the Schur complement (columns >= nc) waits for k_big_schur
                const int M0 = kb1 + w1;
                const int ntr = (N - M0 + TS - 1) / TS, ntc = (E - M0 + TS - 1) / TS;
                const MfRec4 recA{ N, E, rec2.z, rec2.w };
                for (int ti = 0; ti < ntr; ++ti)
                    for (int tj = 0; tj <= ti && tj < ntc; ++tj) {
                        desc.push_back(MfRec4{ di, kb, ti, tj });
                        desc.push_back(recA);
                    }
            }
        }
        R.cnt = ((int)desc.size() - R.off) / 2; // workgroups: two records each
        // the bulk updates that have to run BEHIND this launch (it factored panel j + 1): of every wide front whose outer block ends with that panel
        MfRange& U = P.bulk[j + 1];
        U.off = (int)desc.size();
        for (int s : big) {
            const int N = sym.N(s), nc = sym.nc(s);
            const int p0 = (j + 1) * NB, Eb = p0 + NB; // the panel just factored and its end
            if (!levelWide || nc < 2 * OBW || Eb % OBW != 0 || Eb >= nc) continue;
            const MfRec4 rec2 = geometryRec(sym, s);
            const int ntr = (N - Eb + TQ64 - 1) / TQ64, ntc = (nc - Eb + TQ64 - 1) / TQ64;
            for (int ti = 0; ti < ntr; ++ti)
                for (int tj = 0; tj <= ti && tj < ntc; ++tj) {
                    desc.push_back(MfRec4{ OBW, Eb - OBW, ti, tj });
                    desc.push_back(rec2);
                }
        }
        U.cnt = ((int)desc.size() - U.off) / 2;
    }
}

// Schur complement: one pass behind the chain (k_big_schur / k_big_schur64 / k_big_schur64_ea).
// XCD-aware order (round 5): workgroup b of a launch runs on XCD b % 8 (observed, MI355X_MICROARCH.md; a speed assumption only -- any placement is
// correct) and every XCD has its own 4 MB L2.  In front-after-front order the tiles of one front land on all eight XCDs, so each L2 sees the factor
// panels L21 of ALL fronts of the level (25 MB on the 64-front level of a 45 K-node sheet) and every operand load is an L2 miss.  Here the tile rows of
// a front form groups of about total / 8 tiles, the groups are dealt to eight bins (largest first onto the least loaded bin) and slot b of the
// launch takes the next tile of bin b % 8: an XCD works through whole fronts and reads their panels from memory once.
void schurTiles(const MfSymbolic& sym, MfPlan& plan, const std::vector<int>& recOf, int l)
{
    MfLevelPlan& P = plan.level[l];
    std::vector<MfRec4>& desc = plan.desc;
    const BigFronts big(plan, l);
    P.schur.off = (int)desc.size();
    const int TQl = P.schur64 ? TQ64 : TQ;
    struct Tile {
        MfRec4 a, b;
    };
    std::vector<std::vector<Tile>> groups;
    long long total = 0;
    for (int s : big) {
        const long long nt = (sym.N(s) - sym.nc(s) + TQl - 1) / TQl;
        total += nt * (nt + 1) / 2;
    }
    const long long target = std::max<long long>(1, (total + XCDS - 1) / XCDS);
    for (int s : big) {
        const int nt = (sym.N(s) - sym.nc(s) + TQl - 1) / TQl;
        const MfRec4 rec2 = geometryRec(sym, s);
        groups.emplace_back();
        for (int ti = 0; ti < nt; ++ti) {
            if ((long long)groups.back().size() + ti + 1 > target && !groups.back().empty()) groups.emplace_back(); // next row range of a front too large for one bin
            for (int tj = 0; tj <= ti; ++tj) groups.back().push_back(Tile{ MfRec4{ s, ti, tj, P.fuseEA ? recOf[s] : 0 }, rec2 });
        }
    }
    std::vector<int> order(groups.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return groups[a].size() > groups[b].size(); });
    std::vector<std::vector<Tile>> bins(XCDS);
    for (int g : order) {
        int best = 0;
        for (int x = 1; x < XCDS; ++x)
            if (bins[x].size() < bins[best].size()) best = x;
        bins[best].insert(bins[best].end(), groups[g].begin(), groups[g].end());
    }
    std::vector<size_t> head(XCDS, 0), tail(XCDS);
    for (int x = 0; x < XCDS; ++x) tail[x] = bins[x].size();
    for (long long left = total; left > 0;)
        for (int x = 0; x < XCDS && left > 0; ++x, --left) {
            int from = x;
            if (head[x] >= tail[x]) { // this bin has run dry: take from the END of the fullest one (its head keeps its order)
                for (int y = 0; y < XCDS; ++y)
                    if (tail[y] - head[y] > tail[from] - head[from]) from = y;
            }
            const Tile& t = (from == x) ? bins[x][head[x]++] : bins[from][--tail[from]];
            desc.push_back(t.a);
            desc.push_back(t.b);
        }
    P.schur.cnt = ((int)desc.size() - P.schur.off) / 2; // workgroups: two records each
    P.schurTileOff = (int)(plan.schurTile.size() / TILE_REC);
    if (P.fuseEA) // the same workgroups, as the records k_big_schur64_ea reads (tile indices count from nc, as above)
        for (int w = 0; w < P.schur.cnt; ++w) {
            const MfRec4& a = desc[(size_t)P.schur.off + 2 * w];
            pushTileRecord(sym, plan, a.x, a.y, a.z, plan.schurTile);
        }
}

// the row-/column-parallel halves of the big-front solves below the triangle
void rectSweepRecords(const MfSymbolic& sym, MfPlan& plan, int l)
{
    MfLevelPlan& P = plan.level[l];
    std::vector<MfRec4>& desc = plan.desc;
    P.fwdRect.off = (int)desc.size();
    for (int s : BigFronts(plan, l))
        for (int r0 = 0; r0 < sym.N(s) - sym.nc(s); r0 += MV_ROWS) desc.push_back(MfRec4{ s, r0, 0, 0 });
    P.fwdRect.cnt = (int)desc.size() - P.fwdRect.off;
    P.bwdInit.off = (int)desc.size();
    for (int s : BigFronts(plan, l))
        if (sym.N(s) > sym.nc(s))
            for (int c0 = 0; c0 < sym.nc(s); c0 += 16) desc.push_back(MfRec4{ s, c0, 0, 0 });
    P.bwdInit.cnt = (int)desc.size() - P.bwdInit.off;
}

// Which fronts get an explicit inverse and where it lives; per level (the inverses of a level are formed on a side stream while the levels above
// factorise): the diagonal blocks to invert, the copies into X and the doubling rounds of the fronts the step launches do not border
void inversePlan(const MfSymbolic& sym, MfPlan& plan)
{
    const int nLevels = (int)plan.level.size();
    std::vector<MfRec4>& xd = plan.xinvDesc;
    plan.xinvOff.assign(sym.ns, -1);
    plan.xTot = 0;
    size_t maxInvNc = 0;
    for (int s : plan.bigList) {
        if (!plan.hasXinv(sym, s)) continue;
        plan.xinvOff[s] = plan.xTot;
        plan.xTot += (long long)sym.nc(s) * sym.nc(s);
        maxInvNc = std::max<size_t>(maxInvNc, sym.nc(s));
    }
    plan.xinvLds = std::max<size_t>(maxInvNc, 1) * sizeof(double);
    if (plan.xinvLds > 150 * 1024) throw MfPlanError("a separator front is too wide for the inverse-based triangular solve");
    int nBlocks = 0;
    plan.xinvLevel.assign(nLevels, MfXinvLevel());
    for (int l = 0; l < nLevels; ++l) {
        MfXinvLevel& XL = plan.xinvLevel[l];
        std::vector<int> lf;
        for (int s : BigFronts(plan, l))
            if (plan.hasXinv(sym, s) && !plan.hasBorder(sym, s)) lf.push_back(s); // (the step launches build the bordered inverses, step_border)
        XL.blocks.off = nBlocks;
        XL.init.off = (int)xd.size();
        for (int s : lf)
            for (int b = 0; b < (sym.nc(s) + NB - 1) / NB; ++b) xd.push_back(MfRec4{ s, b, 0, 0 });
        XL.init.cnt = (int)xd.size() - XL.init.off;
        XL.blocks.cnt = XL.init.cnt;
        nBlocks += XL.blocks.cnt;
        if ((xd.size() & 1) != 0) xd.push_back(MfRec4{ 0, 0, 0, 0 }); // GEMM descriptors are pairs: keep them pair-aligned
        int lvlMax = 0;
        for (int s : lf) lvlMax = std::max(lvlMax, sym.nc(s));
        for (int sz = NB; sz < lvlMax; sz *= 2) {
            // pairs (A, C) of this doubling: A = [2 p sz, 2 p sz + sz), C = [2 p sz + sz, min(2 p sz + 2 sz, nc))
            MfRange g1, g2;
            for (int mode = 1; mode <= 2; ++mode) {
                MfRange& g = (mode == 1) ? g1 : g2;
                g.off = (int)xd.size() / 2;
                for (int s : lf) {
                    const int nc = sym.nc(s);
                    for (int a0 = 0; a0 + sz < nc; a0 += 2 * sz) {
                        const int c0 = a0 + sz, cEnd = std::min(a0 + 2 * sz, nc);
                        for (int r = c0; r < cEnd; r += 32)
                            for (int c = a0; c < a0 + sz; c += 32) {
                                xd.push_back(MfRec4{ s, r, c, mode });
                                // mode 1 sums over the columns of A, mode 2 over the rows of C
                                xd.push_back(mode == 1 ? MfRec4{ cEnd, a0 + sz, a0, a0 + sz } : MfRec4{ cEnd, a0 + sz, c0, cEnd });
                            }
                    }
                }
                g.cnt = (int)xd.size() / 2 - g.off;
            }
            XL.rounds.push_back({ g1, g2 });
        }
    }
}

// solve: per level the fronts swept by one workgroup (no inverse) and the row / column blocks of the others
void sweepLists(const MfSymbolic& sym, MfPlan& plan)
{
    std::vector<MfRec4>& xd = plan.xinvDesc;
    plan.maxTriLds = 0;
    for (MfLevelPlan& P : plan.level) {
        P.bigTri.off = (int)plan.triList.size();
        size_t triMax = 1;
        std::vector<MfRec4> fw, bw;
        for (int i = P.bigFronts.off; i < P.bigFronts.off + P.bigFronts.cnt; ++i) {
            const int s = plan.bigList[i];
            if (plan.xinvOff[s] < 0) {
                plan.triList.push_back(s);
                triMax = std::max<size_t>(triMax, sym.nc(s));
                continue;
            }
            for (int r0 = 0; r0 < sym.nc(s); r0 += MV_ROWS) fw.push_back(MfRec4{ s, r0, 0, 0 });
            for (int c0 = 0; c0 < sym.nc(s); c0 += 16) bw.push_back(MfRec4{ s, c0, 0, 0 });
        }
        P.bigTri.cnt = (int)plan.triList.size() - P.bigTri.off;
        P.triLds = triMax * sizeof(double);
        plan.maxTriLds = std::max(plan.maxTriLds, P.triLds);
        if ((xd.size() & 1) != 0) xd.push_back(MfRec4{ 0, 0, 0, 0 });
        P.xinvFwd = MfRange{ (int)xd.size(), (int)fw.size() };
        xd.insert(xd.end(), fw.begin(), fw.end());
        P.xinvBwd = MfRange{ (int)xd.size(), (int)bw.size() };
        xd.insert(xd.end(), bw.begin(), bw.end());
    }
}

} // namespace

void mf_plan_fronts(const MfSymbolic& sym, MfPlan& plan)
{
    const int rank = plan.rank, world = plan.world;
    const MfPlanTuning tune = plan.tune;
    plan = MfPlan();
    plan.rank = rank;
    plan.world = world;
    plan.tune = tune;
    classifyFronts(sym, plan);
    plan.owner.assign(sym.ns, rank);
    plan.exec.assign(sym.ns, rank);
    if (world > 1) exchangeLists(sym, plan);
    orderLevels(sym, plan);
    plan.frontInfo.resize(std::max(sym.ns, 1));
    plan.nodeFront.resize(std::max(sym.nn, 1));
    plan.dinvOff.assign(sym.ns + 1, 0);
    for (int s = 0; s < sym.ns; ++s) {
        plan.frontInfo[s] = MfRec4{ !plan.mine(s) ? -1 : (plan.fused[s] ? 0 : 1), plan.eaTileBase[s], plan.eaColTiles[s], 0 };
        for (int v = sym.firstNode[s]; v < sym.firstNode[s + 1]; ++v) plan.nodeFront[v] = s;
        plan.dinvOff[s + 1] = plan.dinvOff[s] + (sym.nc(s) + NB - 1) / NB;
    }
}

void mf_plan_launches(const MfSymbolic& sym, const int* start, MfPlan& plan)
{
    const int ns = sym.ns, nLevels = (int)plan.level.size();
    plan.aPtr.assign(start, start + ns + 1);
    plan.nFusedA = (size_t)start[ns];
    plan.nBigA = (size_t)(start[ns + plan.nEaTiles] - start[ns]);
    plan.eaAPtr.resize((size_t)plan.nEaTiles + 1);
    for (int t = 0; t <= plan.nEaTiles; ++t) plan.eaAPtr[t] = start[ns + t] - start[ns]; // per extend-add tile: its range among the big fronts' entries
    const std::vector<int> recOf = packBigFronts(sym, plan);
    childMaps(sym, plan);
    for (int l = 0; l < nLevels; ++l) {
        levelLds(sym, plan, l);
        extendAddTiles(sym, plan, recOf, l);
        stepRecords(sym, plan, l);
        schurTiles(sym, plan, recOf, l);
        rectSweepRecords(sym, plan, l);
    }
    packFusedFronts(sym, plan);
    inversePlan(sym, plan);
    sweepLists(sym, plan);
    // no array is left empty: every one of them is uploaded and handed to kernels as a pointer
    if (plan.triList.empty()) plan.triList.push_back(0);
    if (plan.xinvDesc.empty()) plan.xinvDesc.push_back(MfRec4{ 0, 0, 0, 0 });
    if (plan.xinvOff.empty()) plan.xinvOff.push_back(-1);
    if (plan.smallList.empty()) plan.smallList.push_back(0);
    if (plan.bigList.empty()) plan.bigList.push_back(0);
    if (plan.ea.empty()) plan.ea.push_back(MfRec4{ 0, 0, 0, 0 });
    if (plan.bigFd.empty()) plan.bigFd.resize(FD_STRIDE, 0);
    if (plan.eaTile.empty()) plan.eaTile.resize(TILE_REC, 0);
    if (plan.schurTile.empty()) plan.schurTile.resize(TILE_REC, 0);
    if (plan.desc.empty()) plan.desc.push_back(MfRec4{ 0, 0, 0, 0 });
    if (plan.world > 1 && plan.xchgDesc.empty()) plan.xchgDesc.push_back(MfRec4{ 0, 0, 0, 0 });
}

} // namespace ipcgpu
