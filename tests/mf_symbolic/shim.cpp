// TEST INFRASTRUCTURE (host only): the symbolic analysis of the multifrontal solver (ipc_amd/csrc/mf_symbolic.cpp) behind a plain C call, so that
// tests/test_mf_symbolic.py can check its fronts against an independent restatement in Python, and the launch plan of the numeric phase
// (ipc_amd/csrc/mf_plan.cpp) so that tests/test_mf_plan.py can read its records the way the kernels do.  Built by the tests with g++.
#include "../../ipc_amd/csrc/mf_plan.h"
#include "../../ipc_amd/csrc/mf_symbolic.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
using namespace ipcgpu;
static MfSymbolic g_sym;
extern "C" int shim_analyze(int n, const int* ia, const int* ja, const double* coords, int leaf, int* sizes4)
{
    try {
        mf_analyze(n, ia, ja, coords, leaf, g_sym);
    }
    catch (...) {
        return 1;
    }
    sizes4[0] = g_sym.ns;
    sizes4[1] = g_sym.nn;
    sizes4[2] = (int)g_sym.idx.size();
    sizes4[3] = (int)g_sym.child.size();
    return 0;
}
extern "C" void shim_fetch(int* newOf, int* firstNode, int* parent, int* idxPtr, int* idx, int* childPtr, int* child, long long* aDst, int* aFront, long long* frontOff)
{
    auto cp = [](auto* dst, const auto& v) { std::copy(v.begin(), v.end(), dst); };
    cp(newOf, g_sym.newOf);
    cp(firstNode, g_sym.firstNode);
    cp(parent, g_sym.parent);
    cp(idxPtr, g_sym.idxPtr);
    cp(idx, g_sym.idx);
    cp(childPtr, g_sym.childPtr);
    cp(child, g_sym.child);
    cp(aDst, g_sym.aDst);
    cp(aFront, g_sym.aFront);
    cp(frontOff, g_sym.frontOff);
}
// owner of every front (rank, -1 above the cut) and of every node (old numbering) for `world` ranks; returns the share of the flops above the cut
extern "C" double shim_owners(int world, int* frontOwner, int* nodeOwner)
{
    std::vector<int> owner;
    const double shared = mf_assign_owners(g_sym, world, owner);
    std::copy(owner.begin(), owner.end(), frontOwner);
    for (int s = 0; s < g_sym.ns; ++s)
        for (int v = g_sym.firstNode[s]; v < g_sym.firstNode[s + 1]; ++v) nodeOwner[g_sym.oldOf[v]] = owner[s];
    return shared;
}
// round 5: executors, groups and the point-to-point exchange plan of one rank.  level[s] of every front; records of 7 ints:
// (level, kind, front, off lo, off hi, offW, peer), kind 0 = send, 1 = receive (update matrix + vector), 2 = solution segment out, 3 = solution segment in.
// Returns the number of records (-1: more than `cap`).
extern "C" int shim_exchange_plan(int world, int rank, int* exec, unsigned long long* group, int* level, int* rec, int cap)
{
    std::vector<int> owner, ex;
    std::vector<unsigned long long> gr;
    mf_assign_owners(g_sym, world, owner);
    mf_assign_executors(g_sym, owner, ex, gr);
    std::copy(ex.begin(), ex.end(), exec);
    std::copy(gr.begin(), gr.end(), group);
    std::copy(g_sym.level.begin(), g_sym.level.end(), level);
    std::vector<MfExchangeLevel> plan;
    mf_exchange_plan(g_sym, owner, ex, gr, rank, world, plan);
    int n = 0;
    auto put = [&](int l, int kind, const MfExchangeItem& it) {
        if (n < cap) {
            int* r = rec + 7 * n;
            r[0] = l;
            r[1] = kind;
            r[2] = it.front;
            r[3] = (int)(unsigned)(it.off & 0xffffffffll);
            r[4] = (int)(it.off >> 32);
            r[5] = it.offW;
            r[6] = it.peer;
        }
        ++n;
    };
    for (int l = 0; l < (int)plan.size(); ++l) {
        for (const auto& it : plan[l].send) put(l, 0, it);
        for (const auto& it : plan[l].recv) put(l, 1, it);
        for (const auto& it : plan[l].xsSend) put(l, 2, it);
        for (const auto& it : plan[l].xsRecv) put(l, 3, it);
    }
    return n <= cap ? n : -1;
}

// ---- the launch plan of g_sym (both planner steps) for one rank.  tune7 = (fusedLds, ntBigN, xinvMin, borderMaxNc, schur64Min, bulkMinMB, bulkBlock), NaN = the
// default.  The bucket starts step 2 takes are counted here from aFront / aDst the way k_entry_dst buckets the entries (fused front s: bucket s; the others:
// ns + extend-add tile of the entry's slot).  Returns 0, or 1 with the message in err.
static MfPlan g_plan;
static std::vector<int> g_start;
extern "C" int shim_plan(int world, int rank, const double* tune7, char* err, int errCap)
{
    try {
        g_plan = MfPlan();
        g_plan.rank = rank;
        g_plan.world = world;
        MfPlanTuning& t = g_plan.tune;
        if (!std::isnan(tune7[0])) t.fusedLds = (size_t)tune7[0];
        if (!std::isnan(tune7[1])) t.ntBigN = (int)tune7[1];
        if (!std::isnan(tune7[2])) t.xinvMin = (int)tune7[2];
        if (!std::isnan(tune7[3])) t.borderMaxNc = (int)tune7[3];
        if (!std::isnan(tune7[4])) t.schur64Min = (long long)tune7[4];
        if (!std::isnan(tune7[5])) t.bulkMinMB = tune7[5];
        if (!std::isnan(tune7[6])) t.bulkBlock = (int)tune7[6];
        mf_plan_fronts(g_sym, g_plan);
        const int ns = g_sym.ns, nBuckets = ns + g_plan.nEaTiles;
        std::vector<int> count(nBuckets, 0);
        for (size_t k = 0; k < g_sym.aDst.size(); ++k) {
            const int s = g_sym.aFront[k];
            const MfRec4 info = g_plan.frontInfo[s];
            if (info.x < 0) continue;
            if (info.x == 0) {
                count[s]++;
                continue;
            }
            const long long loc = g_sym.aDst[k] - g_sym.frontOff[s];
            const int lr = (int)(loc % g_sym.N(s)), lc = (int)(loc / g_sym.N(s));
            count[ns + g_plan.eaTileOf(s, lr / TS, lc / TS)]++;
        }
        g_start.assign(nBuckets + 1, 0);
        for (int b = 0; b < nBuckets; ++b) g_start[b + 1] = g_start[b] + count[b];
        mf_plan_launches(g_sym, g_start.data(), g_plan);
    }
    catch (const std::exception& e) {
        std::strncpy(err, e.what(), errCap - 1);
        err[errCap - 1] = 0;
        return 1;
    }
    return 0;
}
// one array of the plan (or of g_sym) by name, as 64-bit integers; out == null: only the length.  Records (MfRec4) come as four numbers each; the per-level
// structures are flattened as the comments say.
extern "C" long long shim_plan_fetch(const char* name, long long* out)
{
    const std::string n = name;
    std::vector<long long> v;
    auto ints = [&](const auto& a) { v.assign(a.begin(), a.end()); };
    auto recs = [&](const std::vector<MfRec4>& a) {
        for (const MfRec4& r : a) v.insert(v.end(), { r.x, r.y, r.z, r.w });
    };
    auto range = [&](const MfRange& r) { v.insert(v.end(), { r.off, r.cnt }); };
    auto ops = [&](const std::vector<MfXchgOp>& a) { // count, then (off, count, peer, send) each
        v.push_back((long long)a.size());
        for (const MfXchgOp& o : a) v.insert(v.end(), { o.off, o.count, o.peer, o.send });
    };
    const MfPlan& p = g_plan;
    if (n == "symLevel") ints(g_sym.level);
    else if (n == "symInvPtr") ints(g_sym.invPtr);
    else if (n == "bucketStart") ints(g_start);
    else if (n == "fused") ints(p.fused);
    else if (n == "smallList") ints(p.smallList);
    else if (n == "bigList") ints(p.bigList);
    else if (n == "eaTileBase") ints(p.eaTileBase);
    else if (n == "eaColTiles") ints(p.eaColTiles);
    else if (n == "frontInfo") recs(p.frontInfo);
    else if (n == "nodeFront") ints(p.nodeFront);
    else if (n == "dinvOff") ints(p.dinvOff);
    else if (n == "owner") ints(p.owner);
    else if (n == "exec") ints(p.exec);
    else if (n == "nodeExec") ints(p.nodeExec);
    else if (n == "xchgDesc") recs(p.xchgDesc);
    else if (n == "aPtr") ints(p.aPtr);
    else if (n == "eaAPtr") ints(p.eaAPtr);
    else if (n == "ea") recs(p.ea);
    else if (n == "bigFd") ints(p.bigFd);
    else if (n == "fdesc") ints(p.fdesc);
    else if (n == "desc") recs(p.desc);
    else if (n == "xinvDesc") recs(p.xinvDesc);
    else if (n == "xinvOff") ints(p.xinvOff);
    else if (n == "triList") ints(p.triList);
    else if (n == "scalars")
        v = { p.nEaTiles, p.xTot, (long long)p.nFusedA, (long long)p.nBigA, (long long)p.maxSmallLds, (long long)p.maxSolveLds, (long long)p.maxBwdLds,
            (long long)p.maxTriLds, (long long)p.xinvLds, p.xchgStaging };
    else if (n == "levels") // 30 numbers per level
        for (const MfLevelPlan& P : p.level) {
            range(P.small);
            range(P.bigFronts);
            range(P.ea);
            range(P.schur);
            range(P.fwdRect);
            range(P.bwdInit);
            range(P.bigTri);
            range(P.xinvFwd);
            range(P.xinvBwd);
            v.insert(v.end(), { (long long)P.smallLds, (long long)P.solveLds, (long long)P.triLds, (long long)P.bwdLds, P.smallThreads, P.schur64, P.stepTop, P.fuseEA,
                                  (long long)P.step.size(), 0, 0, 0 });
        }
    else if (n == "steps" || n == "bulks") // per level, per launch: (off, cnt)
        for (const MfLevelPlan& P : p.level)
            for (const MfRange& r : (n == "steps" ? P.step : P.bulk)) range(r);
    else if (n == "xinvLevels") // per level: blocks, init, number of rounds, then both ranges of every round
        for (const MfXinvLevel& X : p.xinvLevel) {
            range(X.blocks);
            range(X.init);
            v.push_back((long long)X.rounds.size());
            for (const auto& r : X.rounds) {
                range(r.first);
                range(r.second);
            }
        }
    else if (n == "xchgLevels") // per level: pack, unpack, count, countW, then the three groups
        for (const MfXchgLevel& X : p.xchg) {
            range(X.pack);
            range(X.unpack);
            v.insert(v.end(), { X.count, X.countW });
            ops(X.opsM);
            ops(X.opsW);
            ops(X.opsX);
        }
    else return -1;
    if (out) std::copy(v.begin(), v.end(), out);
    return (long long)v.size();
}
