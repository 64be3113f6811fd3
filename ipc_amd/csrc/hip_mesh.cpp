// HipMesh: the Mesh<3> data contract of the hot path, derived on the host once per mesh and uploaded.
#include "hip_ipc.h"
#include <algorithm>
#include <cmath>

namespace ipcgpu {

namespace {
inline double det3(const double X[9])
{
    return X[0] * (X[4] * X[8] - X[7] * X[5]) - X[3] * (X[1] * X[8] - X[7] * X[2]) + X[6] * (X[1] * X[5] - X[4] * X[2]);
}
// inverse of a column-major 3x3 through the adjugate
inline void inv3(const double X[9], double R[9])
{
    const double d = det3(X);
    R[0] = (X[4] * X[8] - X[7] * X[5]) / d;
    R[1] = (X[7] * X[2] - X[1] * X[8]) / d;
    R[2] = (X[1] * X[5] - X[4] * X[2]) / d;
    R[3] = (X[6] * X[5] - X[3] * X[8]) / d;
    R[4] = (X[0] * X[8] - X[6] * X[2]) / d;
    R[5] = (X[3] * X[2] - X[0] * X[5]) / d;
    R[6] = (X[3] * X[7] - X[6] * X[4]) / d;
    R[7] = (X[6] * X[1] - X[0] * X[7]) / d;
    R[8] = (X[0] * X[4] - X[3] * X[1]) / d;
}
} // namespace

void HipMesh::computeFeatures(int nV_, int nT_, const double* Vr, const int* Fc, double YM, double PR, double density,
    hipStream_t s)
{
    if (nV_ <= 0 || nT_ < 0) throw ArgError("set_mesh: bad sizes");
    ++featuresVersion;
    ++nbVersion;
    if (shell.nTri()) shell.plan = ShellPlan(); // the shell belongs to the previous mesh
    shell.limit = ShellLimitPlan(); // ... and its strain limit with it
    shell.rubber = ShellRubberPlan(); // ... and its rubber membrane
    shell.weave = ShellWeavePlan(); // ... and its woven cloth
    shell.plastic.drop(); // ... and its plastic parameters and history
    if (rod.nSeg()) rod.plan = RodPlan(); // ... and so does the rod
    if (attach.n()) attach.plan = AttachPlan(); // ... and so do the attachments
    if (chamber.n()) chamber.plan = ChamberPlan(); // ... and the pressure chambers
    chamber.gas = ChamberGas(); // ... with their gas law
    if (aero.n()) aero.drop(); // ... and the aerodynamic surfaces
    if (plastic.allocated()) plastic.drop(); // ... and the plastic parameters and history
    if (fiber.plan.nT) fiber.drop(); // ... and the fibres
    nV = nV_;
    nT = nT_;
    V_rest.assign(Vr, Vr + 3 * (size_t)nV);
    F.assign(Fc, Fc + 4 * (size_t)nT);
    for (size_t i = 0; i < F.size(); ++i)
        if (F[i] < 0 || F[i] >= nV) throw ArgError("set_mesh: tetrahedron index out of range");
    dbcType.assign(nV, 0);
    restTriInv.assign(9 * (size_t)nT, 0.0);
    triArea.assign(nT, 0.0);
    mass.assign(nV, 0.0);
    std::vector<std::pair<int, int>> edges;
    edges.reserve(12 * (size_t)nT);
    double edgeSum = 0.0;
    auto X = [&](int v, int c) { return Vr[v + (size_t)nV * c]; };
    for (int t = 0; t < nT; ++t) {
        const int v[4] = { Fc[t], Fc[t + (size_t)nT], Fc[t + 2 * (size_t)nT], Fc[t + 3 * (size_t)nT] };
        double X0[9], A[9];
        for (int k = 0; k < 3; ++k)
            for (int i = 0; i < 3; ++i) X0[i + 3 * k] = X(v[k + 1], i) - X(v[0], i);
        inv3(X0, A); // restTriInv = X0^-1 (Mesh.cpp:449)
        for (int k = 0; k < 9; ++k) restTriInv[(size_t)k * nT + t] = A[k];
        const double d = det3(X0);
        triArea[t] = d / 3 / 2; // Mesh.cpp:455
        const double vol = std::fabs(d) / 6.0; // Mesh.cpp:255-266
        for (int k = 0; k < 4; ++k) mass[v[k]] += vol / 4.0;
        for (int a = 0; a < 4; ++a)
            for (int b = a + 1; b < 4; ++b) {
                edges.emplace_back(v[a], v[b]);
                edges.emplace_back(v[b], v[a]);
            }
        for (int a = 0; a < 4; ++a) { // igl::avg_edge_length walks the columns cyclically: edges (0,1) (1,2) (2,3) (3,0)
            const int b = (a + 1) % 4;
            double l2 = 0;
            for (int i = 0; i < 3; ++i) {
                const double dd = X(v[a], i) - X(v[b], i);
                l2 += dd * dd;
            }
            edgeSum += std::sqrt(l2);
        }
    }
    // Mesh.cpp:460: the mean over four of the six edges of every tetrahedron (what libigl's avg_edge_length computes for a
    // 4-column F); a third of it is the cell size of the reference's spatial hash, which caps the full-CCD step (SpatialHash.hpp:603-618)
    avgEdgeLen = nT ? edgeSum / (4.0 * nT) : 0.0;
    for (int v = 0; v < nV; ++v) mass[v] *= density; // Mesh.cpp:399
    this->density = density;
    mu.assign(nT, YM / 2.0 / (1.0 + PR)); // Mesh.cpp:663-664
    lam.assign(nT, YM * PR / (1.0 + PR) / (1.0 - 2.0 * PR));
    // vNeighbor (Mesh.cpp:470-479); the surface triangles join in addSurfaceEdges
    std::sort(edges.begin(), edges.end());
    edges.erase(std::unique(edges.begin(), edges.end()), edges.end());
    nbPtr.assign(nV + 1, 0);
    for (auto& e : edges) nbPtr[e.first + 1]++;
    for (int v = 0; v < nV; ++v) nbPtr[v + 1] += nbPtr[v];
    nb.resize(edges.size());
    for (size_t i = 0; i < edges.size(); ++i) nb[i] = edges[i].second;
    // bounding box of the simulated material (Mesh::matSpaceBBoxSize2): nodes of elements only -- a kinematic obstacle riding
    // along as a surface-only component must not change dHat = dHatEps^2 * diagonal^2.  (Surface-only components that DO belong
    // to the mesh are declared afterwards: setCodimNodes.)
    inMesh.assign(nV, 0);
    for (int t = 0; t < nT; ++t)
        for (int k = 0; k < 4; ++k) inMesh[F[t + (size_t)nT * k]] = 1;
    meshBBox();
    // upload
    std::vector<double> aos(3 * (size_t)nV);
    for (int v = 0; v < nV; ++v)
        for (int c = 0; c < 3; ++c) aos[3 * (size_t)v + c] = X(v, c);
    d_x.upload(aos, s);
    d_xTilde.upload(aos, s);
    d_mass.upload(mass, s);
    d_A.upload(restTriInv, s);
    d_vol.upload(triArea, s);
    d_mu.upload(mu, s);
    d_lam.upload(lam, s);
    std::vector<int4> tets(nT);
    for (int t = 0; t < nT; ++t) tets[t] = make_int4(Fc[t], Fc[t + (size_t)nT], Fc[t + 2 * (size_t)nT], Fc[t + 3 * (size_t)nT]);
    d_tet.upload(tets.data(), tets.size(), s);
    uploadDBC(s);
    HIP_CHECK(hipStreamSynchronize(s));
}

void HipMesh::meshBBox()
{
    nElemNodes = 0;
    for (int v = 0; v < nV; ++v) nElemNodes += inMesh[v];
    bboxDiag2 = 0;
    for (int c = 0; c < 3; ++c) {
        double lo = 1e300, hi = -1e300;
        for (int v = 0; v < nV; ++v) {
            if (nElemNodes && !inMesh[v]) continue;
            lo = std::min(lo, V_rest[v + (size_t)nV * c]);
            hi = std::max(hi, V_rest[v + (size_t)nV * c]);
        }
        bboxLo[c] = lo;
        bboxHi[c] = hi;
        bboxDiag2 += (hi - lo) * (hi - lo);
    }
}

void HipMesh::setCodimNodes(int n, const int* ids, const double* nodeMass, hipStream_t s)
{
    for (int i = 0; i < n; ++i) {
        if (ids[i] < 0 || ids[i] >= nV) throw ArgError("set_codim_nodes: node id out of range");
        if (!(nodeMass[i] >= 0.0)) throw ArgError("set_codim_nodes: negative mass");
    }
    // Nodes of Mesh<3> with their lumped area masses; the Optimizer's bounding box and mean mass (matSpaceBBoxSize2(dim),
    // avgNodeMass(dim): Mesh.cpp:576-637, Optimizer.cpp:101, 2220, 2232) run over the components of codimension 3 only, so these
    // nodes stay out of both.
    for (int i = 0; i < n; ++i) mass[ids[i]] = nodeMass[i];
    meshBBox();
    d_mass.upload(mass, s);
    HIP_CHECK(hipStreamSynchronize(s));
}

void HipMesh::addNeighbourPairs(const std::vector<int>& pairs)
{
    ++nbVersion;
    std::vector<std::pair<int, int>> edges;
    edges.reserve(nb.size() + pairs.size());
    for (int v = 0; v < nV; ++v)
        for (int k = nbPtr[v]; k < nbPtr[v + 1]; ++k) edges.emplace_back(v, nb[k]);
    for (size_t i = 0; i + 1 < pairs.size(); i += 2) {
        edges.emplace_back(pairs[i], pairs[i + 1]);
        edges.emplace_back(pairs[i + 1], pairs[i]);
    }
    std::sort(edges.begin(), edges.end());
    edges.erase(std::unique(edges.begin(), edges.end()), edges.end());
    if (edges.size() != nb.size()) {
        nbPtr.assign(nV + 1, 0);
        for (auto& e : edges) nbPtr[e.first + 1]++;
        for (int v = 0; v < nV; ++v) nbPtr[v + 1] += nbPtr[v];
        nb.resize(edges.size());
        for (size_t i = 0; i < edges.size(); ++i) nb[i] = edges[i].second;
    }
}

void HipMesh::replaceBodyMasses(const std::vector<char>* oldNodes, std::vector<double>& massBefore, const std::vector<char>& newNodes, const std::vector<double>& newMass)
{
    if (oldNodes) // the body this call replaces or removes: its nodes go back to what they were
        for (int v = 0; v < nV; ++v)
            if ((*oldNodes)[v]) {
                mass[v] = massBefore[v];
                inMesh[v] = 0;
            }
    massBefore = mass;
    for (int v = 0; v < nV; ++v)
        if (newNodes[v]) {
            mass[v] = newMass[v];
            inMesh[v] = 1;
        }
}

void HipMesh::setShell(int nTri, const int* tri, const double* thickness, const double* YM, const double* PR, const double* rho, double bendScale, hipStream_t s)
{
    if (nTri == 0 && shell.nTri() == 0) return; // nothing to remove: no state changes at all
    if (!(bendScale >= 0.0)) throw ArgError("set_shell: bendScale must not be negative");
    ShellPlan plan;
    std::string err;
    if (!buildShellPlan(nV, nTri, tri, V_rest.data(), thickness, YM, PR, rho, nT, F.data(), plan, err)) throw ArgError(err);
    if (rod.nSeg())
        for (int v = 0; v < nV; ++v)
            if (plan.isShellNode[v] && rod.plan.isRodNode[v]) throw ArgError("set_shell: shell node " + std::to_string(v) + " belongs to a rod segment");
    if (shell.nTri()) avgEdgeLen = shell.avgEdgeLenBefore; // (the shell this call replaces or removes)
    shell.avgEdgeLenBefore = avgEdgeLen;
    replaceBodyMasses(shell.nTri() ? &shell.plan.isShellNode : nullptr, shell.massBefore, plan.isShellNode, plan.mass);
    meshBBox();
    if (nT == 0 && nTri) avgEdgeLen = plan.edgeLenSum / (3.0 * nTri);
    // the plan's pairs join vNeighbor: triangle edges (addSurfaceEdges adds the same ones) and the opposite pair of every hinge
    addNeighbourPairs(plan.pairs);
    shell.plan = std::move(plan);
    shell.limit = ShellLimitPlan(); // a strain limit belongs to the shell it was set on
    shell.rubber = ShellRubberPlan(); // ... and so does a rubber membrane (d_triConst below is the new plan's own)
    shell.weave = ShellWeavePlan(); // ... and a woven cloth (d_triConst and row 1 of d_hingeConst below are the new plan's own)
    shell.plastic.drop(); // ... and the plastic parameters and history (d_triConst and d_hingeConst below are the new plan's own)
    shell.bendScale = bendScale;
    const ShellPlan& p = shell.plan;
    d_mass.upload(mass, s);
    shell.d_tri.upload(p.tri, s);
    shell.d_triConst.upload(p.triConst, s);
    std::vector<int4> h4((size_t)p.nHinge);
    std::vector<double> hc(2 * (size_t)p.nHinge);
    for (int i = 0; i < p.nHinge; ++i) {
        h4[i] = make_int4(p.hinge[4 * (size_t)i], p.hinge[4 * (size_t)i + 1], p.hinge[4 * (size_t)i + 2], p.hinge[4 * (size_t)i + 3]);
        hc[i] = p.restAngle[i];
        hc[(size_t)p.nHinge + i] = bendScale * p.hingeK[i] * p.hingeWeight[i];
    }
    shell.d_hinge.upload(h4.data(), h4.size(), s);
    shell.d_hingeConst.upload(hc, s);
    if (!d_codimErr.n) { // the first shell or rod of this mesh
        d_codimErr.alloc(1);
        d_codimErr.zero(s);
    }
    HIP_CHECK(hipStreamSynchronize(s));
}

void HipMesh::setShellStrainLimit(const double* limit, const double* onset, const double* stiff, hipStream_t s)
{
    if (!shell.nTri()) throw StateError("shell_set_strain_limit: no shell is set (call ipcgpu_set_shell first)");
    ShellLimitPlan plan;
    std::string err;
    if (!buildShellLimitPlan(shell.nTri(), limit, onset, stiff, shell.plan.membraneK.data(), plan, err)) throw ArgError(err);
    shell.limit = std::move(plan);
    shell.limitUnchecked = shell.limit.nLimited > 0;
    if (!shell.limit.nLimited) return;
    shell.d_limTri.upload(shell.limit.tri, s);
    shell.d_limConst.upload(shell.limit.limConst, s);
    shell.d_triLimit.upload(shell.limit.triLimit, s);
    HIP_CHECK(hipStreamSynchronize(s));
}

void HipMesh::uploadShellTriConst(hipStream_t s)
{
    // (the shell plan's own once the last rubber and the last woven triangle are gone)
    std::vector<double> triConst = shellTriConstWithoutWeave(shellTriConstWithoutRubber(shell.plan.triConst, shell.rubber), shell.weave);
    if (shell.plastic.allocated()) // rows 0-3 on the device may have flowed: they stay what they are, rows 4-5 alone are new
        shell.d_triConst.download(triConst.data(), 4 * (size_t)shell.nTri(), s);
    shell.d_triConst.upload(triConst, s);
}

void HipMesh::setShellMembrane(const int* model, const double* alpha, hipStream_t s)
{
    if (!shell.nTri()) throw StateError("shell_set_membrane: no shell is set (call ipcgpu_set_shell first)");
    ShellRubberPlan plan;
    std::string err;
    if (!buildShellRubberPlan(shell.nTri(), model, alpha, shell.plan.membraneK.data(), plan, err)) throw ArgError(err);
    if (!plan.nRubber && !shell.rubber.nRubber) return; // StVK before and after: nothing is touched
    for (int t : plan.tri) // (shell_plastic_kernels.h: rows 4 and 5 of a rubber triangle are zero, its strain norm has no meaning)
        if (shellPlasticTriOn(shell.plastic.plan, t)) throw UnsupportedError("shell_set_membrane: rubber on a plastic triangle (triangle " + std::to_string(t) + ")");
    if (shell.nWoven())
        for (int t : plan.tri)
            if (shell.weave.woven[(size_t)t]) throw UnsupportedError("shell_set_membrane: rubber on a woven triangle (triangle " + std::to_string(t) + ")");
    shell.rubber = std::move(plan);
    shell.rubberUnchecked = shell.rubber.nRubber > 0;
    uploadShellTriConst(s);
    if (shell.rubber.nRubber) {
        shell.d_rubTri.upload(shell.rubber.tri, s);
        shell.d_rubConst.upload(shell.rubber.rubConst, s);
    }
    HIP_CHECK(hipStreamSynchronize(s));
}

void HipMesh::setShellWeave(const int* woven, const double* dir, const double* E1, const double* E2, const double* G12, const double* nu12, const double* bendWarp,
    const double* bendWeft, hipStream_t s)
{
    if (!shell.nTri()) throw StateError("shell_set_weave: no shell is set (call ipcgpu_set_shell first)");
    ShellWeavePlan plan;
    std::string err;
    if (!buildShellWeavePlan(shell.plan, nV, V_rest.data(), woven, dir, E1, E2, G12, nu12, bendWarp, bendWeft, plan, err)) throw ArgError(err);
    if (!plan.nWoven && !shell.weave.nWoven) return; // no woven triangle before and after: nothing is touched
    // (flow rewrites Dm^-1, and a, b would stop being orthonormal in the new rest metric; a rubber triangle has its own membrane law)
    for (int t : plan.tri) {
        if (shell.nRubber() && shell.rubber.model[(size_t)t]) throw UnsupportedError("shell_set_weave: triangle " + std::to_string(t) + " carries the rubber membrane");
        if (shellPlasticTriOn(shell.plastic.plan, t)) throw UnsupportedError("shell_set_weave: triangle " + std::to_string(t) + " is plastic");
    }
    shell.weave = std::move(plan);
    uploadShellTriConst(s);
    const std::vector<double> k = shellHingeStiffnessWithWeave(shell.plan, shell.bendScale, shell.weave); // (the plan's own once the last woven triangle is gone)
    if (!k.empty()) // row 1 alone: row 0, the rest angles, may have flowed
        HIP_CHECK(hipMemcpyAsync(shell.d_hingeConst.p + k.size(), k.data(), k.size() * sizeof(double), hipMemcpyHostToDevice, s));
    if (shell.weave.nWoven) {
        shell.d_wovTri.upload(shell.weave.tri, s);
        shell.d_wovConst.upload(shell.weave.wovConst, s);
    }
    HIP_CHECK(hipStreamSynchronize(s)); // (k leaves scope)
}

void HipMesh::uploadShellPlasticParams(hipStream_t s)
{
    HipShellPlastic& h = shell.plastic;
    h.d_yield.upload(h.plan.yield, s);
    h.d_creep.upload(h.plan.creep, s);
    h.d_harden.upload(h.plan.harden, s);
    h.d_hYield.upload(h.plan.hingeYield, s);
    h.d_hCreep.upload(h.plan.hingeCreep, s);
    h.d_hHarden.upload(h.plan.hingeHarden, s);
    h.d_hG.upload(h.plan.hingeG, s);
    HIP_CHECK(hipStreamSynchronize(s));
}

void HipMesh::ensureShellPlastic(hipStream_t s)
{
    HipShellPlastic& h = shell.plastic;
    if (h.allocated()) return;
    if (!shell.nTri()) throw StateError("shell_set_plasticity: no shell is set (call ipcgpu_set_shell first)");
    std::string err;
    if (!setShellPlasticRange(h.plan, shell.plan, nV, V_rest.data(), nullptr, 0, 0, INFINITY, INFINITY, INFINITY, 0.0, err)) throw ArgError(err); // everything elastic
    const size_t nTri = (size_t)shell.nTri(), nH = (size_t)shell.nHinge();
    uploadShellPlasticParams(s);
    std::vector<double> hA(nTri);
    for (size_t t = 0; t < nTri; ++t) hA[t] = shell.plan.thickness[t] * shell.plan.area[t];
    h.d_hA.upload(hA, s);
    h.d_alpha.alloc(nTri);
    h.d_alpha.zero(s);
    h.d_alphaB.alloc(nH);
    h.d_alphaB.zero(s);
    h.d_count.alloc(SPC_COUNT);
    h.d_count.zero(s);
    h.d_totals.alloc(SPT_COUNT);
    h.d_totals.zero(s);
    h.d_B0.alloc(4 * nTri);
    HIP_CHECK(hipMemcpyAsync(h.d_B0.p, shell.d_triConst.p, 4 * nTri * sizeof(double), hipMemcpyDeviceToDevice, s));
    h.d_thetaBar0.alloc(nH);
    if (nH) HIP_CHECK(hipMemcpyAsync(h.d_thetaBar0.p, shell.d_hingeConst.p, nH * sizeof(double), hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s)); // (hA leaves scope)
}

void HipMesh::setShellPlasticity(int triBegin, int triEnd, double yield, double bendYield, double creep, double harden, hipStream_t s)
{
    if (!shell.nTri()) throw StateError("shell_set_plasticity: no shell is set (call ipcgpu_set_shell first)");
    ShellPlasticPlan next = shell.plastic.plan; // a refused call changes nothing
    std::string err;
    if (!setShellPlasticRange(next, shell.plan, nV, V_rest.data(), nullptr, triBegin, triEnd, yield, bendYield, creep, harden, err)) throw ArgError(err);
    if (shell.nRubber() && (yield < INFINITY || bendYield < INFINITY)) // (the plan refuses a rubber triangle too when handed the models; here it is its own error class)
        for (int t = triBegin; t < triEnd; ++t)
            if (shell.rubber.model[t]) throw UnsupportedError("shell_set_plasticity: triangle " + std::to_string(t) + " carries the rubber membrane");
    if (shell.nWoven() && (yield < INFINITY || bendYield < INFINITY)) // (flow rewrites Dm^-1: the warp and weft directions would stop being orthonormal in the new rest metric)
        for (int t = triBegin; t < triEnd; ++t)
            if (shell.weave.woven[t]) throw UnsupportedError("shell_set_plasticity: triangle " + std::to_string(t) + " is woven");
    ensureShellPlastic(s);
    shell.plastic.plan = std::move(next);
    uploadShellPlasticParams(s);
}

void HipMesh::setRod(int nSeg, const int* seg, const double* radius, const double* YM, const double* rho, double bendScale, hipStream_t s)
{
    if (nSeg == 0 && rod.nSeg() == 0) return; // nothing to remove: no state changes at all
    if (!(bendScale >= 0.0)) throw ArgError("set_rod: bendScale must not be negative");
    RodPlan plan;
    std::string err;
    if (!buildRodPlan(nV, nSeg, seg, V_rest.data(), radius, YM, rho, nT, F.data(), shell.nTri(), shell.plan.tri.data(), plan, err)) throw ArgError(err);
    if (rod.nSeg() && rod.ownsAvgEdgeLen) { // (the rod this call replaces or removes)
        // (a shell set after this rod took the rod's mean length for the value to put back: it gets the one from before the rod)
        if (shell.nTri()) shell.avgEdgeLenBefore = rod.avgEdgeLenBefore;
        else avgEdgeLen = rod.avgEdgeLenBefore;
    }
    rod.avgEdgeLenBefore = avgEdgeLen;
    replaceBodyMasses(rod.nSeg() ? &rod.plan.isRodNode : nullptr, rod.massBefore, plan.isRodNode, plan.mass);
    meshBBox();
    rod.ownsAvgEdgeLen = nT == 0 && shell.nTri() == 0 && nSeg > 0;
    if (rod.ownsAvgEdgeLen) avgEdgeLen = plan.lenSum / nSeg;
    // the plan's pairs join vNeighbor: the segments (addSurfaceEdges adds the same ones) and the outer pair (a, c) of every bending triple
    addNeighbourPairs(plan.pairs);
    rod.plan = std::move(plan);
    rod.bendScale = bendScale;
    const RodPlan& p = rod.plan;
    d_mass.upload(mass, s);
    std::vector<int2> s2((size_t)p.nSeg);
    for (int i = 0; i < p.nSeg; ++i) s2[i] = make_int2(p.seg[2 * (size_t)i], p.seg[2 * (size_t)i + 1]);
    rod.d_seg.upload(s2.data(), s2.size(), s);
    rod.d_segConst.upload(p.segConst, s);
    std::vector<int> b3(3 * (size_t)p.nBend);
    std::vector<double> bc((size_t)p.nBend);
    for (int i = 0; i < p.nBend; ++i) {
        for (int k = 0; k < 3; ++k) b3[(size_t)k * p.nBend + i] = p.bend[3 * (size_t)i + k];
        bc[i] = bendScale * p.bendK[i];
    }
    rod.d_bend.upload(b3, s);
    rod.d_bendConst.upload(bc, s);
    if (!d_codimErr.n) { // the first shell or rod of this mesh
        d_codimErr.alloc(1);
        d_codimErr.zero(s);
    }
    HIP_CHECK(hipStreamSynchronize(s));
}

void HipMesh::setAttachments(int n, const int* nodesA, const double* weightsA, const int* nodesB, const double* weightsB, const double* k, const double* L, hipStream_t s)
{
    if (n == 0 && attach.n() == 0) return; // nothing to remove: no state changes at all
    AttachPlan plan;
    std::string err;
    if (!buildAttachPlan(nV, n, nodesA, weightsA, nodesB, weightsB, k, L, plan, err)) throw ArgError(err);
    // The plan's pairs join vNeighbor: every pair among the (up to six) nodes of an attachment.  The pairs of the set this call replaces or removes
    // leave it again where nothing else has touched vNeighbor since (then a context is, to the bit, what it was without them); otherwise they stay.
    if (attach.n() && attach.nbVersionAfter == nbVersion) {
        nbPtr = attach.nbPtrBefore;
        nb = attach.nbBefore;
    }
    attach.nbPtrBefore = nbPtr;
    attach.nbBefore = nb;
    addNeighbourPairs(plan.pairs);
    attach.nbVersionAfter = nbVersion;
    attach.plan = std::move(plan);
    if (!attach.n()) return;
    const AttachPlan& p = attach.plan;
    attach.d_node.upload(p.node, s);
    attach.d_coef.upload(p.coef, s);
    attach.d_kL.upload(p.kL, s);
    if (!d_codimErr.n) { // the first codimensional term of this mesh
        d_codimErr.alloc(1);
        d_codimErr.zero(s);
    }
    HIP_CHECK(hipStreamSynchronize(s));
}

void HipMesh::setChambers(int nCh, const int* triEnd, const int* tri, const double* pressure, hipStream_t s)
{
    if (nCh == 0 && chamber.n() == 0) return; // nothing to remove: no state changes at all
    ChamberPlan plan;
    std::string err;
    if (!buildChamberPlan(nV, V_rest.data(), nCh, triEnd, tri, pressure, plan, err)) throw ArgError(err);
    // The plan's pairs (the triangle edges) join vNeighbor.  As with the attachments, the pairs of the set this call replaces or removes leave it again
    // where nothing else has touched vNeighbor since (then a context is, to the bit, what it was without them); otherwise they stay.
    if (chamber.n() && chamber.nbVersionAfter == nbVersion) {
        nbPtr = chamber.nbPtrBefore;
        nb = chamber.nbBefore;
    }
    chamber.nbPtrBefore = nbPtr;
    chamber.nbBefore = nb;
    addNeighbourPairs(plan.pairs);
    chamber.nbVersionAfter = nbVersion;
    chamber.plan = std::move(plan);
    chamber.gas = ChamberGas(); // the gas law belonged to the chambers this call replaces
    if (!chamber.n()) return;
    const ChamberPlan& p = chamber.plan;
    chamber.d_tri.upload(p.tri, s);
    chamber.d_chamberOf.upload(p.chamberOf, s);
    chamber.d_triEnd.upload(p.triEnd, s);
    chamber.d_pressure.upload(p.pressure, s);
    chamber.d_ref.upload(p.restRef, s);
    if (!d_codimErr.n) { // the first codimensional term of this mesh
        d_codimErr.alloc(1);
        d_codimErr.zero(s);
    }
    HIP_CHECK(hipStreamSynchronize(s));
}

void HipMesh::setAero(int nSurf, const int* triEnd, const int* tri, const double* cn, const double* ct, const int* oneSided, hipStream_t s)
{
    if (nSurf == 0 && aero.n() == 0) return; // nothing to remove: no state changes at all
    AeroPlan plan;
    std::string err;
    if (!buildAeroPlan(nV, V_rest.data(), nSurf, triEnd, tri, cn, ct, oneSided, plan, err)) throw ArgError(err);
    // The plan's pairs (the triangle edges) join vNeighbor; those of the set this call replaces or removes leave it again where nothing else has touched
    // vNeighbor since (setChambers)
    if (aero.n() && aero.nbVersionAfter == nbVersion) {
        nbPtr = aero.nbPtrBefore;
        nb = aero.nbBefore;
    }
    aero.nbPtrBefore = nbPtr;
    aero.nbBefore = nb;
    addNeighbourPairs(plan.pairs);
    aero.nbVersionAfter = nbVersion;
    if (!plan.n) {
        aero.drop();
        return;
    }
    aero.plan = std::move(plan);
    const AeroPlan& p = aero.plan;
    aero.d_tri.upload(p.tri, s);
    aero.d_surfOf.upload(p.surfOf, s);
    aero.d_coef.upload(p.coef, s);
    aero.d_lagged.upload(p.restRecord, s);
    if (!d_codimErr.n) { // the first codimensional term of this mesh
        d_codimErr.alloc(1);
        d_codimErr.zero(s);
    }
    HIP_CHECK(hipStreamSynchronize(s));
}

void HipMesh::setAeroWind(const double* wind3, double density)
{
    if (!wind3 || !std::isfinite(wind3[0]) || !std::isfinite(wind3[1]) || !std::isfinite(wind3[2])) throw ArgError("aero_set_wind: the wind is not finite");
    if (!(density > 0.0) || !std::isfinite(density)) throw ArgError("aero_set_wind: the air density must be positive and finite");
    if (!aero.n()) return;
    for (int a = 0; a < 3; ++a) aero.wind[a] = wind3[a];
    aero.density = density;
}

void HipMesh::ensurePlastic(hipStream_t s)
{
    if (plastic.allocated()) return;
    std::string err;
    if (!setPlasticRange(plastic.plan, nT, 0, 0, INFINITY, INFINITY, 0.0, err)) throw ArgError(err); // every element elastic
    const size_t n = (size_t)nT;
    plastic.d_yield.upload(plastic.plan.yield, s);
    plastic.d_creep.upload(plastic.plan.creep, s);
    plastic.d_harden.upload(plastic.plan.harden, s);
    plastic.d_alpha.alloc(n);
    plastic.d_alpha.zero(s);
    plastic.d_count.alloc(PC_COUNT);
    plastic.d_count.zero(s);
    plastic.d_totals.alloc(PT_COUNT);
    plastic.d_totals.zero(s);
    plastic.d_A0.alloc(9 * n);
    HIP_CHECK(hipMemcpyAsync(plastic.d_A0.p, d_A.p, 9 * n * sizeof(double), hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
}

void HipMesh::setPlasticity(int tetBegin, int tetEnd, double yield, double creep, double harden, hipStream_t s)
{
    PlasticPlan next = plastic.plan; // a refused call changes nothing
    std::string err;
    if (!setPlasticRange(next, nT, tetBegin, tetEnd, yield, creep, harden, err)) throw ArgError(err);
    if (fiber.n() && yield < INFINITY) // (fiber_kernels.h: the rest shape of a fibred element must not flow under b = A_t a)
        for (int t = tetBegin; t < tetEnd; ++t)
            if (fiber.plan.k[t] > 0.0) throw UnsupportedError("plasticity on a fibred element (element " + std::to_string(t) + "): its rest shape would flow under the fibre direction");
    ensurePlastic(s);
    plastic.plan = std::move(next);
    plastic.d_yield.upload(plastic.plan.yield, s);
    plastic.d_creep.upload(plastic.plan.creep, s);
    plastic.d_harden.upload(plastic.plan.harden, s);
    HIP_CHECK(hipStreamSynchronize(s));
}

void HipMesh::resetPlasticHistory(hipStream_t s)
{
    if (!plastic.allocated()) return;
    HIP_CHECK(hipMemcpyAsync(plastic.d_A0.p, d_A.p, 9 * (size_t)nT * sizeof(double), hipMemcpyDeviceToDevice, s));
    plastic.d_alpha.zero(s);
    plastic.d_count.zero(s);
    HIP_CHECK(hipStreamSynchronize(s));
}

void HipMesh::uploadFibers(hipStream_t s)
{
    if (!fiber.plan.nT) return;
    std::vector<double> A;
    const double* Ap = restTriInv.data();
    if (plastic.allocated()) { // (the host copy may be stale: HipPlastic)
        A.resize(9 * (size_t)nT);
        d_A.download(A.data(), A.size(), s);
        Ap = A.data();
    }
    buildFiberLists(fiber.plan, Ap, triArea.data());
    const FiberPlan& p = fiber.plan;
    fiber.d_fibTet.upload(p.fibTet, s);
    fiber.d_flags.upload(p.flagsF, s);
    fiber.d_groupOf.upload(p.groupOf, s);
    fiber.d_b.upload(p.b, s);
    fiber.d_volK.upload(p.volK, s);
    fiber.d_k2.upload(p.k2F, s);
    fiber.d_l0.upload(p.l0, s);
    if (!d_codimErr.n) { // the first codimensional term of this mesh
        d_codimErr.alloc(1);
        d_codimErr.zero(s);
    }
    HIP_CHECK(hipStreamSynchronize(s));
}

void HipMesh::setFibers(int tetBegin, int tetEnd, const double* dir, bool dirPerElement, double k, int law, double k2, bool tensionOnly, int group, hipStream_t s)
{
    FiberPlan next = fiber.plan; // a refused call changes nothing
    std::string err;
    if (!setFiberRange(next, nT, tetBegin, tetEnd, dir, dirPerElement, k, law, k2, tensionOnly, group, err)) throw ArgError(err);
    if (k > 0.0 && plastic.on()) // (fiber_kernels.h)
        for (int t = tetBegin; t < tetEnd; ++t)
            if (plastic.plan.yield[t] < INFINITY) throw UnsupportedError("fibres on a plastic element (element " + std::to_string(t) + "): its rest shape would flow under the fibre direction");
    fiber.plan = std::move(next);
    uploadFibers(s);
}

void HipMesh::setFiberActivation(int group, double act, hipStream_t s)
{
    std::string err;
    if (!ipcgpu::setFiberActivation(fiber.plan, group, act, err)) { // (the plan's function, fiber_plan.h)
        if (!fiber.plan.nT) throw StateError("ipcgpu_fiber_set_activation without fibres: call ipcgpu_set_fibers first");
        throw ArgError(err);
    }
    fiber.d_l0.upload(fiber.plan.l0, s);
    HIP_CHECK(hipStreamSynchronize(s));
}

void HipMesh::setChamberPressure(const double* pressure, hipStream_t s)
{
    if (!chamber.n()) throw StateError("ipcgpu_chamber_set_pressure without chambers: call ipcgpu_set_chambers first");
    if (!pressure) throw ArgError("chamber_set_pressure: null argument");
    for (int c = 0; c < chamber.n(); ++c)
        if (!std::isfinite(pressure[c])) throw ArgError("chamber_set_pressure: the pressure of chamber " + std::to_string(c) + " is not finite");
    std::string err;
    if (!chamberGasPressureOk(chamber.gas, chamber.n(), pressure, err)) throw ArgError("chamber_set_pressure: " + err);
    chamber.plan.pressure.assign(pressure, pressure + chamber.n());
    chamber.d_pressure.upload(chamber.plan.pressure, s);
    if (chamber.nGas()) uploadChamberGasPressures(s);
    HIP_CHECK(hipStreamSynchronize(s));
}

void HipMesh::uploadChamberGasPressures(hipStream_t s)
{
    // the gas chambers' entries of d_pEff hold p_c until the next gas update overwrites them with gauge(V_c): every assembly enqueues one first
    std::vector<double> pConst = chamber.plan.pressure;
    for (int c : chamber.gas.gasChamber) pConst[c] = 0.0;
    chamber.d_pConst.upload(pConst, s);
    chamber.d_pEff.upload(chamber.plan.pressure, s);
    HIP_CHECK(hipStreamSynchronize(s)); // (pConst leaves scope)
}

void HipMesh::setChamberGas(const int* isGas, const double* ambient, const double* gamma, const double* fillVolume, hipStream_t s)
{
    if (!chamber.n()) throw StateError("ipcgpu_chamber_set_gas without chambers: call ipcgpu_set_chambers first");
    ChamberGas gas;
    std::string err;
    if (!buildChamberGas(chamber.plan, isGas, ambient, gamma, fillVolume, gas, err)) throw ArgError(err);
    HIP_CHECK(hipStreamSynchronize(s)); // (nothing enqueued reads the arrays this call replaces)
    if (!gas.nGas) { // every chamber constant: the context is what it was before the gas law was ever set
        chamber.gas = ChamberGas();
        return;
    }
    chamber.gas = std::move(gas);
    const ChamberGas& g = chamber.gas;
    const size_t n = (size_t)chamber.n();
    chamber.d_sliceBegin.upload(g.sliceBegin, s);
    chamber.d_sliceEnd.upload(g.sliceEnd, s);
    chamber.d_sliceOff.upload(g.sliceOff, s);
    chamber.d_gasChamber.upload(g.gasChamber, s);
    chamber.d_isGas.upload(g.isGas, s);
    std::vector<double> param(3 * n), select((size_t)g.nGas * n, 0.0);
    for (size_t c = 0; c < n; ++c) {
        param[3 * c] = g.ambient[c];
        param[3 * c + 1] = g.gamma[c];
        param[3 * c + 2] = g.fillVolume[c];
    }
    for (int i = 0; i < g.nGas; ++i) select[(size_t)i * n + (size_t)g.gasChamber[i]] = 1.0;
    chamber.d_gasParam.upload(param, s);
    chamber.d_gasSelect.upload(select, s);
    chamber.d_slicePartial.alloc((size_t)g.nSlice());
    chamber.d_gasState.alloc(4 * n);
    chamber.d_gasState.zero(s);
    uploadChamberGasPressures(s);
}

void HipMesh::addSurfaceEdges(int nSF, const int* SF, int nCE, const int* CE)
{
    // Mesh.cpp:480-487: every surface triangle's edges enter vNeighbor too.  For a tet component they only repeat tet edges; for
    // a surface-only component (shell, scripted collision surface) they are the only adjacency its nodes have, and the barrier
    // blocks of a stencil whose nodes share such a triangle land on them once the nodes are free (penalty phase of a moving DBC).
    ++nbVersion;
    std::vector<std::pair<int, int>> edges;
    edges.reserve(nb.size() + 6 * (size_t)nSF);
    for (int v = 0; v < nV; ++v)
        for (int k = nbPtr[v]; k < nbPtr[v + 1]; ++k) edges.emplace_back(v, nb[k]);
    for (int t = 0; t < nSF; ++t)
        for (int a = 0; a < 3; ++a) {
            const int i = SF[t + (size_t)nSF * a], j = SF[t + (size_t)nSF * ((a + 1) % 3)];
            if (i < 0 || i >= nV || j < 0 || j >= nV) throw ArgError("set_surface: node id out of range");
            edges.emplace_back(i, j);
            edges.emplace_back(j, i);
        }
    for (int e = 0; e < nCE; ++e) { // codimensional segments (`.seg` shapes, Mesh.cpp:490-493)
        const int i = CE[2 * (size_t)e], j = CE[2 * (size_t)e + 1];
        if (i < 0 || i >= nV || j < 0 || j >= nV || i == j) throw ArgError("set_surface: bad codimensional segment");
        edges.emplace_back(i, j);
        edges.emplace_back(j, i);
    }
    std::sort(edges.begin(), edges.end());
    edges.erase(std::unique(edges.begin(), edges.end()), edges.end());
    if (edges.size() == nb.size()) return;
    nbPtr.assign(nV + 1, 0);
    for (auto& e : edges) nbPtr[e.first + 1]++;
    for (int v = 0; v < nV; ++v) nbPtr[v + 1] += nbPtr[v];
    nb.resize(edges.size());
    for (size_t i = 0; i < edges.size(); ++i) nb[i] = edges[i].second;
}

void HipMesh::uploadDBC(hipStream_t s)
{
    d_dbc.upload(dbcType, s);
    HIP_CHECK(hipStreamSynchronize(s));
}

void HipMesh::setComponentMaterial(int nodeBegin, int nodeEnd, int tetBegin, int tetEnd, double rho, double YM, double PR, hipStream_t s)
{
    // Mesh::setLameParam, componentMaterial branch (Mesh.cpp:665-671)
    for (int v = nodeBegin; v < nodeEnd; ++v) mass[v] *= rho / density;
    for (int t = tetBegin; t < tetEnd; ++t) {
        mu[t] = YM / 2.0 / (1.0 + PR);
        lam[t] = YM * PR / (1.0 + PR) / (1.0 - 2.0 * PR);
    }
    d_mass.upload(mass, s);
    d_mu.upload(mu, s);
    d_lam.upload(lam, s);
    HIP_CHECK(hipStreamSynchronize(s));
}

} // namespace ipcgpu
