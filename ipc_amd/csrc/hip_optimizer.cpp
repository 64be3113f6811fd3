// HipOptimizer: the Newton time stepper of Optimizer<3> with all state in HBM.
//   solve()            Optimizer.cpp:510-602        beginTimestep / newtonIter* / endTimestep
//   fullyImplicit_IP() Optimizer.cpp:1518-1819      (contact-free branch: one solveSub_IP per time step)
//   solveSub_IP()      Optimizer.cpp:1822-2213      newtonIter()
//   computeSearchDir() Optimizer.cpp:2324-2355
//   lineSearch()       Optimizer.cpp:2662-2916      (armijoParam = 0 at the IP call site :2059)
//   computeEnergyVal / computeGradient / computePrecondMtr   Optimizer.cpp:3199-3239, 3409-3450, 3549-3668
// Per Newton iteration only a handful of scalars cross PCIe (energies, step bound, |p|_inf, not-PD flag).
#include "hip_ipc.h"
#include <fstream>
#include <iomanip>
#include <limits>
#include <sstream>
#include <algorithm>
#include <cfloat>
#include <chrono>
#include <thread>
#include <iterator>
#include <cmath>
#include <cstring>
#include <type_traits>

#ifndef BEGIN_BATCHED
#define BEGIN_BATCHED 1 // 0: the time-step set-up of the contact-free twist question by question, as in rounds 1-5 (A/B: profiles/r06_begin_timestep_batch_ab.txt)
#endif

namespace ipcgpu {

// The reference's Optimizer constructor calls setTime(10.0, 0.025) (Optimizer.cpp:116) and derives eps_v^2 h^2 (fricDHat0 / fricDHatTarget, :290-303)
// and CN_MBC (:268) from THAT step size; main.cpp:1398 sets the scene's dt afterwards and setTime (:421-429) recomputes neither.  So in the reference
// these three carry h = 0.025 whatever `time` the scene file gives -- found on otherExamples/typical/sphere1K_DCORotCylinders.txt (dt 0.04, selfFric 0.5:
// 47 Newton iterations in the step after the first contact, 20 with eps_v scaled by the scene's own dt; same counts once this is followed).
// The value is an optimizer parameter since round 4 (HipOptimizer::ctorDt, ipcgpu_opt_set_constructor_dt): 0.025 = the reference's behaviour is the default,
// the scene's own dt gives the paper's eps_v h.

namespace {
struct Tic {
    double& acc;
    hipStream_t s;
    std::chrono::high_resolution_clock::time_point t0;
    bool nosync = false; // the caller has synchronised what it timed by an event: the stream may carry work enqueued AHEAD (speculativeAssembly) that must not be waited for
    Tic(double& a, hipStream_t st) : acc(a), s(st), t0(std::chrono::high_resolution_clock::now()) {}
    ~Tic()
    {
        if (!nosync) (void)hipStreamSynchronize(s);
        acc += std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
    }
};
} // namespace

HipOptimizer::HipOptimizer(HipMesh& m, HipLinSysSolver& l, hipStream_t s) : mesh(m), lin(l), stream(s) {}

ElemView HipOptimizer::view() const
{
    ElemView v;
    v.nV = mesh.nV;
    v.nT = mesh.nT;
    v.tetBegin = tetBegin;
    v.tetEnd = tetEnd;
    v.energyType = mesh.energyType;
    v.x = mesh.d_x.p;
    v.xTilde = mesh.d_xTilde.p;
    v.mass = mesh.d_mass.p;
    v.dbc = mesh.d_dbc.p;
    v.tet = mesh.d_tet.p;
    v.A = mesh.d_A.p;
    v.vol = mesh.d_vol.p;
    v.mu = mesh.d_mu.p;
    v.lam = mesh.d_lam.p;
    v.rowBase = lin.d_rowBase.p;
    v.rowLen = lin.d_rowLen.p;
    v.edgeP0 = lin.d_edgeP0.p;
    return v;
}

// the kernel argument of every view holds the term's own fields first and the shared ones behind them (codim_view.h): a reorder changes the kernels' code
#define CODIM_VIEW_LAYOUT(View, Fields, first)                                                                                              \
    static_assert(std::is_trivially_copyable<View>::value && sizeof(View) == sizeof(Fields) + sizeof(CodimBase) && __builtin_offsetof(View, first) == 0 \
            && __builtin_offsetof(View, x) == sizeof(Fields),                                                                                    \
        #View " is " #Fields " followed by CodimBase, nothing else")
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof" // (the views are not standard-layout: two bases with fields; the offsets are the ABI's all the same)
CODIM_VIEW_LAYOUT(ShellView, ShellFields, nTri);
CODIM_VIEW_LAYOUT(ShellLimitView, ShellLimitFields, nTri);
CODIM_VIEW_LAYOUT(ShellRubberView, ShellRubberFields, nTri);
CODIM_VIEW_LAYOUT(ShellWeaveView, ShellWeaveFields, nTri);
CODIM_VIEW_LAYOUT(RodView, RodFields, nSeg);
CODIM_VIEW_LAYOUT(AttachView, AttachFields, n);
CODIM_VIEW_LAYOUT(ChamberView, ChamberFields, nTri);
CODIM_VIEW_LAYOUT(AeroView, AeroFields, nTri);
CODIM_VIEW_LAYOUT(FiberView, FiberFields, nF);
#pragma clang diagnostic pop
#undef CODIM_VIEW_LAYOUT

CodimBase HipOptimizer::codimBase(const double* x_dev) const
{
    return CodimBase{ x_dev, mesh.d_dbc.p, lin.d_rowBase.p, lin.d_rowLen.p, lin.d_ja.p };
}

ShellView HipOptimizer::shellView(const double* x_dev) const
{
    const HipShell& sh = mesh.shell;
    ShellView v;
    static_cast<CodimBase&>(v) = codimBase(x_dev);
    v.nTri = sh.nTri();
    v.nHinge = sh.nHinge();
    v.tri = sh.d_tri.p;
    v.triConst = sh.d_triConst.p;
    v.hinge = sh.d_hinge.p;
    v.hingeConst = sh.d_hingeConst.p;
    return v;
}

ShellLimitView HipOptimizer::shellLimitView(const double* x_dev) const
{
    const HipShell& sh = mesh.shell;
    ShellLimitView v;
    static_cast<CodimBase&>(v) = codimBase(x_dev);
    v.nTri = sh.nTri();
    v.nLimited = sh.nLimited();
    v.tri = sh.d_tri.p;
    v.triConst = sh.d_triConst.p;
    v.limTri = sh.d_limTri.p;
    v.limConst = sh.d_limConst.p;
    v.triLimit = sh.nLimited() ? sh.d_triLimit.p : nullptr;
    return v;
}

ShellRubberView HipOptimizer::shellRubberView(const double* x_dev) const
{
    const HipShell& sh = mesh.shell;
    ShellRubberView v;
    static_cast<CodimBase&>(v) = codimBase(x_dev);
    v.nTri = sh.nTri();
    v.nRubber = sh.nRubber();
    v.tri = sh.d_tri.p;
    v.triConst = sh.d_triConst.p;
    v.rubTri = sh.d_rubTri.p;
    v.rubConst = sh.d_rubConst.p;
    return v;
}

ShellWeaveView HipOptimizer::shellWeaveView(const double* x_dev) const
{
    const HipShell& sh = mesh.shell;
    ShellWeaveView v;
    static_cast<CodimBase&>(v) = codimBase(x_dev);
    v.nTri = sh.nTri();
    v.nWoven = sh.nWoven();
    v.tri = sh.d_tri.p;
    v.triConst = sh.d_triConst.p;
    v.wovTri = sh.d_wovTri.p;
    v.wovConst = sh.d_wovConst.p;
    return v;
}

RodView HipOptimizer::rodView(const double* x_dev) const
{
    const HipRod& r = mesh.rod;
    RodView v;
    static_cast<CodimBase&>(v) = codimBase(x_dev);
    v.nSeg = r.nSeg();
    v.nBend = r.nBendActive();
    v.seg = r.d_seg.p;
    v.segConst = r.d_segConst.p;
    v.bend = r.d_bend.p;
    v.bendConst = r.d_bendConst.p;
    return v;
}

AttachView HipOptimizer::attachView(const double* x_dev) const
{
    const HipAttach& t = mesh.attach;
    AttachView v;
    static_cast<CodimBase&>(v) = codimBase(x_dev);
    v.n = t.n();
    v.node = t.d_node.p;
    v.coef = t.d_coef.p;
    v.kL = t.d_kL.p;
    return v;
}

FiberView HipOptimizer::fiberView(const double* x_dev) const
{
    const HipFiber& f = mesh.fiber;
    FiberView v;
    static_cast<CodimBase&>(v) = codimBase(x_dev);
    v.nF = f.n();
    v.fibTet = f.d_fibTet.p;
    v.tet = mesh.d_tet.p;
    v.b = f.d_b.p;
    v.volK = f.d_volK.p;
    v.k2 = f.d_k2.p;
    v.flags = f.d_flags.p;
    v.groupOf = f.d_groupOf.p;
    v.l0 = f.d_l0.p;
    return v;
}

ChamberView HipOptimizer::chamberView(const double* x_dev, int pressure) const
{
    const HipChamber& h = mesh.chamber;
    ChamberView v;
    static_cast<CodimBase&>(v) = codimBase(x_dev);
    v.nTri = h.nTri();
    v.n = h.n();
    v.tri = h.d_tri.p;
    v.chamberOf = h.d_chamberOf.p;
    v.triEnd = h.d_triEnd.p;
    v.pressure = !h.nGas() ? h.d_pressure.p : pressure == CHAMBER_P_CONSTANT ? h.d_pConst.p : h.d_pEff.p;
    v.ref = h.d_ref.p;
    return v;
}

void HipOptimizer::chamberVolumeGradient(int gasIndex, bool projectDBC, double* u_dev)
{
    const HipChamber& h = mesh.chamber;
    launch_chamber_volume_gradient(chamberView(mesh.d_x.p), h.d_gasSelect.p + (size_t)gasIndex * (size_t)h.n(), projectDBC ? 1 : 0, u_dev, 3 * (size_t)mesh.nV, stream);
}

void HipOptimizer::chamberGasCorrect(double coef, bool projectDBC, double* y_dev)
{
    const HipChamber& h = mesh.chamber;
    const int k = h.nGas();
    if (!k) return;
    const size_t n3 = 3 * (size_t)mesh.nV;
    d_gasU.alloc((size_t)k * n3);
    d_gasZ.alloc((size_t)k * n3);
    d_gasDots.alloc(chamber_gas_dot_doubles(n3, k));
    d_gasW.alloc(8);
    launch_chamber_gas_update(chamberView(mesh.d_x.p), h.gasView(), 0.0, nullptr, false, stream); // beta_c at the current positions
    for (int c = 0; c < k; ++c) {
        chamberVolumeGradient(c, projectDBC, d_gasU.p + (size_t)c * n3);
        lin.solve(d_gasU.p + (size_t)c * n3, d_gasZ.p + (size_t)c * n3);
    }
    launch_chamber_gas_woodbury(h.gasView(), coef, n3, d_gasU.p, d_gasZ.p, y_dev, d_gasDots.p, d_gasW.p, stream);
    HIP_CHECK(hipGetLastError());
}

void HipOptimizer::refreshChamberRef()
{
    if (!mesh.chamber.n()) return;
    launch_chamber_state(chamberView(mesh.d_x.p), nullptr, nullptr, mesh.chamber.d_ref.p, stream);
    HIP_CHECK(hipGetLastError());
}

AeroView HipOptimizer::aeroView(const double* x_dev) const
{
    const HipAero& h = mesh.aero;
    AeroView v;
    static_cast<CodimBase&>(v) = codimBase(x_dev);
    v.nTri = h.nTri();
    v.n = h.n();
    v.tri = h.d_tri.p;
    v.surfOf = h.d_surfOf.p;
    v.coef = h.d_coef.p;
    v.lagged = h.d_lagged.p;
    for (int a = 0; a < 3; ++a) v.wind[a] = h.wind[a];
    v.density = h.density;
    v.dt = dt;
    return v;
}

PlasticView HipOptimizer::plasticView(const double* x_dev, double dt_) const
{
    const HipPlastic& h = mesh.plastic;
    return PlasticView{ mesh.nT, tetBegin, tetEnd, x_dev, mesh.d_tet.p, mesh.d_A.p, mesh.d_vol.p, h.d_yield.p, h.d_creep.p, h.d_harden.p, h.d_alpha.p, dt_ };
}

void HipOptimizer::plasticFlow(const double* x_dev, double dt_)
{
    specAsmValid = false; // an assembly enqueued ahead read the rest shapes this flow rewrites
    mesh.plastic.d_count.zero(stream);
    launch_plastic_flow(plasticView(x_dev, dt_), mesh.plastic.d_count.p, stream);
}

ShellPlasticView HipOptimizer::shellPlasticView(const double* x_dev, double dt_) const
{
    const HipShell& sh = mesh.shell;
    const HipShellPlastic& h = sh.plastic;
    ShellPlasticView v;
    v.nTri = sh.nTri();
    v.nHinge = sh.nHinge();
    v.x = x_dev;
    v.tri = sh.d_tri.p;
    v.triConst = sh.d_triConst.p;
    v.hinge = sh.d_hinge.p;
    v.hingeConst = sh.d_hingeConst.p;
    v.yield = h.d_yield.p;
    v.creep = h.d_creep.p;
    v.harden = h.d_harden.p;
    v.alpha = h.d_alpha.p;
    v.hYield = h.d_hYield.p;
    v.hCreep = h.d_hCreep.p;
    v.hHarden = h.d_hHarden.p;
    v.hG = h.d_hG.p;
    v.alphaB = h.d_alphaB.p;
    v.hA = h.d_hA.p;
    v.B0 = h.d_B0.p;
    v.thetaBar0 = h.d_thetaBar0.p;
    v.dt = dt_;
    return v;
}

void HipOptimizer::shellPlasticFlow(const double* x_dev, double dt_)
{
    specAsmValid = false; // an assembly enqueued ahead read the rest records these flows rewrite
    HipShellPlastic& h = mesh.shell.plastic;
    h.d_count.zero(stream);
    launch_shell_plastic_flow(shellPlasticView(x_dev, dt_), h.plan.nOn > 0, h.plan.nHingeOn > 0, h.d_count.p, stream);
}

void HipOptimizer::refreshAeroLagged()
{
    if (!mesh.aero.n()) return;
    launch_aero_refresh(aeroView(mesh.d_x.p), mesh.aero.d_lagged.p, stream);
    HIP_CHECK(hipGetLastError());
}

// The codimensional terms, one row each, in launch order.  A new term is a kernel file, a view builder and a row here.
namespace {
struct CodimTerm {
    unsigned bit;
    int (*lanes)(const HipMesh&); // lanes of its energy kernel; 0: the mesh has no such term and nothing of it is launched
    void (*energy)(const HipOptimizer&, const double* x, double coef, double* partial, double* out, bool accumulate);
    void (*assemble)(const HipOptimizer&, const double* x, double coef, int projectDBC, double* grad, double* a, int* err);
};
const CodimTerm CODIM_TERMS[] = {
    { HipOptimizer::CODIM_SHELL, [](const HipMesh& m) { return m.shell.nTri() ? m.shell.nTri() + m.shell.nHinge() : 0; },
        [](const HipOptimizer& o, const double* x, double coef, double* partial, double* out, bool acc) { launch_shell_energy(o.shellView(x), coef, partial, out, acc, o.stream); },
        [](const HipOptimizer& o, const double* x, double coef, int proj, double* g, double* a, int* err) { launch_shell_assemble(o.shellView(x), coef, proj, g, a, err, o.stream); } },
    { HipOptimizer::CODIM_SHELL_RUBBER, [](const HipMesh& m) { return m.shell.nRubber(); },
        [](const HipOptimizer& o, const double* x, double coef, double* partial, double* out, bool acc) { launch_shell_rubber_energy(o.shellRubberView(x), coef, partial, out, acc, o.stream); },
        [](const HipOptimizer& o, const double* x, double coef, int proj, double* g, double* a, int* err) { launch_shell_rubber_assemble(o.shellRubberView(x), coef, proj, g, a, err, o.stream); } },
    { HipOptimizer::CODIM_SHELL_WEAVE, [](const HipMesh& m) { return m.shell.nWoven(); },
        [](const HipOptimizer& o, const double* x, double coef, double* partial, double* out, bool acc) { launch_shell_weave_energy(o.shellWeaveView(x), coef, partial, out, acc, o.stream); },
        [](const HipOptimizer& o, const double* x, double coef, int proj, double* g, double* a, int* err) { launch_shell_weave_assemble(o.shellWeaveView(x), coef, proj, g, a, err, o.stream); } },
    { HipOptimizer::CODIM_SHELL_LIMIT, [](const HipMesh& m) { return m.shell.nLimited(); },
        [](const HipOptimizer& o, const double* x, double coef, double* partial, double* out, bool acc) { launch_shell_limit_energy(o.shellLimitView(x), coef, partial, out, acc, o.stream); },
        [](const HipOptimizer& o, const double* x, double coef, int proj, double* g, double* a, int* err) { launch_shell_limit_assemble(o.shellLimitView(x), coef, proj, g, a, err, o.stream); } },
    { HipOptimizer::CODIM_ROD, [](const HipMesh& m) { return m.rod.nSeg() ? m.rod.nSeg() + m.rod.nBend() : 0; },
        [](const HipOptimizer& o, const double* x, double coef, double* partial, double* out, bool acc) { launch_rod_energy(o.rodView(x), coef, partial, out, acc, o.stream); },
        [](const HipOptimizer& o, const double* x, double coef, int proj, double* g, double* a, int* err) { launch_rod_assemble(o.rodView(x), coef, proj, g, a, err, o.stream); } },
    { HipOptimizer::CODIM_ATTACH, [](const HipMesh& m) { return m.attach.n(); },
        [](const HipOptimizer& o, const double* x, double coef, double* partial, double* out, bool acc) { launch_attach_energy(o.attachView(x), coef, partial, out, acc, o.stream); },
        [](const HipOptimizer& o, const double* x, double coef, int proj, double* g, double* a, int* err) { launch_attach_assemble(o.attachView(x), coef, proj, g, a, err, o.stream); } },
    { HipOptimizer::CODIM_CHAMBER, [](const HipMesh& m) { return m.chamber.nTri(); },
        // with a gas chamber: the per-triangle energy of the constant chambers (where there is one), then the gas update, which adds the gas chambers' W; and the
        // gas update ahead of the assembly, which reads the gauge pressures it leaves (chamber_kernels.h).  Without one: the two launches as they always were.
        [](const HipOptimizer& o, const double* x, double coef, double* partial, double* out, bool acc) {
            const HipChamber& h = o.mesh.chamber;
            if (!h.nGas() || h.nGas() < h.n()) {
                launch_chamber_energy(o.chamberView(x, HipOptimizer::CHAMBER_P_CONSTANT), coef, partial, out, acc, o.stream);
                acc = true;
            }
            if (h.nGas()) launch_chamber_gas_update(o.chamberView(x), h.gasView(), coef, out, acc, o.stream);
        },
        [](const HipOptimizer& o, const double* x, double coef, int proj, double* g, double* a, int* err) {
            const HipChamber& h = o.mesh.chamber;
            if (h.nGas()) launch_chamber_gas_update(o.chamberView(x), h.gasView(), 0.0, nullptr, false, o.stream);
            launch_chamber_assemble(o.chamberView(x), coef, proj, g, a, err, o.stream);
        } },
    { HipOptimizer::CODIM_AERO, [](const HipMesh& m) { return m.aero.nTri(); },
        [](const HipOptimizer& o, const double* x, double coef, double* partial, double* out, bool acc) { launch_aero_energy(o.aeroView(x), coef, partial, out, acc, o.stream); },
        [](const HipOptimizer& o, const double* x, double coef, int proj, double* g, double* a, int* err) { launch_aero_assemble(o.aeroView(x), coef, proj, g, a, err, o.stream); } },
    { HipOptimizer::CODIM_FIBER, [](const HipMesh& m) { return m.fiber.n(); },
        [](const HipOptimizer& o, const double* x, double coef, double* partial, double* out, bool acc) { launch_fiber_energy(o.fiberView(x), coef, partial, out, acc, o.stream); },
        [](const HipOptimizer& o, const double* x, double coef, int proj, double* g, double* a, int* err) { launch_fiber_assemble(o.fiberView(x), coef, proj, g, a, err, o.stream); } },
};
} // namespace

size_t HipOptimizer::codimPartials() const
{
    size_t n = 0;
    for (const CodimTerm& t : CODIM_TERMS) n = std::max(n, (size_t)t.lanes(mesh));
    return n;
}

void HipOptimizer::codimEnergyAdd(const double* x_dev, double coef, double* out_dev, bool accumulate, unsigned which)
{
    for (const CodimTerm& t : CODIM_TERMS) {
        if (!(which & t.bit) || !t.lanes(mesh)) continue;
        t.energy(*this, x_dev, coef, d_partial.p, out_dev, accumulate);
        accumulate = true;
    }
}

void HipOptimizer::codimAssembleAdd(double coef, bool projectDBC, double* grad_dev, double* a_dev, const double* x_dev, unsigned which)
{
    for (const CodimTerm& t : CODIM_TERMS)
        if ((which & t.bit) && t.lanes(mesh)) t.assemble(*this, x_dev ? x_dev : mesh.d_x.p, coef, projectDBC ? 1 : 0, grad_dev, a_dev, mesh.d_codimErr.p);
}

void HipOptimizer::enqueueElasticEnergy(bool ownerRank, double* out_dev)
{
    launch_energy(view(), elasticCoef(), true, ownerRank, d_partial.p, (int)d_partial.n, out_dev, stream);
    codimEnergyAdd(mesh.d_x.p, elasticCoef(), out_dev, /*accumulate=*/true);
}

void HipOptimizer::shellStretch(double* sigma_host, double* maxRatio, int* nOver, const double* x_dev)
{
    HipShell& sh = mesh.shell;
    if (maxRatio) *maxRatio = 0.0;
    if (nOver) *nOver = 0;
    if (!sh.nTri()) return;
    const ShellLimitView v = shellLimitView(x_dev ? x_dev : mesh.d_x.p);
    DevBuf<double> sigma;
    if (sigma_host) sigma.alloc(2 * (size_t)sh.nTri());
    sh.d_stretchPartial.ensure(2 * (size_t)shell_stretch_blocks(v));
    sh.d_stretchOut.alloc(2);
    launch_shell_stretch(v, sigma_host ? sigma.p : nullptr, sh.d_stretchPartial.p, sh.d_stretchOut.p, stream);
    HIP_CHECK(hipGetLastError());
    double out[2] = { 0.0, 0.0 };
    if (sigma_host) HIP_CHECK(hipMemcpyAsync(sigma_host, sigma.p, 2 * (size_t)sh.nTri() * sizeof(double), hipMemcpyDeviceToHost, stream));
    sh.d_stretchOut.download(out, 2, stream); // synchronises
    if (maxRatio) *maxRatio = out[0];
    if (nOver) *nOver = (int)out[1];
}

bool HipOptimizer::shellLimitFeasible()
{
    if (!mesh.shell.nLimited()) return true;
    int nOver = 0;
    shellStretch(nullptr, nullptr, &nOver);
    return nOver == 0;
}

void HipOptimizer::requireShellLimitFeasible()
{
    if (!mesh.shell.nLimited()) return;
    int nOver = 0;
    shellStretch(nullptr, nullptr, &nOver);
    mesh.shell.limitUnchecked = false;
    if (nOver)
        throw StateError(std::to_string(nOver) + " shell triangle" + (nOver == 1 ? " has" : "s have") + " a principal stretch at or over the strain limit at the start of the time step");
}

int HipOptimizer::shellRubberDegenerate()
{
    HipShell& sh = mesh.shell;
    if (!sh.nRubber()) return 0;
    const ShellRubberView v = shellRubberView(mesh.d_x.p);
    sh.d_rubCount.ensure((size_t)shell_rubber_energy_blocks(v) + 1); // the count, then the partial sums
    launch_shell_rubber_degenerate(v, sh.d_rubCount.p + 1, sh.d_rubCount.p, stream);
    HIP_CHECK(hipGetLastError());
    double n = 0.0;
    sh.d_rubCount.download(&n, 1, stream); // synchronises
    return (int)n;
}

void HipOptimizer::requireShellRubberFeasible()
{
    if (!mesh.shell.nRubber()) return;
    const int n = shellRubberDegenerate();
    mesh.shell.rubberUnchecked = false;
    if (n) throw StateError(std::to_string(n) + " rubber triangle" + (n == 1 ? " is" : "s are") + " degenerate (collapsed to a line: the energy is infinite) at the start of the time step");
}

void HipOptimizer::init(double dt_, bool withGravity)
{
    dt = dt_;
    dtSq = dt * dt;
    gravity[0] = gravity[2] = 0.0;
    gravity[1] = withGravity ? -9.80665 : 0.0; // Optimizer.cpp:112-115
    const size_t n3 = 3 * (size_t)mesh.nV;
    d_vel.alloc(n3);
    d_vel.zero(stream);
    d_acc.alloc(n3); // Optimizer.cpp:176-177
    d_acc.zero(stream);
    d_dxElastic.alloc(n3);
    d_dxElastic.zero(stream);
    d_xPrev.alloc(n3);
    d_xStepStart.alloc(n3);
    d_searchDir.alloc(n3);
    d_searchDir.zero(stream);
    d_gradient.alloc(n3);
    d_gradient.zero(stream);
    d_minusG.alloc(n3);
    d_x0.alloc(n3);
    d_partial.alloc(std::max((size_t)std::max(mesh.nT, mesh.nV), codimPartials()) / 256 + 2);
    d_scalar.alloc(S_COUNT);
    d_flag.alloc(2); // [0] the inversion flag of the stepper, [1] a second one for batches that test two states (beginTimestep)
    h_scalar.alloc(S_COUNT);
    h_flag.alloc(2);
    HIP_CHECK(hipMemcpyAsync(d_xPrev.p, mesh.d_x.p, n3 * sizeof(double), hipMemcpyDeviceToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(d_xStepStart.p, mesh.d_x.p, n3 * sizeof(double), hipMemcpyDeviceToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(mesh.d_xTilde.p, mesh.d_x.p, n3 * sizeof(double), hipMemcpyDeviceToDevice, stream));
    for (int c = 0; c < 3; ++c) rotCenter[c] = 0.5 * (mesh.bboxLo[c] + mesh.bboxHi[c]);
    // element shard of this rank (contiguous blocks of the caller's tet order)
    tetBegin = (int)((long long)mesh.nT * rank / worldSize);
    tetEnd = (int)((long long)mesh.nT * (rank + 1) / worldSize);
    setRelGL2Tol(1.0e-2); // main.cpp:159 -> Optimizer.hpp:148 default
    innerIterAmt = globalIterNum = k = 0;
    std::memset(timers, 0, sizeof(timers));
    initialised = true;
    HIP_CHECK(hipStreamSynchronize(stream));
    computeXTilta(); // Optimizer.cpp:247-248: the first time step already sees gravity
}

void HipOptimizer::setRelGL2Tol(double relTol)
{
    relGL2Tol = relTol * relTol;
    targetGRes = std::sqrt(relGL2Tol * (absParameters ? 1.0 : mesh.bboxDiag2 * dtSq)); // Optimizer.cpp:2941-2945
    CN_MBC = std::sqrt(1.0e-4 * mesh.bboxDiag2 * (ctorDt * ctorDt)); // Optimizer.cpp:268 -- evaluated in the constructor, see (ctorDt * ctorDt)
}

void HipOptimizer::setParameterScaling(bool absolute, double dTolRel_, double kappaMinMultiplier_)
{
    // `useAbsParameters`, tuning[3], `kappaMinMultiplier` of the scene file (Config.cpp:553-558, Optimizer.cpp:102-109, 279-302, 1535-1537,
    // 2228-2233, 2941-2945): dHat, its target, dTol, eps_v and the Newton tolerance are absolute lengths instead of fractions of the
    // bounding-box diagonal; the distances of suggestKappa and CN_MBC stay relative there too
    if (!(dTolRel_ > 0.0) || !(kappaMinMultiplier_ > 0.0)) throw ArgError("set_parameter_scaling: dTolRel and kappaMinMultiplier must be positive");
    absParameters = absolute;
    dTolRel = dTolRel_;
    kappaMinMultiplier = kappaMinMultiplier_;
    targetGRes = std::sqrt(relGL2Tol * (absParameters ? 1.0 : mesh.bboxDiag2 * dtSq));
    if (ipOn()) {
        dHat = dHatEps * dHatEps * lenScale2();
        dTol = dTolRel * dTolRel * lenScale2();
    }
}

void HipOptimizer::setTwist(int nL, const int* left, int nR, const int* right, double angVel)
{
    // AnimScripter.cpp:555-572: handle set bI rotates with (-1)^bI * -0.4 pi about x through the rest bbox centre
    std::vector<int> ids;
    std::vector<double> ang;
    for (int i = 0; i < nL; ++i) {
        mesh.dbcType[left[i]] = 2;
        ids.push_back(left[i]);
        ang.push_back(-angVel * dt);
    }
    for (int i = 0; i < nR; ++i) {
        mesh.dbcType[right[i]] = 2;
        ids.push_back(right[i]);
        ang.push_back(angVel * dt);
    }
    nHandles = (int)ids.size();
    if (nHandles) {
        d_handleIds.upload(ids, stream);
        d_handleAng.upload(ang, stream);
    }
    mesh.uploadDBC(stream);
    if (initialised) computeXTilta(); // the handles are Dirichlet nodes now: xTilta = V_prev there (Optimizer.cpp:1244-1246)
}

void HipOptimizer::addNeumannBC(int n, const int* ids, const double* accel3, double t0, double t1)
{
    std::unique_ptr<NbcGroup> g(new NbcGroup);
    g->n = n;
    g->d_ids.upload(ids, (size_t)n, stream);
    for (int c = 0; c < 3; ++c) g->a[c] = accel3[c];
    g->t0 = t0;
    g->t1 = t1;
    HIP_CHECK(hipStreamSynchronize(stream));
    nbcGroups.push_back(std::move(g));
}

void HipOptimizer::neumannGradientAdd(double* grad_dev)
{
    for (const auto& g : nbcGroups) {
        if (stepStartTime < g->t0 || stepStartTime >= g->t1) continue;
        const double c[3] = { dtSq * g->a[0], dtSq * g->a[1], dtSq * g->a[2] };
        launch_nbc_gradient(g->n, g->d_ids.p, mesh.d_dbc.p, mesh.d_mass.p, c, grad_dev, stream);
    }
}

double HipOptimizer::neumannEnergy()
{
    double E = 0.0;
    for (const auto& g : nbcGroups) {
        if (stepStartTime < g->t0 || stepStartTime >= g->t1) continue;
        const double c[3] = { dtSq * g->a[0], dtSq * g->a[1], dtSq * g->a[2] };
        launch_nbc_energy(g->n, g->d_ids.p, mesh.d_dbc.p, mesh.d_mass.p, mesh.d_x.p, c, slot(S_SCRATCH), stream);
        E -= readScalar(S_SCRATCH);
    }
    return E;
}

void HipOptimizer::addDirichletBC(int n, const int* ids, const double* lin3, const double* angRad3, double t0, double t1)
{
    std::unique_ptr<DbcGroup> g(new DbcGroup);
    g->ids.assign(ids, ids + n);
    for (int c = 0; c < 3; ++c) {
        g->lin[c] = lin3[c];
        g->ang[c] = angRad3[c];
    }
    g->t0 = t0;
    g->t1 = t1;
    g->d_ids.upload(g->ids, stream);
    g->d_pos.alloc(3 * (size_t)n);
    if (baseDbcType.empty()) baseDbcType = mesh.dbcType;
    dbcGroups.push_back(std::move(g));
    setDBCVertices(); // initAnimScript (AnimScripter.cpp:122-124)
    if (initialised) computeXTilta();
}

void HipOptimizer::setDBCVertices()
{
    if (dbcGroups.empty()) return;
    if (baseDbcType.empty()) baseDbcType = mesh.dbcType;
    std::vector<int> t = baseDbcType;
    for (const auto& g : dbcGroups) {
        if (stepStartTime < g->t0 || stepStartTime >= g->t1) continue;
        const int type = g->isZero() ? 1 : 2;
        for (int v : g->ids) t[v] = std::max(t[v], type); // NONZERO overrides ZERO
    }
    if (t != mesh.dbcType) {
        mesh.dbcType = t;
        mesh.uploadDBC(stream);
    }
}

bool HipOptimizer::dbcGroupMotion()
{
    bool any = false;
    std::vector<double> pos;
    for (const auto& g : dbcGroups) {
        if (stepStartTime < g->t0 || stepStartTime >= g->t1 || g->ids.empty() || g->hasTargets) continue;
        const int n = (int)g->ids.size();
        // centre of the group's current bounding box (AnimScripter.cpp:1450-1455): a few KB to the host, once per time step
        launch_gather3(n, g->d_ids.p, mesh.d_x.p, g->d_pos.p, stream);
        pos.resize(3 * (size_t)n);
        g->d_pos.download(pos.data(), pos.size(), stream);
        HIP_CHECK(hipStreamSynchronize(stream));
        DbcMotion m;
        double lo[3] = { pos[0], pos[1], pos[2] }, hi[3] = { pos[0], pos[1], pos[2] };
        for (int i = 0; i < n; ++i)
            for (int c = 0; c < 3; ++c) {
                lo[c] = std::min(lo[c], pos[3 * (size_t)i + c]);
                hi[c] = std::max(hi[c], pos[3 * (size_t)i + c]);
            }
        for (int c = 0; c < 3; ++c) {
            m.c[c] = g->hasCenter ? g->center[c] : (lo[c] + hi[c]) / 2;
            m.linDt[c] = g->lin[c] * dt;
        }
        const double ax = g->ang[0] * dt, ay = g->ang[1] * dt, az = g->ang[2] * dt;
        const double cx = std::cos(ax), sx = std::sin(ax), cy = std::cos(ay), sy = std::sin(ay), cz = std::cos(az), sz = std::sin(az);
        const double Rx[9] = { 1, 0, 0, 0, cx, -sx, 0, sx, cx }, Ry[9] = { cy, 0, sy, 0, 1, 0, -sy, 0, cy }, Rz[9] = { cz, -sz, 0, sz, cz, 0, 0, 0, 1 };
        double T[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) T[3 * i + j] = Rx[3 * i] * Ry[j] + Rx[3 * i + 1] * Ry[3 + j] + Rx[3 * i + 2] * Ry[6 + j];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) m.R[3 * i + j] = T[3 * i] * Rz[j] + T[3 * i + 1] * Rz[3 + j] + T[3 * i + 2] * Rz[6 + j];
        launch_dbc_motion(n, g->d_ids.p, m, mesh.d_x.p, d_searchDir.p, stream);
        any = true;
    }
    for (const auto& g : dbcGroups) { // behind the velocities, as in AnimScripter.cpp:1465: the sequence SETS the move of its nodes
        if (!g->hasTargets || stepStartTime < g->t0 || stepStartTime >= g->t1 || g->ids.empty()) continue;
        launch_dbc_targets((int)g->ids.size(), g->d_ids.p, g->d_targets.p, mesh.d_x.p, d_searchDir.p, stream);
        any = true;
    }
    return any;
}

void HipOptimizer::reduceSum(double* dev, long long n)
{
    if (worldSize > 1) hookReduce(dev, n, 0);
}
void HipOptimizer::reduceMin(double* dev, long long n)
{
    if (worldSize > 1) hookReduce(dev, n, 1);
}
void HipOptimizer::hookReduce(double* dev, long long n, int op)
{
    commBytes += 8 * n;
    commCalls++;
    if (allreduceStream) { // RCCL from C, ordered on our stream
        if (allreduceStream(allreduceStreamUser, dev, n, op, (void*)stream) != 0) throw HipError("all-reduce hook failed");
        return;
    }
    if (!allreduce) throw StateError("sharded context without an all-reduce hook");
    HIP_CHECK(hipStreamSynchronize(stream));
    if (allreduce(allreduceUser, dev, n, op) != 0) throw HipError("all-reduce hook failed");
}
void HipOptimizer::publish(ScalarSlot first, int count)
{
    launch_publish(slot(first), slotMapped(first), count, stream);
}
double HipOptimizer::readScalar(ScalarSlot s)
{
    publish(s);
    HIP_CHECK(hipStreamSynchronize(stream));
    return published(s);
}

double HipOptimizer::computeEnergyVal()
{
    enqueueElasticEnergy(rank == 0, slot(S_E_ITERATE));
    reduceSum(slot(S_E_ITERATE), 1);
    // the barrier energy of the self-contact sets is enqueued behind the elastic one and read back with it: one synchronisation instead of two (round 6; the
    // reduction of the elastic partial sums is on the stream before the contact kernel reuses d_partial)
    const bool contactQueued = selfCollision && contact->energyEnqueue(mesh.d_x.p, dHat, kappa, d_partial, slot(S_CONTACT_E), slot(S_E_ITERATE), slotMapped(S_E_ITERATE), slotSpan(S_E_ITERATE, S_CONTACT_E));
    if (!(contactQueued && contact->publishedByEnergy())) publish(S_E_ITERATE, slotSpan(S_E_ITERATE, S_CONTACT_E));
    HIP_CHECK(hipStreamSynchronize(stream));
    double E = published(S_E_ITERATE);
    const double Econtact = contactQueued ? published(S_CONTACT_E) : 0.0;
    if (!nbcGroups.empty()) E += neumannEnergy();
    // barrier terms over the current constraint sets (Optimizer.cpp:3252-3353); replicated on every rank
    for (auto* h : colliders) E += h->energy(mesh.d_x.p, dHat, kappa);
    if (selfCollision) E += Econtact;
    if (fricDHat > 0.0) { // lagged friction (Optimizer.cpp:3357-3377)
        for (auto* h : colliders)
            if (h->friction > 0.0) E += h->frictionEnergy(mesh.d_x.p, d_xPrev.p, fricDHat);
        if (selfCollision && selfFric > 0.0) E += contact->frictionEnergy(mesh.d_x.p, d_xPrev.p, fricDHat, selfFric, d_partial, slot(S_FRICTION_E));
    }
    if (dampingStiff > 0.0) E += dampingEnergy();
    if (rhoDBC && !tpIds.empty()) { // augmentMDBCEnergy (Optimizer.cpp:3402-3404)
        launch_mdbc_reduce(mdbc(), mesh.d_x.p, rhoDBC, 0, slot(S_SCRATCH), stream);
        E += readScalar(S_SCRATCH);
    }
    return E;
}

// ---- lagged damping ----------------------------------------------------------------------------------------------
void HipOptimizer::setDamping(double stiff)
{
    dampingStiff = stiff > 0.0 ? stiff : 0.0; // Config.cpp:141-147
}
void HipOptimizer::computeDampingMtr()
{
    // computeDampingMtr (Optimizer.cpp:3723-3735) at the end of a time step (:593-595) and inside the first computePrecondMtr (:470,
    // 3598-3612).  The positions are kept: when the pattern grows the values are rebuilt from them on the new pattern.
    if (!(dampingStiff > 0.0)) return;
    d_xDamp.ensure(3 * (size_t)mesh.nV);
    HIP_CHECK(hipMemcpyAsync(d_xDamp.p, mesh.d_x.p, sizeof(double) * 3 * (size_t)mesh.nV, hipMemcpyDeviceToDevice, stream));
    assembleDampingMtr();
}
void HipOptimizer::assembleDampingMtr()
{
    const size_t nnz = lin.ja.size();
    d_damp.ensure(nnz);
    if (d_zeroMass.n < (size_t)mesh.nV) {
        d_zeroMass.alloc(mesh.nV);
        d_zeroMass.zero(stream);
    }
    ensurePatchPlan();
    int pb, pe;
    patchShard(pb, pe);
    ElemView v = view();
    v.x = d_xDamp.p;
    v.xTilde = d_xDamp.p;
    v.mass = d_zeroMass.p; // the patch pass owns the diagonal: no mass here, and the identity of the projected rows is cleared below
    if (worldSize > 1) HIP_CHECK(hipMemsetAsync(d_damp.p, 0, sizeof(double) * nnz, stream));
    if (shellOnly()) HIP_CHECK(hipMemsetAsync(d_damp.p, 0, sizeof(double) * nnz, stream)); // (no patch plan without tetrahedra: nothing else writes the values)
    launch_assemble_patches(v, patch, pb, pe, dampingStiff / dt, 1, nullptr, d_damp.p, stream);
    codimAssembleAdd(dampingStiff / dt, true, nullptr, d_damp.p, d_xDamp.p, CODIM_STIFFNESS); // the shell, rubber, weave, limit, rod, attachment and fibre Hessians at the damping positions (a chamber's pressure is no stiffness, nor is air drag)
    if (worldSize > 1) reduceSum(d_damp.p, (long long)nnz);
    launch_damp_clear_diag(mesh.nV, mesh.d_dbc.p, lin.d_ia.p, d_damp.p, stream);
    dampPatternVersion = lin.patternVersion;
}
double HipOptimizer::dampingEnergy()
{
    // Optimizer.cpp:3381-3400: 1/2 dx^T D dx with the displacement of the step, zero on every Dirichlet node
    if (dampPatternVersion != lin.patternVersion) assembleDampingMtr();
    const int n3 = 3 * mesh.nV;
    d_dampDx.ensure(n3);
    d_dampAdx.ensure(n3);
    launch_damp_dx(mesh.nV, mesh.d_dbc.p, 0, 1, mesh.d_x.p, d_xPrev.p, d_dampDx.p, stream);
    launch_csr_symv(n3, lin.d_ia.p, lin.d_ja.p, d_damp.p, d_dampDx.p, d_dampAdx.p, stream);
    launch_dot_scaled(n3, d_dampDx.p, d_dampAdx.p, 0.5, slot(S_DAMPING_E), stream);
    return readScalar(S_DAMPING_E);
}
void HipOptimizer::dampingGradientAdd(bool projectDBC, double* grad_dev)
{
    // Optimizer.cpp:3519-3540: gradient += D dx, the displacement cleared on the projected Dirichlet nodes
    if (dampPatternVersion != lin.patternVersion) assembleDampingMtr();
    const int n3 = 3 * mesh.nV;
    d_dampDx.ensure(n3);
    d_dampAdx.ensure(n3);
    launch_damp_dx(mesh.nV, mesh.d_dbc.p, 1, projectDBC ? 1 : 0, mesh.d_x.p, d_xPrev.p, d_dampDx.p, stream);
    launch_csr_symv(n3, lin.d_ia.p, lin.d_ja.p, d_damp.p, d_dampDx.p, d_dampAdx.p, stream);
    launch_axpy(n3, 1.0, d_dampAdx.p, grad_dev, stream);
}

// ---- lagged friction ---------------------------------------------------------------------------------------------
bool HipOptimizer::solveFric() const
{
    if (fricLoopForced) return true;
    if (selfCollision && selfFric > 0.0) return true;
    for (const auto* h : colliders)
        if (h->friction > 0.0) return true;
    return false;
}

void HipOptimizer::updateFrictionLag()
{
    // multipliers, closest points and tangent bases of the current constraint sets (Optimizer.cpp:1553-1600 / 1620-1675)
    if (!solveFric()) return;
    for (auto* h : colliders)
        if (h->friction > 0.0) h->lagUpdate(mesh.d_x.p, dHat, kappa);
    if (selfCollision && selfFric > 0.0) contact->frictionLagUpdate(mesh.d_x.p, dHat, kappa);
}

bool HipOptimizer::nextSubproblem()
{
    // tail of the fullyImplicit_IP loop body (Optimizer.cpp:1617-1790 with USE_DISCRETE_CMS, HOMOTOPY_VAR 1)
    specAsmValid = false; // friction lag / dHat / kappa change under an assembly enqueued ahead
    if (!ipOn()) return false;
    const double dHatTarget = dHatTargetEps > 0.0 ? dHatTargetEps * dHatTargetEps * lenScale2() : dHat;
    const bool fric = solveFric(), homotopy = dHat > dHatTarget;
    if (!fric && !homotopy) return false; // every active distance is below dHat = dHatTarget: nothing left to update (:1706-1709, 1754-1757)
    fricIterI++;
    if (fric) updateFrictionLag();
    if (!nConstraints()) return false; // "no collision in this time step"
    bool updateDHat = true;
    { // discrete complementarity slackness on the distances of the active sets (:1706-1713); once per sub-problem, on the host
        double dMax = 0.0, dMin = 1.0e300;
        std::vector<double> d;
        for (auto* h : colliders) {
            h->evalDist2(h->set, mesh.d_x.p, d);
            for (size_t i = 0; i < h->set.size(); ++i) {
                dMax = std::max(dMax, d[i]);
                dMin = std::min(dMin, d[i]);
            }
        }
        if (selfCollision) {
            std::vector<std::array<int, 4>> ids;
            contact->closeStencils(mesh.d_x.p, 1.0e300, ids, d);
            for (size_t i = 0; i < ids.size(); ++i) {
                dMax = std::max(dMax, d[i]);
                dMin = std::min(dMin, d[i]);
            }
        }
        if (dMax < dHatTarget) updateDHat = false;
        else if (dMin < dTol) return false; // "tiny distance fail-safe"
    }
    bool updateFricDHat = fric;
    if (fric && fricDHat <= fricDHatTarget) { // :1717 (the target equals the start value unless `tuning` gives a sixth entry)
        // tangent-space convergence test: one Newton direction with the refreshed lag (:1717-1731)
        computePrecondMtr(true, true);
        computeSearchDir();
        enqueueDirNorm();
        if (readScalar(S_DIR_NORM) < targetGRes) updateFricDHat = false;
        if (fricIterAmt > 0 && fricIterI >= fricIterAmt) updateFricDHat = false;
    }
    if (!updateDHat && !updateFricDHat) return false;
    if (updateDHat) { // :1763-1774
        dHat = std::max(0.5 * dHat, dHatTarget);
        computeConstraintSets();
        initKappa();
    }
    if (updateFricDHat && fricDHat > 0.0) fricDHat = std::max(0.5 * fricDHat, fricDHatTarget); // :1776-1781
    initSubProblem(); // the next solveSub_IP starts with m_projectDBC = true, rho_DBC = 0 (Optimizer.cpp:1826-1828)
    closeID.clear(); // initSubProb_IP
    closeVal.clear();
    closeHS.clear();
    closeHSVal.clear();
    k = 0;
    return true;
}

size_t HipOptimizer::nConstraints() const
{
    size_t n = selfCollision ? (size_t)contact->nActive() : 0;
    for (const auto* h : colliders) n += h->set.size();
    return n;
}

int HipOptimizer::addHalfSpace(HipContact* c, const double* origin3, const double* normal3, double eps)
{
    // `ground` / `halfSpace` script keywords (Config.cpp:306-345) -> animConfig.collisionObjects; friction is a SURVEY 8f row
    if (!c || !c->surfaceSet) throw StateError("opt_add_half_space before set_surface");
    // one dHat for the whole interior-point problem, as in the reference (a single `dHat` script keyword, Config.cpp:41-45):
    // a second object registered with another value would silently change the first one's activation distance
    if (ipOn() && eps != dHatEps) throw ArgError("all collision objects of a context share one dHat (Config.cpp:41-45): got a different dHatEps");
    contact = c;
    planes.push_back(HipHalfSpace::create(stream, origin3, normal3));
    listColliders();
    dHatEps = eps;
    dHat = eps * eps * lenScale2();
    dTol = dTolRel * dTolRel * lenScale2();
    return (int)planes.size() - 1;
}

int HipOptimizer::addRoundCollider(HipContact* c, const double* p0, const double* p1, double R, int hollow, double eps)
{
    // sphere / capsule obstacle (round_collider_kernels.h): registered like a half-space, one dHat for the whole context
    if (!c || !c->surfaceSet) throw StateError("opt_add_round_collider before set_surface");
    if (worldSize > 1) throw UnsupportedError("round colliders on a sharded context");
    if (ipOn() && eps != dHatEps) throw ArgError("all collision objects of a context share one dHat (Config.cpp:41-45): got a different dHatEps");
    RoundShape shape;
    std::string err;
    if (!planRoundCollider(p0, p1, R, hollow, eps * eps * lenScale2(), shape, err)) throw ArgError(err);
    std::unique_ptr<HipRoundCollider> h = HipRoundCollider::create(stream, shape);
    if (h->intersected(mesh.nV, mesh.d_x.p, mesh.d_dbc.p)) throw StateError("round collider: a node lies on or inside the collider at the current positions (an intersecting start state)");
    contact = c;
    rounds.push_back(std::move(h));
    listColliders();
    dHatEps = eps;
    dHat = eps * eps * lenScale2();
    dTol = dTolRel * dTolRel * lenScale2();
    return (int)rounds.size() - 1;
}

void HipOptimizer::listColliders()
{
    colliders.clear();
    for (const auto& h : planes) colliders.push_back(h.get());
    for (const auto& h : rounds) colliders.push_back(h.get());
}

void HipOptimizer::requireRoundsFeasible()
{
    std::string err;
    for (auto& h : rounds) {
        if (!checkRoundColliderDHat(h->shape, dHatEps * dHatEps * lenScale2(), err)) throw ArgError(err);
        if (h->intersected(mesh.nV, mesh.d_x.p, mesh.d_dbc.p)) throw StateError("round collider: a node lies on or inside the collider at the current positions (an intersecting start state)");
    }
}

bool HipOptimizer::anyIntersection()
{
    // isIntersected (Optimizer.cpp:2626-2659): analytic objects first, then the mesh against itself
    for (auto* h : colliders)
        if (h->intersected(mesh.nV, mesh.d_x.p, mesh.d_dbc.p)) return true;
    return selfCollision && isIntersected();
}

// ---- self-contact ----------------------------------------------------------------------------------------------
void HipOptimizer::enableSelfCollision(HipContact* c, double eps)
{
    // `selfCollisionOn` + interior point; dHat = dHatEps^2 * bbox diagonal^2 (Optimizer.cpp:1534-1537, Config.cpp:41-45)
    if (!c || !c->surfaceSet) throw StateError("opt_enable_self_collision before set_surface");
    if (!colliders.empty() && eps != dHatEps) throw ArgError("all collision objects of a context share one dHat (Config.cpp:41-45): got a different dHatEps");
    contact = c;
    selfCollision = true;
    dHatEps = eps;
    dHat = eps * eps * lenScale2();
    dTol = dTolRel * dTolRel * lenScale2(); // dTolRel = tuning[3], 1e-9 by default (Optimizer.cpp:102-109)
}

void HipOptimizer::computeXTilta()
{
    // Optimizer.cpp:1236-1257 on the host: only used when the caller overrides the velocity
    const size_t n3 = 3 * (size_t)mesh.nV;
    std::vector<double> xp(n3), vel(n3), xt(n3), acc(n3, 0.0);
    d_xPrev.download(xp.data(), n3, stream);
    d_vel.download(vel.data(), n3, stream);
    d_acc.download(acc.data(), n3, stream);
    for (int v = 0; v < mesh.nV; ++v)
        for (int c = 0; c < 3; ++c) {
            const size_t i = 3 * (size_t)v + c;
            if (mesh.isDBCVertex(v)) xt[i] = xp[i];
            else if (timeIntegration == 1) xt[i] = xp[i] + (vel[i] * dt + betaNM * (dtSq * gravity[c]) + (0.5 - betaNM) * (dtSq * acc[i])); // :1259-1277
            else xt[i] = xp[i] + (vel[i] * dt + dtSq * gravity[c]);
        }
    mesh.d_xTilde.upload(xt, stream);
    HIP_CHECK(hipStreamSynchronize(stream));
}

void HipOptimizer::setTimeIntegration(int type, double beta, double gamma)
{
    timeIntegration = type;
    betaNM = beta;
    gammaNM = gamma;
    computeXTilta();
}

void HipOptimizer::getDbcState(double* out4) const
{
    out4[0] = completedStep;
    out4[1] = rhoDBC;
    out4[2] = projDBC ? 1.0 : 0.0;
    out4[3] = (double)tpIds.size();
}

void HipOptimizer::getKinematics(double* vel, double* acc, double* dxElastic)
{
    const size_t n3 = 3 * (size_t)mesh.nV;
    if (vel) d_vel.download(vel, n3, stream);
    if (acc) d_acc.download(acc, n3, stream);
    if (dxElastic) d_dxElastic.download(dxElastic, n3, stream);
    HIP_CHECK(hipStreamSynchronize(stream));
}

// Optimizer::saveStatus (Optimizer.cpp:2964-3011): the reference's text checkpoint, readable by either implementation
void HipOptimizer::saveStatus(const std::string& path)
{
    const size_t n3 = 3 * (size_t)mesh.nV;
    std::vector<double> x(n3), vel(n3), acc(n3), dx(n3);
    mesh.d_x.download(x.data(), n3, stream);
    getKinematics(vel.data(), acc.data(), dx.data());
    std::ofstream out(path, std::ios::out);
    if (!out.is_open()) throw StateError("unable to create status file " + path);
    out << std::setprecision(std::numeric_limits<long double>::digits10 + 2);
    out << "timestep " << globalIterNum << "\n\n";
    auto rows = [&](const char* name, const std::vector<double>& a) {
        out << name << " " << mesh.nV << " 3\n";
        for (int v = 0; v < mesh.nV; ++v) out << a[3 * (size_t)v] << " " << a[3 * (size_t)v + 1] << " " << a[3 * (size_t)v + 2] << "\n";
    };
    rows("position", x);
    out << "\n";
    out << "velocity " << n3 << "\n";
    for (size_t i = 0; i < n3; ++i) out << vel[i] << "\n";
    out << "\n";
    rows("acceleration", acc);
    out << "\n";
    rows("dx_Elastic", dx);
    if (mesh.plastic.on()) { // a project extension (the reference's reader skips the tokens): restTriInv (nine entries, column-major) and alpha per element
        const size_t nT = (size_t)mesh.nT;
        std::vector<double> A(9 * nT), alpha(nT);
        mesh.d_A.download(A.data(), A.size(), stream);
        mesh.plastic.d_alpha.download(alpha.data(), nT, stream);
        out << "\nplastic " << mesh.nT << " 10\n";
        for (size_t t = 0; t < nT; ++t) {
            for (int k = 0; k < 9; ++k) out << A[k * nT + t] << " ";
            out << alpha[t] << "\n";
        }
    }
    if (mesh.fiber.n()) { // a project extension, beside `plastic`: the activations per group, then k, k2, the flag word, the group and the unit direction per element
        const FiberPlan& p = mesh.fiber.plan;
        const size_t nT = (size_t)mesh.nT;
        out << "\nfiber " << mesh.nT << " 7 " << FIBER_MAX_GROUPS << "\n";
        for (int g = 0; g < FIBER_MAX_GROUPS; ++g) out << p.act[g] << (g + 1 < FIBER_MAX_GROUPS ? " " : "\n");
        for (size_t t = 0; t < nT; ++t)
            out << p.k[t] << " " << p.k2[t] << " " << p.flags[t] << " " << p.group[t] << " " << p.dir[t] << " " << p.dir[nT + t] << " " << p.dir[2 * nT + t] << "\n";
    }
    if (mesh.shell.plastic.on()) { // a project extension, beside `plastic`: B (b00 b10 b01 b11) and alpha per shell triangle, then thetaBar and alphaB per hinge
        const HipShell& sh = mesh.shell;
        const size_t nTri = (size_t)sh.nTri(), nH = (size_t)sh.nHinge();
        std::vector<double> B(4 * nTri), alpha(nTri), thetaBar(nH), alphaB(nH);
        sh.d_triConst.download(B.data(), B.size(), stream);
        sh.plastic.d_alpha.download(alpha.data(), nTri, stream);
        sh.d_hingeConst.download(thetaBar.data(), nH, stream);
        sh.plastic.d_alphaB.download(alphaB.data(), nH, stream);
        out << "\nshellplastic " << sh.nTri() << " 5 " << sh.nHinge() << " 2\n";
        for (size_t t = 0; t < nTri; ++t) {
            for (int k = 0; k < 4; ++k) out << B[k * nTri + t] << " ";
            out << alpha[t] << "\n";
        }
        for (size_t i = 0; i < nH; ++i) out << thetaBar[i] << " " << alphaB[i] << "\n";
    }
    if (!out.good()) throw StateError("write error on status file " + path);
}

// restart branch of the Optimizer constructor (Optimizer.cpp:179-248): same token grammar, then V_prev = V and computeXTilta
void HipOptimizer::loadStatus(const std::string& path)
{
    specAsmValid = false;
    std::ifstream in(path);
    if (!in.is_open()) throw StateError("unable to open status file " + path);
    const size_t n3 = 3 * (size_t)mesh.nV;
    std::vector<double> x(n3), vel(n3, 0.0), acc(n3, 0.0), dx(n3, 0.0);
    mesh.d_x.download(x.data(), n3, stream);
    HIP_CHECK(hipStreamSynchronize(stream));
    auto readRows = [&](std::stringstream& ss, std::vector<double>& dst, bool zeroFirst) {
        int rowsIn = 0, dimIn = 0;
        ss >> rowsIn >> dimIn;
        if (rowsIn < 0 || rowsIn > mesh.nV || dimIn != 3) throw StateError("status file does not match the mesh");
        if (ss.fail()) throw StateError("malformed section header in status file " + path);
        if (zeroFirst) std::fill(dst.begin(), dst.end(), 0.0);
        for (int v = 0; v < rowsIn; ++v) in >> dst[3 * (size_t)v] >> dst[3 * (size_t)v + 1] >> dst[3 * (size_t)v + 2];
        // a truncated or malformed section leaves failbit set: a restart from a corrupt checkpoint must not go on with
        // partly read (or stale) arrays
        if (in.fail()) throw StateError("truncated or malformed section in status file " + path);
    };
    std::vector<double> plasticA, plasticAlpha; // the plastic section, where the file has one
    FiberPlan fiberIn; // the fiber section, where the file has one
    std::vector<double> shellB, shellAlpha, shellThetaBar, shellAlphaB; // the shellplastic section, where the file has one
    bool shellPlasticIn = false;
    std::string line;
    while (std::getline(in, line)) {
        std::stringstream ss(line);
        std::string token;
        ss >> token;
        if (token == "timestep") ss >> globalIterNum;
        else if (token == "position") readRows(ss, x, false);
        else if (token == "velocity") {
            long long n = 0;
            ss >> n;
            if (n < 0 || n > (long long)n3) throw StateError("status file does not match the mesh");
            std::fill(vel.begin(), vel.end(), 0.0);
            for (long long i = 0; i < n; ++i) in >> vel[i];
            if (in.fail()) throw StateError("truncated or malformed velocity section in status file " + path);
        }
        else if (token == "acceleration") readRows(ss, acc, true);
        else if (token == "dx_Elastic") readRows(ss, dx, true);
        else if (token == "plastic") {
            int rowsIn = 0, dimIn = 0;
            ss >> rowsIn >> dimIn;
            if (ss.fail()) throw StateError("malformed section header in status file " + path);
            if (rowsIn != mesh.nT || dimIn != 10) throw StateError("status file does not match the mesh");
            const size_t nT = (size_t)mesh.nT;
            plasticA.assign(9 * nT, 0.0);
            plasticAlpha.assign(nT, 0.0);
            for (size_t t = 0; t < nT; ++t) {
                for (int k = 0; k < 9; ++k) in >> plasticA[k * nT + t];
                in >> plasticAlpha[t];
            }
            if (in.fail()) throw StateError("truncated or malformed plastic section in status file " + path);
        }
        else if (token == "shellplastic") {
            int rowsIn = 0, dimIn = 0, hingesIn = 0, hdimIn = 0;
            ss >> rowsIn >> dimIn >> hingesIn >> hdimIn;
            if (ss.fail()) throw StateError("malformed section header in status file " + path);
            if (!mesh.shell.nTri() || rowsIn != mesh.shell.nTri() || dimIn != 5 || hingesIn != mesh.shell.nHinge() || hdimIn != 2) throw StateError("status file does not match the shell");
            const size_t nTri = (size_t)rowsIn, nH = (size_t)hingesIn;
            shellB.assign(4 * nTri, 0.0);
            shellAlpha.assign(nTri, 0.0);
            shellThetaBar.assign(nH, 0.0);
            shellAlphaB.assign(nH, 0.0);
            for (size_t t = 0; t < nTri; ++t) {
                for (int k = 0; k < 4; ++k) in >> shellB[k * nTri + t];
                in >> shellAlpha[t];
            }
            for (size_t i = 0; i < nH; ++i) in >> shellThetaBar[i] >> shellAlphaB[i];
            if (in.fail()) throw StateError("truncated or malformed shellplastic section in status file " + path);
            shellPlasticIn = true;
        }
        else if (token == "fiber") {
            int rowsIn = 0, dimIn = 0, groupsIn = 0;
            ss >> rowsIn >> dimIn >> groupsIn;
            if (ss.fail()) throw StateError("malformed section header in status file " + path);
            if (rowsIn != mesh.nT || dimIn != 7 || groupsIn != FIBER_MAX_GROUPS) throw StateError("status file does not match the mesh");
            const size_t nT = (size_t)mesh.nT;
            std::vector<double> act(FIBER_MAX_GROUPS), k(nT), k2(nT), dir(3 * nT);
            std::vector<int> flags(nT), group(nT);
            for (double& v : act) in >> v;
            for (size_t t = 0; t < nT; ++t) in >> k[t] >> k2[t] >> flags[t] >> group[t] >> dir[3 * t] >> dir[3 * t + 1] >> dir[3 * t + 2];
            if (in.fail()) throw StateError("truncated or malformed fiber section in status file " + path);
            // the rows go through the plan's own calls, in the order a caller would make them: one set of rules (fiber_plan.h).  The plan normalises the
            // direction again; the file's own is kept where it is that unit vector to rounding, so that a restart continues to the bit
            std::string err;
            auto bad = [&](const std::string& what) { return StateError("fiber section of status file " + path + ": " + what); };
            const double none[3] = { 1.0, 0.0, 0.0 };
            if (!setFiberRange(fiberIn, mesh.nT, 0, 0, none, false, 0.0, 0, 0.0, false, 0, err)) throw bad(err); // no fibre anywhere
            for (int g = 0; g < FIBER_MAX_GROUPS; ++g)
                if (!setFiberActivation(fiberIn, g, act[g], err)) throw bad(err);
            for (size_t t = 0; t < nT; ++t) {
                if (k[t] == 0.0) continue;
                if (worldSize > 1) throw UnsupportedError("fibres on a sharded context");
                if (flags[t] != 0 && flags[t] != FIBER_FLAG_EXP && flags[t] != FIBER_FLAG_TENSION_ONLY) throw bad("element " + std::to_string(t) + ": unknown flag word");
                const bool isExp = flags[t] == FIBER_FLAG_EXP;
                if (!setFiberRange(fiberIn, mesh.nT, (int)t, (int)t + 1, &dir[3 * t], false, k[t], isExp ? FIBER_LAW_EXP : FIBER_LAW_SPRING, k2[t], flags[t] == FIBER_FLAG_TENSION_ONLY,
                        group[t], err))
                    throw bad("element " + std::to_string(t) + ": " + err);
                for (int r = 0; r < 3; ++r) {
                    if (!(std::fabs(fiberIn.dir[r * nT + t] - dir[3 * t + r]) <= 4.0 * DBL_EPSILON)) throw bad("element " + std::to_string(t) + ": the direction is no unit vector");
                    fiberIn.dir[r * nT + t] = dir[3 * t + r];
                }
                if (mesh.plastic.on() && mesh.plastic.plan.yield[t] < INFINITY) throw bad("element " + std::to_string(t) + " is plastic in this context");
            }
        }
    }
    if (in.bad()) throw StateError("read error on status file " + path);
    mesh.d_x.upload(x, stream);
    mesh.shell.limitUnchecked = mesh.shell.nLimited() > 0;
    mesh.shell.rubberUnchecked = mesh.shell.nRubber() > 0;
    d_xPrev.upload(x, stream);
    d_xStepStart.upload(x, stream); // V_prev = V (Optimizer.cpp:247): a report right after a restart has no kinetic part
    d_vel.upload(vel, stream);
    d_acc.upload(acc, stream);
    d_dxElastic.upload(dx, stream);
    if (!plasticA.empty()) { // (a file without the section leaves A and alpha untouched)
        mesh.ensurePlastic(stream);
        HIP_CHECK(hipMemcpyAsync(mesh.d_A.p, plasticA.data(), plasticA.size() * sizeof(double), hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(mesh.plastic.d_alpha.p, plasticAlpha.data(), plasticAlpha.size() * sizeof(double), hipMemcpyHostToDevice, stream));
    }
    if (shellPlasticIn) { // (a file without the section leaves the shell's records and history untouched)
        if (worldSize > 1) throw UnsupportedError("shell plasticity on a sharded context");
        mesh.ensureShellPlastic(stream);
        HipShell& sh = mesh.shell;
        HIP_CHECK(hipMemcpyAsync(sh.d_triConst.p, shellB.data(), shellB.size() * sizeof(double), hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipMemcpyAsync(sh.plastic.d_alpha.p, shellAlpha.data(), shellAlpha.size() * sizeof(double), hipMemcpyHostToDevice, stream));
        if (!shellThetaBar.empty()) {
            HIP_CHECK(hipMemcpyAsync(sh.d_hingeConst.p, shellThetaBar.data(), shellThetaBar.size() * sizeof(double), hipMemcpyHostToDevice, stream));
            HIP_CHECK(hipMemcpyAsync(sh.plastic.d_alphaB.p, shellAlphaB.data(), shellAlphaB.size() * sizeof(double), hipMemcpyHostToDevice, stream));
        }
    }
    HIP_CHECK(hipStreamSynchronize(stream));
    if (fiberIn.nT) { // (a file without the section leaves the fibres untouched)
        mesh.fiber.plan = std::move(fiberIn);
        mesh.uploadFibers(stream);
    }
    computeXTilta();
}

void HipOptimizer::setVelocity(const double* vel3nV)
{
    HIP_CHECK(hipMemcpyAsync(d_vel.p, vel3nV, 3 * (size_t)mesh.nV * sizeof(double), hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    computeXTilta();
}

void HipOptimizer::computeConstraintSets()
{
    if (!ipOn()) return;
    Tic t(timers[14], stream);
    for (auto* h : colliders) h->build(contact->nSVI, contact->d_SVI.p, mesh.d_x.p, mesh.d_dbc.p, dHat); // Optimizer.cpp:2460-2462
    if (selfCollision) contact->buildConstraintSet(mesh, mesh.d_x.p, mesh.d_dbc.p, dHat); // Optimizer.cpp:2448-2470
}

bool HipOptimizer::isIntersected() { return contact->isIntersected(mesh, mesh.d_x.p, mesh.d_dbc.p); }

double HipOptimizer::kappaFloor() const
{
    // suggestKappa (Optimizer.cpp:2228-2233): kappaMinMultiplier (1e11, Config.hpp:139) * mean nodal mass / (4e-16 L^2 b''(1e-16 L^2))
    const double d = 1.0e-16 * mesh.bboxDiag2, t2 = d - dHat, lg = std::log(d / dHat);
    const double Hb = (lg * -2.0 - t2 * 4.0 / d) + 1.0 / (d * d) * (t2 * t2); // BarrierFunctions.hpp:76-83
    double avgMass = 0; // Mesh::avgNodeMass(dim): over the nodes of the tetrahedral components (Mesh.cpp:576-609)
    for (int v = 0; v < mesh.nV; ++v)
        if (!mesh.nElemNodes || mesh.inMesh[v]) avgMass += mesh.mass[v];
    avgMass /= std::max(mesh.nElemNodes, 1);
    return kappaMinMultiplier * avgMass / (4.0e-16 * mesh.bboxDiag2 * Hb);
}

void HipOptimizer::initKappa()
{
    // Optimizer.cpp:2236-2313: balance the barrier gradient of the active set against elasticity + inertia.  Once per time step; the two dot products are taken
    // on the device (round 6: both gradients used to travel to the host, 2 x 24 nV bytes per time step, to be dotted there)
    if (!nConstraints()) return;
    const int n3 = 3 * mesh.nV;
    elasticInertiaGradient(true); // computeGradient with solveIP == false (:2243-2245)
    if (dampingStiff > 0.0) dampingGradientAdd(true, d_gradient.p); // still part of it (:3519-3540)
    d_minusG.zero(stream);
    barrierGradientAdd(true, 1.0, true, d_minusG.p); // also clears the DBC rows (:2275-2277)
    launch_dot2(n3, d_minusG.p, d_gradient.p, d_partial.p, (int)d_partial.n, slot(S_KAPPA_NUM), stream);
    publish(S_KAPPA_NUM, slotSpan(S_KAPPA_NUM, S_KAPPA_DEN));
    HIP_CHECK(hipStreamSynchronize(stream));
    const double num = published(S_KAPPA_NUM), den = published(S_KAPPA_DEN);
    double minKappa = -num / den;
    if (minKappa > 0.0) kappa = minKappa;
    minKappa = kappaFloor();
    if (kappa < minKappa) kappa = minKappa;
    const double kappaMax = 100 * kappaFloor(); // upperBoundKappa, :2216-2225
    if (kappa > kappaMax) kappa = kappaMax;
}

void HipOptimizer::postLineSearch()
{
    // Optimizer.cpp:2357-2445 (ADAPTIVE_KAPPA)
    if (!ipOn()) return;
    if (kappa == 0.0) {
        initKappa();
        return;
    }
    std::vector<double> d;
    bool updateKappa = false;
    for (size_t ci = 0; ci < colliders.size() && !updateKappa; ++ci) {
        std::vector<int> verts;
        std::vector<double> was;
        for (size_t i = 0; i < closeHS.size(); ++i)
            if (closeHS[i].first == (int)ci) {
                verts.push_back(closeHS[i].second);
                was.push_back(closeHSVal[i]);
            }
        colliders[ci]->evalDist2(verts, mesh.d_x.p, d);
        for (size_t i = 0; i < verts.size(); ++i)
            if (d[i] <= was[i]) updateKappa = true;
    }
    if (!updateKappa && selfCollision) {
        contact->evalStencils(closeID, mesh.d_x.p, d);
        for (size_t i = 0; i < closeID.size(); ++i)
            if (d[i] <= closeVal[i]) {
                updateKappa = true;
                break;
            }
    }
    if (updateKappa) {
        kappa *= 2.0;
        const double kappaMax = 100 * kappaFloor();
        if (kappa > kappaMax) kappa = kappaMax;
    }
    closeID.clear();
    closeVal.clear();
    closeHS.clear();
    closeHSVal.clear();
    for (size_t ci = 0; ci < colliders.size(); ++ci) {
        const std::vector<int>& set = colliders[ci]->set;
        colliders[ci]->evalDist2(set, mesh.d_x.p, d);
        for (size_t i = 0; i < set.size(); ++i)
            if (d[i] < dTol) {
                closeHS.push_back({ (int)ci, set[i] });
                closeHSVal.push_back(d[i]);
            }
    }
    if (!selfCollision) return;
    // ... and, in the same batch, whether the pattern holds every block of the sets the next assembly will use (computePrecondMtr asks first thing)
    int cov = 1;
    contact->closeStencils(mesh.d_x.p, dTol, closeID, closeVal, &lin, &cov);
    coverSets = contact->setsVersion;
    coverPattern = lin.patternVersion;
    coverAnswer = cov != 0;
}

void HipOptimizer::ensurePatchPlan()
{
    if (patchVersion == lin.patternVersion && patch.valid) return;
    patch.build(mesh, lin, stream);
    patchVersion = lin.patternVersion;
}
bool HipOptimizer::ownerMode() const
{
    // both halves sharded, and nothing in play that reads the WHOLE matrix every iteration (the lagged damping matrix is a second value array on the pattern
    // that enters energy and gradient through products with it: those runs keep the all-reduce of the values)
    return worldSize > 1 && lin.solverWorld() == worldSize && lin.solverType == 0 && lin.analyzed() && !(dampingStiff > 0.0); // (before the first analysis: the older scheme)
}

void HipOptimizer::ensureOwnerPlan()
{
    ensurePatchPlan();
    if (ownerPlanPatch == patchVersion && ownerPlanAnalysis == lin.analysisVersion) return;
    std::vector<int> owner;
    lin.nodeOwners(owner); // rank of the subtree that eliminates the node, -1 above the cut
    const int nV = mesh.nV;
    std::vector<unsigned char> need(nV, 0), mine(nV, 0);
    ownerNeededNodes = 0;
    for (int v = 0; v < nV; ++v) {
        const int o = (v < (int)owner.size()) ? owner[v] : -1;
        need[v] = (o < 0 || o == rank) ? 1 : 0;
        mine[v] = (o == rank || (o < 0 && rank == 0)) ? 1 : 0;
        ownerNeededNodes += need[v];
    }
    std::vector<int> list;
    const std::vector<int>&np = patch.topo.nodePtr, &nodes = patch.topo.nodes;
    for (int p = 0; p + 1 < (int)np.size(); ++p) {
        bool any = false;
        for (int j = np[p]; j < np[p + 1] && !any; ++j) any = need[nodes[j]] != 0;
        if (any) list.push_back(p);
    }
    nOwnerPatches = (int)list.size();
    if (list.empty()) list.push_back(0);
    d_ownerPatches.upload(list, stream);
    d_need.upload(need, stream);
    d_mine.upload(mine, stream);
    HIP_CHECK(hipStreamSynchronize(stream));
    ownerPlanPatch = patchVersion;
    ownerPlanAnalysis = lin.analysisVersion;
}

void HipOptimizer::maskAndReduceGradient(double* g)
{
    launch_keep_mine3(mesh.nV, d_mine.p, g, stream);
    reduceSum(g, 3LL * mesh.nV);
}

void HipOptimizer::completeMatrix()
{
    if (matrixComplete || worldSize <= 1) return;
    launch_keep_mine_rows(lin.numRows, d_mine.p, lin.d_ia.p, lin.d_a.p, stream);
    reduceSum(lin.d_a.p, (long long)lin.ja.size());
    matrixComplete = true;
}

void HipOptimizer::patchShard(int& pb, int& pe) const
{
    pb = (int)((long long)patch.nPatches * rank / worldSize);
    pe = (int)((long long)patch.nPatches * (rank + 1) / worldSize);
}

void HipOptimizer::barrierGradientAdd(bool projectDBC, double kappa_, bool activeOnly, double* grad_dev, int part)
{
    // barrier forces of the half-spaces and of the mesh against itself; the projected rows are cleared again at the end
    // (Optimizer.cpp:3452-3516).  activeOnly: initKappa leaves the mollified parallel-edge set out (:2262-2270)
    // part (owner-computes sharding): 0 = everything; 1 = only the self-contact stencils this rank evaluates, BEFORE the gradient exchange; 2 = the terms every
    // rank evaluates alike (half-spaces, lagged friction), after it
    if (part == 1) {
        if (contact && selfCollision)
            contact->gradientAdd(mesh.d_x.p, mesh.d_dbc.p, mesh.nV, dHat, kappa_, 0, grad_dev, true, !activeOnly, d_need.p);
        return;
    }
    for (auto* h : colliders) h->gradientAdd(mesh.d_x.p, dHat, kappa_, grad_dev);
    if (!activeOnly && fricDHat > 0.0) { // Optimizer.cpp:3474-3478, 3504-3506
        for (auto* h : colliders)
            if (h->friction > 0.0) h->frictionGradientAdd(mesh.d_x.p, d_xPrev.p, fricDHat, grad_dev);
        if (selfCollision && selfFric > 0.0) contact->frictionGradientAdd(mesh.d_x.p, d_xPrev.p, fricDHat, selfFric, grad_dev);
    }
    if (!contact) return;
    if (part == 2) { // the stencils went in before the exchange: only the projected rows are left to clear
        launch_clear_projected(mesh.nV, mesh.d_dbc.p, projectDBC ? 1 : 0, grad_dev, stream);
        return;
    }
    if (ownerMode() && !lin.rowBase.empty()) {
        // a caller outside computeGradient (initKappa's barrier-only gradient): this rank's stencils into a zeroed scratch vector, the designated entries
        // exchanged, the sum on top of the caller's vector
        ensureOwnerPlan();
        const size_t n3 = 3 * (size_t)mesh.nV;
        d_contactG.ensure(n3);
        d_contactG.zeroN(n3, stream);
        contact->gradientAdd(mesh.d_x.p, mesh.d_dbc.p, mesh.nV, dHat, kappa_, 0, d_contactG.p, selfCollision, selfCollision && !activeOnly, d_need.p);
        maskAndReduceGradient(d_contactG.p);
        launch_axpy((long long)n3, 1.0, d_contactG.p, grad_dev, stream);
        launch_clear_projected(mesh.nV, mesh.d_dbc.p, projectDBC ? 1 : 0, grad_dev, stream);
        return;
    }
    contact->gradientAdd(mesh.d_x.p, mesh.d_dbc.p, mesh.nV, dHat, kappa_, projectDBC, grad_dev, selfCollision, selfCollision && !activeOnly);
}

void HipOptimizer::elasticInertiaGradient(bool projectDBC, bool finish)
{
    if (lin.rowBase.empty() || shellOnly()) { // no pattern yet (or no tetrahedron, hence no patch plan): tet-parallel atomic path
        launch_node_init(view(), projectDBC, rank == 0, nullptr, d_gradient.p, stream);
        launch_assemble(view(), elasticCoef(), projectDBC, d_gradient.p, nullptr, stream);
        codimAssembleAdd(elasticCoef(), projectDBC, d_gradient.p, nullptr);
        reduceSum(d_gradient.p, 3LL * mesh.nV);
        neumannGradientAdd(d_gradient.p);
        return;
    }
    ensurePatchPlan();
    if (ownerMode()) { // this rank's patches only; the caller (computeGradient) adds its share of the barrier forces and exchanges the sum once
        ensureOwnerPlan();
        d_gradient.zero(stream);
        launch_assemble_patches(view(), patch, 0, nOwnerPatches, elasticCoef(), projectDBC, d_gradient.p, nullptr, stream, d_ownerPatches.p);
        if (finish) { // a caller that wants the elastic + inertia gradient by itself (initKappa)
            maskAndReduceGradient(d_gradient.p);
            neumannGradientAdd(d_gradient.p);
        }
        return;
    }
    int pb, pe;
    patchShard(pb, pe);
    if (worldSize > 1) d_gradient.zero(stream);
    launch_assemble_patches(view(), patch, pb, pe, elasticCoef(), projectDBC, d_gradient.p, nullptr, stream);
    codimAssembleAdd(elasticCoef(), projectDBC, d_gradient.p, nullptr);
    reduceSum(d_gradient.p, 3LL * mesh.nV);
    neumannGradientAdd(d_gradient.p);
}

void HipOptimizer::computeGradient(bool projectDBC)
{
    const bool owner = ownerMode() && !lin.rowBase.empty();
    elasticInertiaGradient(projectDBC, !owner);
    if (owner) {
        ownerGradientTail(projectDBC);
        return;
    }
    if (ipOn()) barrierGradientAdd(projectDBC, kappa, false, d_gradient.p);
    penaltyGradientAdd(projectDBC);
}

// owner-computes: d_gradient holds the elastic + inertia forces of this rank's patches; its share of the self-contact stencils (those that touch a node it owns
// rows of) goes on top, then ONE exchange in which every node is contributed by its designated rank; what is evaluated identically everywhere follows
void HipOptimizer::ownerGradientTail(bool projectDBC)
{
    if (ipOn()) barrierGradientAdd(projectDBC, kappa, false, d_gradient.p, 1);
    maskAndReduceGradient(d_gradient.p);
    neumannGradientAdd(d_gradient.p);
    if (ipOn()) barrierGradientAdd(projectDBC, kappa, false, d_gradient.p, 2);
    penaltyGradientAdd(projectDBC);
}

// tail of Optimizer::computeGradient when the Dirichlet rows are not all projected: rows of the nodes that still are get
// cleared (Optimizer.cpp:3512-3516; with projectDBC the element pass never wrote them), then augmentMDBCGradient (:3542-3544)
void HipOptimizer::penaltyGradientAdd(bool projectDBC)
{
    if (dampingStiff > 0.0) dampingGradientAdd(projectDBC, d_gradient.p); // Optimizer.cpp:3519-3540 (rows of D of Dirichlet nodes are empty)
    if (projectDBC) return;
    launch_clear_projected(mesh.nV, mesh.d_dbc.p, 0, d_gradient.p, stream);
    if (rhoDBC && !tpIds.empty()) launch_mdbc_gradient(mdbc(), mesh.d_x.p, rhoDBC, d_gradient.p, stream);
}

void HipOptimizer::computePrecondMtr(bool projectDBC, bool withGradient)
{
    if (lin.rowBase.empty()) throw StateError("computePrecondMtr needs a pattern built by set_pattern");
    static const bool timeIt = std::getenv("IPCGPU_PATTERN_TIMES") != nullptr; // stderr: where a pattern change spends its time
    auto tLap = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (!timeIt) return;
        HIP_CHECK(hipStreamSynchronize(stream));
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "pattern change: %-34s %.2f ms\n", what, std::chrono::duration<double, std::milli>(now - tLap).count());
        tLap = now;
    };
    if (!patternCoversContact()) {
        lap("coverage check");
        growPattern(lap);
    }
    const bool planStale = !(patchVersion == lin.patternVersion && patch.valid);
    ensurePatchPlan();
    if (planStale) lap("patch plan");
    assembleSystem(projectDBC, withGradient);
}

bool HipOptimizer::patternCoversContact()
{
    // The common case by far: the pattern already holds every block the current sets need (it only grows, and it is built with
    // look-ahead).  One small kernel answers that; the host-side connectivity (hundreds of thousands of pairs to build, filter
    // and sort) runs only when a pair is missing.  Lagged friction keeps its own set: always the host path there.
    if (!selfCollision) return true;
    if (fricDHat > 0.0 && selfFric > 0.0) return false;
    // (the coverage answer usually arrived with the close-stencil bookkeeping at the end of the last iteration, postLineSearch: same sets, same pattern)
    const bool cached = coverSets == contact->setsVersion && coverPattern == lin.patternVersion;
    return cached ? coverAnswer : contact->patternCovers(lin);
}

// the pattern follows the contact connectivity (augmentConnectivity into vNeighbor_IP, Optimizer.cpp:3560-3612); which pairs make it grow, and to what:
// ContactPattern (contact_pattern.h)
void HipOptimizer::growPattern(const std::function<void(const char*)>& lap)
{
    // The connectivity of the live sets on the host (read-back of the tuples, node pairs, filter, sort: 1-2 ms at 40 K nodes) is needed only for the lagged
    // friction set and for a look-ahead below 1.  Otherwise (round 6) the device has already said that the pattern lacks a block of the live sets -- a new
    // analysis is certain --, and the look-ahead list below, the FULL stencils of every candidate within lookahead() x dHat >= dHat, contains every node pair
    // of the live sets: their stencils are sub-stencils of candidates, the mollified pairs' four nodes are their candidates' four nodes.
    const bool frictionPairs = fricDHat > 0.0 && selfFric > 0.0;
    const bool liveOnHost = frictionPairs || lookahead() < 1.0;
    NodePairs live;
    if (liveOnHost) {
        if (contact->nActive() + contact->nPara()) contact->connectivity(live);
        if (frictionPairs) contact->frictionConnectivity(live); // lagged set (:3565-3566)
        live = nonMeshPairs(live, mesh.nbPtr.data(), mesh.nb.data());
    }
    lap("connectivity of the live sets");
    // Look-ahead: contact spreads, so the next iterations bring pairs that are a little farther apart now.  The new
    // pattern is built from the constraint set at a larger distance (lookahead() * dHat, squared distances): its
    // blocks hold explicit zeros until the pairs become active, and pattern + symbolic analysis (tens of ms on the
    // host) are needed far less often.  Costs two extra constraint-set builds per analysis.
    auto lookAheadPairs = [&] {
        NodePairs ahead;
        const double pad = lookahead();
        if (pad >= 1.0) {
            if (pad > 1.0) contact->buildConstraintSet(mesh, mesh.d_x.p, mesh.d_dbc.p, pad * dHat);
            contact->candidateConnectivitySorted(ahead); // full stencils: closest-feature changes need no new blocks; sorted, unique
            if (pad > 1.0) contact->buildConstraintSet(mesh, mesh.d_x.p, mesh.d_dbc.p, dHat); // back to the real sets
            ahead = nonMeshPairs(ahead, mesh.nbPtr.data(), mesh.nb.data());
        }
        lap("look-ahead sets + connectivity");
        return ahead;
    };
    if (!contactPattern.grow(liveOnHost ? &live : nullptr, lookAheadPairs)) return;
    nPatternChanges++;
    lap("union + flatten");
    {
        Tic t(timers[1], stream);
        lin.set_pattern(mesh, (int)contactPattern.pairs().size(), contactPattern.flat().data());
    }
    lap("set_pattern");
    {
        // the assembly plan of the new pattern is built on a second host thread while this one runs the symbolic analysis:
        // both only read the pattern, and the GPU is idle either way
        int dev = 0;
        HIP_CHECK(hipGetDevice(&dev));
        std::exception_ptr planErr;
        std::thread planThread([&] {
            try {
                HIP_CHECK(hipSetDevice(dev));
                ensurePatchPlan();
            }
            catch (...) {
                planErr = std::current_exception();
            }
        });
        std::exception_ptr anaErr;
        try {
            Tic t(timers[2], stream);
            lin.analyze_pattern(&mesh);
        }
        catch (...) {
            anaErr = std::current_exception();
        }
        planThread.join();
        if (anaErr) std::rethrow_exception(anaErr);
        if (planErr) std::rethrow_exception(planErr);
    }
    lap("analyze_pattern + patch plan");
}

// setZero (Optimizer.cpp:3616), elastic Hessian (:3619-3623) and the mass / DBC diagonal (:3638-3668) are one pass: every owned CSR row is written exactly
// once by the patch that owns its node; the barrier, friction, damping and penalty terms go on top.  Two schemes for several ranks:
// Owner-computes (round 4): this rank's patches write the complete CSR rows of the nodes it owns or shares, its share of the contact stencils adds their
// blocks to those rows -- and that is all its fronts ever read (an entry belongs to the front of whichever of its two nodes is eliminated first; the other
// node then sits in the same subtree or above the cut).  No matrix value crosses ranks.  The rows of other ranks' nodes stay zero.
// The older scheme, kept for contexts whose solver is not sharded: a slice of the patches per rank, partial matrices summed by one all-reduce of the values;
// the contact stencils are then evaluated alike on every rank, after the exchange.
void HipOptimizer::assembleSystem(bool projectDBC, bool withGradient)
{
    const bool owner = ownerMode();
    int pb = 0, pe = 0;
    if (owner) {
        ensureOwnerPlan();
        pe = nOwnerPatches;
    }
    else patchShard(pb, pe);
    if (worldSize > 1) {
        lin.setZero();
        if (withGradient) d_gradient.zero(stream);
    }
    if (shellOnly()) { // no patch plan: the node pass writes mass / identity on a cleared matrix and the inertia term of the gradient
        lin.setZero();
        launch_node_init(view(), projectDBC, rank == 0, lin.d_a.p, withGradient ? d_gradient.p : nullptr, stream);
    }
    launch_assemble_patches(view(), patch, pb, pe, elasticCoef(), projectDBC, withGradient ? d_gradient.p : nullptr, lin.d_a.p, stream,
        owner ? d_ownerPatches.p : nullptr);
    codimAssembleAdd(elasticCoef(), projectDBC, withGradient ? d_gradient.p : nullptr, lin.d_a.p);
    matrixComplete = !owner;
    if (owner) {
        if (withGradient) ownerGradientTail(projectDBC);
    }
    else {
        if (worldSize > 1) {
            reduceSum(lin.d_a.p, (long long)lin.ja.size());
            if (withGradient) reduceSum(d_gradient.p, 3LL * mesh.nV);
        }
        if (withGradient) {
            neumannGradientAdd(d_gradient.p);
            if (ipOn()) barrierGradientAdd(projectDBC, kappa, false, d_gradient.p);
        }
    }
    if (ipOn()) { // barrier blocks, PSD-projected per stencil (Optimizer.cpp:3625-3636, 3670-3676)
        // (half-spaces and lagged friction: vertex-wise diagonal blocks / one set, evaluated alike on every rank and added to the rows each rank holds)
        for (auto* h : colliders)
            h->hessianAdd(mesh.d_x.p, mesh.d_dbc.p, lin.d_rowBase.p, lin.d_rowLen.p, dHat, kappa, projectDBC, lin.d_a.p);
        if (selfCollision) // owner-computes: the stencils that touch a row this rank needs
            contact->hessianAdd(mesh.d_x.p, mesh.d_dbc.p, lin, dHat, kappa, projectDBC, lin.d_a.p, owner ? d_need.p : nullptr, /*deferCheck=*/true);
        if (fricDHat > 0.0) { // Optimizer.cpp:3677-3702
            for (auto* h : colliders)
                if (h->friction > 0.0)
                    h->frictionHessianAdd(mesh.d_x.p, d_xPrev.p, mesh.d_dbc.p, lin.d_rowBase.p, lin.d_rowLen.p, fricDHat, projectDBC, lin.d_a.p);
            if (selfCollision && selfFric > 0.0)
                contact->frictionHessianAdd(mesh.d_x.p, d_xPrev.p, mesh.d_dbc.p, lin, fricDHat, selfFric, projectDBC, lin.d_a.p);
        }
    }
    if (dampingStiff > 0.0) { // addCoeff(dampingMtr, 1.0), Optimizer.cpp:3707-3709 (never in owner mode: ownerMode())
        if (dampPatternVersion != lin.patternVersion) assembleDampingMtr();
        launch_axpy((long long)lin.ja.size(), 1.0, d_damp.p, lin.d_a.p, stream);
    }
    if (withGradient && !owner) penaltyGradientAdd(projectDBC); // (the owner's came with its gradient tail)
    if (!projectDBC && rhoDBC && !tpIds.empty()) launch_mdbc_hessian(mdbc(), lin.d_ia.p, rhoDBC, lin.d_a.p, stream); // :3711-3713
}

bool HipOptimizer::checkInversion(bool meshQuery)
{
    // Optimizer.cpp:252,517,545,2710: only under getNeedElemInvSafeGuard().  meshQuery: the caller asks about the mesh, not on behalf of the material
    if (!mesh.needElemInvSafeGuard() && !meshQuery) return true;
    d_flag.zero(stream);
    launch_check_inversion(view(), d_flag.p, stream);
    launch_publish(d_flag.p, h_flag.dev, 1, stream);
    HIP_CHECK(hipStreamSynchronize(stream));
    int f = h_flag.p[0];
    if (worldSize > 1) {
        h_scalar.p[S_INVERSION_SUM] = (double)f; // (the one host write into the mirror: its own position is the pinned staging word of the upload)
        HIP_CHECK(hipMemcpyAsync(slot(S_INVERSION_SUM), h_scalar.p + S_INVERSION_SUM, sizeof(double), hipMemcpyHostToDevice, stream));
        reduceSum(slot(S_INVERSION_SUM), 1);
        f = readScalar(S_INVERSION_SUM) != 0.0;
    }
    return f == 0;
}

double HipOptimizer::fullCcd(double slackness, double stepSize)
{
    if (contact->ccdMode == 1) {
        int arg3[3];
        const double a = contact->ccdFullReference(mesh, mesh.d_x.p, d_searchDir.p, mesh.d_dbc.p, slackness, stepSize, nullptr, arg3, nullptr);
        lastCCDPair[0] = arg3[1];
        lastCCDPair[1] = arg3[2];
        return a;
    }
    return contact->ccdFull(mesh, mesh.d_x.p, d_searchDir.p, mesh.d_dbc.p, slackness, stepSize, lastCCDPair, nullptr);
}

double HipOptimizer::filterStepSize(const double* p_dev, double stepSize)
{
    // Energy.cpp:565-581: min over elements of the root, applied only when 0 < min < stepSize
    if (!mesh.needElemInvSafeGuard()) return stepSize; // :567 needElemInvSafeGuard
    launch_fill(slot(S_STEP_FILTER), 1, 1e20, stream);
    launch_inversion_step(view(), p_dev, 0.2, stepSize, slot(S_STEP_FILTER), stream);
    reduceMin(slot(S_STEP_FILTER), 1);
    const double t = readScalar(S_STEP_FILTER);
    if (t > 0.0 && t < stepSize) stepSize = t;
    return stepSize;
}

void HipOptimizer::stepForward(const double* x0_dev, double alpha)
{
    launch_step_forward(3 * mesh.nV, x0_dev, d_searchDir.p, alpha, mesh.d_x.p, stream);
}

#ifndef ASM_TIME_EVERY
#define ASM_TIME_EVERY 8
#endif
void HipOptimizer::speculativeAssembly()
{
    specAsmValid = false;
    if (!fastPath() || !projDBC || lin.rowBase.empty()) return;
    ensurePatchPlan();
    d_aSpec.alloc(lin.d_a.n); // same capacity as the solver's value array: the two are swapped
    d_gradSpec.alloc(d_gradient.n);
    // The assembly bucket of the timers is fed by a pair of events around the launch -- on every ASM_TIME_EVERY-th launch only, counted ASM_TIME_EVERY times
    // (round 6): a timing event is a barrier packet that drains the stream in front of the assembly and behind it, every iteration, for a bucket that holds 2 % of it
    const bool timeIt = (asmLaunches++ % ASM_TIME_EVERY) == 0;
    if (timeIt) {
        resolveEventTimers(); // (the last timed assembly: finished long ago)
        HIP_CHECK(hipEventRecord(evAsm0, stream));
    }
    if (shellOnly()) {
        HIP_CHECK(hipMemsetAsync(d_aSpec.p, 0, sizeof(double) * lin.ja.size(), stream));
        launch_node_init(view(), 1, true, d_aSpec.p, d_gradSpec.p, stream);
    }
    launch_assemble_patches(view(), patch, 0, patch.nPatches, elasticCoef(), 1, d_gradSpec.p, d_aSpec.p, stream); // what computePrecondMtr(true, true) launches on this path
    codimAssembleAdd(elasticCoef(), true, d_gradSpec.p, d_aSpec.p);
    if (timeIt) {
        HIP_CHECK(hipEventRecord(evAsm1, stream));
        evAsmPending = true;
        evAsmWeight = ASM_TIME_EVERY; // (this pair stands for ASM_TIME_EVERY launches)
    }
    specAsmValid = true;
}

// |p|_inf of the search direction into S_DIR_NORM (convergence test of the next pass, Optimizer.cpp:1869-1879): enqueued, the caller publishes or reads it
void HipOptimizer::enqueueDirNorm()
{
    launch_fill(slot(S_DIR_NORM), 1, 0.0, stream);
    launch_max_abs(3 * mesh.nV, d_searchDir.p, slot(S_DIR_NORM), stream);
}

void HipOptimizer::computeSearchDir()
{
    bool ok;
    // The multifrontal solver takes the sign in the pass that permutes its right-hand side: no vector pass for -g on that path, where the diagonal fallback
    // below forms d_minusG when it is taken.  The other solver types take d_minusG as their right-hand side as before.  (Elsewhere the buffer is scratch: the
    // barrier gradient of the kappa update, the output of ipcgpu_bench_factor_solve.)
    const bool signInSolver = lin.solverType == 0;
    const double* const rhs = signInSolver ? d_gradient.p : d_minusG.p;
    if (!signInSolver) launch_negate(3 * mesh.nV, d_gradient.p, d_minusG.p, stream);
    cachedTrialValid = false;
    cachedDistValid = false; // (|p|_inf of the direction this call replaces)
    if (fastPath()) {
        // ONE synchronisation per Newton iteration.  Behind factorisation + sweeps, on the same stream and without the host in between: |p|_inf
        // (convergence test of the next pass, Optimizer.cpp:1869-1879), the inversion step filter (:1887), E at the iterate (:2681), then the
        // first trial of the line search -- step size decided on the device from the filter's result, the step, its inversion flag
        // (:2710-2717), E at the trial point (:2757).  The pivot flag of the factorisation arrives with them.  The host then only decides:
        // bad pivot -> back to the iterate and the diagonal fallback; trial inverted or uphill -> back to the iterate and the general loop.
        Tic t(timers[3], stream); // (its synchronisation is the one)
        const size_t bytes = 3 * (size_t)mesh.nV * sizeof(double);
        if (lin.factorizeSolve(rhs, d_searchDir.p, /*wait=*/false, signInSolver)) {
            // ten launches (fifteen before round 4: the resets, the copy + step-size + step and the two read-backs are one launch each now)
            launch_iter_reset(d_scalar.p, d_flag.p, stream); // (zeroes the slot of |p|_inf with the others: no enqueueDirNorm(), whose fill would be one launch more)
            launch_max_abs(3 * mesh.nV, d_searchDir.p, slot(S_DIR_NORM), stream);
            if (mesh.needElemInvSafeGuard()) launch_inversion_step(view(), d_searchDir.p, 0.2, 1.0, slot(S_STEP_FILTER), stream); // (the trial step starts at 1)
            enqueueElasticEnergy(true, slot(S_E_ITERATE));
            launch_trial_step_fused(3 * mesh.nV, mesh.d_x.p, d_x0.p, d_searchDir.p, slot(S_STEP_FILTER), mesh.needElemInvSafeGuard(), slot(S_TRIAL_ALPHA), stream);
            if (mesh.needElemInvSafeGuard()) launch_check_inversion(view(), d_flag.p, stream);
            enqueueElasticEnergy(true, slot(S_E_TRIAL));
            launch_publish2(d_flag.p, h_flag.dev, 1, slot(S_E_ITERATE), slotMapped(S_E_ITERATE), slotSpan(S_E_ITERATE, S_TRIAL_ALPHA), stream); // the inversion flag + the scalars
            // the ONE synchronisation waits for the read-back, not for the stream: behind it runs the next pass's assembly at the trial point, enqueued ahead
            if (!evTail) HIP_CHECK(hipEventCreateWithFlags(&evTail, hipEventDisableTiming));
            HIP_CHECK(hipEventRecord(evTail, stream));
            speculativeAssembly();
            HIP_CHECK(hipEventSynchronize(evTail));
            t.nosync = specAsmValid;
            if (lin.lastPivotsOk()) {
                cachedE0 = published(S_E_ITERATE);
                cachedTrialE = published(S_E_TRIAL);
                cachedFilter = published(S_STEP_FILTER);
                cachedDist = published(S_DIR_NORM);
                cachedAlpha = published(S_TRIAL_ALPHA);
                cachedTrialInverted = mesh.needElemInvSafeGuard() && h_flag.p[0] != 0;
                cachedDistValid = cachedE0Valid = cachedTrialValid = true;
                return;
            }
            HIP_CHECK(hipMemcpyAsync(mesh.d_x.p, d_x0.p, bytes, hipMemcpyDeviceToDevice, stream)); // the step was taken along garbage
            specAsmValid = false;
            t.nosync = false;
        }
        ok = false;
    }
    else {
        // the right-hand side is known before the factorisation starts: the forward sweep of each level runs beside the pivot chain of
        // the levels above (MfNumeric::factorizeSolve); this bucket then holds factorisation + both sweeps
        Tic t(timers[3], stream);
        if (worldSize == 1) {
            // one process: nothing waits inside the solver; |p|_inf for the convergence test of the next pass (Optimizer.cpp:1869-1879) is enqueued behind
            // the sweeps and the pivot flag comes back with it -- one synchronisation (round 6; two before, and a third at the head of the next pass)
            ok = lin.factorizeSolve(rhs, d_searchDir.p, /*wait=*/false, signInSolver);
            if (ok) {
                chamberGasCorrect(elasticCoef(), projDBC, d_searchDir.p); // (enqueued behind the sweeps; a bad pivot ends in the diagonal fallback below, which ignores the rank-k term)
                enqueueDirNorm();
                publish(S_DIR_NORM);
                HIP_CHECK(hipStreamSynchronize(stream));
                ok = lin.lastPivotsOk();
                if (ok) {
                    cachedDist = published(S_DIR_NORM);
                    cachedDistValid = true;
                }
            }
        }
        else ok = lin.factorizeSolve(rhs, d_searchDir.p, /*wait=*/true, signInSolver);
    }
    Tic t(timers[4], stream);
    if (!ok) {
        if (signInSolver) launch_negate(3 * mesh.nV, d_gradient.p, d_minusG.p, stream);
        completeMatrix(); // (owner-computes sharding: the diagonal of the rows other ranks hold)
        lin.precondition_diag(d_minusG.p, d_searchDir.p); // Optimizer.cpp:2331-2348
    }
    if (fastPath()) {
        // everything the host needs next, behind the solve on the same stream, read back with ONE synchronisation (the Tic's): |p|_inf
        // (convergence test of the next pass, Optimizer.cpp:1869-1879), the inversion step filter (:1887) and E at the current iterate
        // (line search entry, :2681)
        enqueueDirNorm();
        launch_fill(slot(S_STEP_FILTER), 1, 1e20, stream);
        if (mesh.needElemInvSafeGuard()) launch_inversion_step(view(), d_searchDir.p, 0.2, 1.0, slot(S_STEP_FILTER), stream); // (the trial step starts at 1)
        enqueueElasticEnergy(true, slot(S_E_ITERATE));
        publish(S_E_ITERATE, slotSpan(S_E_ITERATE, S_DIR_NORM));
        HIP_CHECK(hipStreamSynchronize(stream));
        cachedE0 = published(S_E_ITERATE);
        cachedFilter = published(S_STEP_FILTER);
        cachedDist = published(S_DIR_NORM);
        cachedDistValid = cachedE0Valid = true;
    }
    else {
        // the barrier Hessian's deferred "pair outside the pattern" flag has arrived with the solve's synchronisation; |p|_inf as above where it has not
        // come back yet (several processes, or the diagonal fallback just replaced the direction)
        if (!cachedDistValid) {
            enqueueDirNorm();
            publish(S_DIR_NORM);
            HIP_CHECK(hipStreamSynchronize(stream));
            cachedDist = published(S_DIR_NORM);
            cachedDistValid = true;
        }
        if (selfCollision) contact->takeHessianError();
    }
}

bool HipOptimizer::fastPath() const
{
    // (the iterative solver synchronises inside its solve and may end in the diagonal fallback: the general branch of computeSearchDir)
    // (a gas chamber puts k further solves and the rank-k correction behind the solve: the general branch too)
    return worldSize == 1 && !ipOn() && nbcGroups.empty() && !(dampingStiff > 0.0) && !(rhoDBC && !tpIds.empty()) && lin.solverType != 2 && !mesh.chamber.nGas();
}

void HipOptimizer::resolveEventTimers()
{
    if (!evAsmPending) return;
    HIP_CHECK(hipEventSynchronize(evAsm1));
    float ms = 0.0f;
    HIP_CHECK(hipEventElapsedTime(&ms, evAsm0, evAsm1));
    timers[0] += 1.0e-3 * (double)ms * evAsmWeight;
    evAsmPending = false;
}

// x = x0 + stepSize p from d_x0, stepSize halved while an element is inverted there, then, with contact, while the surface intersects itself or an obstacle
// (AnimScripter.cpp:2172-2180; Optimizer.cpp:1117-1215)
void HipOptimizer::stepFeasible(double& stepSize)
{
    stepForward(d_x0.p, stepSize);
    while (!checkInversion()) {
        stepSize /= 2.0;
        stepForward(d_x0.p, stepSize);
    }
    if (ipOn())
        while (anyIntersection()) {
            stepSize /= 2.0;
            stepForward(d_x0.p, stepSize);
        }
    // the shells' strain limit: the feasible set is convex and d_x0 lies inside it (beginTimestep), so halving ends, and a step shortened further for
    // another reason stays feasible.  What a scripted Dirichlet move loses here the augmented-Lagrangian solve takes up (completedStep < 1).
    // The rubber membrane likewise: d_x0 has no degenerate rubber triangle (beginTimestep), and a move that flattens one is halved away from it.
    while (stepSize > 0.0 && !(shellLimitFeasible() && shellRubberFeasible())) {
        stepSize /= 2.0;
        stepForward(d_x0.p, stepSize);
        if (ipOn())
            while (anyIntersection()) {
                stepSize /= 2.0;
                stepForward(d_x0.p, stepSize);
            }
    }
}

void HipOptimizer::lineSearch(double& stepSize)
{
    const size_t bytes = 3 * (size_t)mesh.nV * sizeof(double);
    if (cachedTrialValid && fastPath()) {
        // the first trial came back with the solve (computeSearchDir): d_x0 holds the iterate, x the trial point
        cachedTrialValid = cachedE0Valid = false;
        lastEnergyVal = cachedE0; // Optimizer.cpp:2681
        // (a +infinity trial energy -- a rod node folded flat, rod_kernels.h -- is greater than every finite one: rejected here, in the branch below and in
        // the halving loop, which backtracks it like any increase.  The rod kernels return +infinity, never NaN, which `!(NaN > E)` would accept.)
        if (!cachedTrialInverted && !(cachedTrialE > lastEnergyVal)) {
            lastEnergyVal = cachedTrialE;
            return;
        }
        HIP_CHECK(hipMemcpyAsync(mesh.d_x.p, d_x0.p, bytes, hipMemcpyDeviceToDevice, stream)); // back to the iterate: the general loop redoes the step
        specAsmValid = false;
    }
    else if (cachedE0Valid && fastPath()) {
        // E at the iterate came back with the solve; the trial step, its inversion flag and E at the trial point are enqueued together
        // and read with one synchronisation.  Anything but "not inverted and E decreased" falls through to the general loop below.
        cachedE0Valid = false;
        lastEnergyVal = cachedE0; // Optimizer.cpp:2681
        bool done = false;
        double testingE = 0.0;
        {
            Tic t(timers[5], stream);
            HIP_CHECK(hipMemcpyAsync(d_x0.p, mesh.d_x.p, bytes, hipMemcpyDeviceToDevice, stream));
            stepForward(d_x0.p, stepSize);
            int inverted = 0;
            if (mesh.needElemInvSafeGuard()) {
                d_flag.zero(stream);
                launch_check_inversion(view(), d_flag.p, stream);
                launch_publish(d_flag.p, h_flag.dev, 1, stream);
            }
            enqueueElasticEnergy(true, slot(S_E_ITERATE));
            publish(S_E_ITERATE);
            HIP_CHECK(hipStreamSynchronize(stream));
            if (mesh.needElemInvSafeGuard()) inverted = h_flag.p[0];
            testingE = published(S_E_ITERATE);
            done = !inverted && !(testingE > lastEnergyVal);
        }
        if (done) {
            lastEnergyVal = testingE;
            return;
        }
        HIP_CHECK(hipMemcpyAsync(mesh.d_x.p, d_x0.p, bytes, hipMemcpyDeviceToDevice, stream)); // back to the iterate: the general loop redoes the step
    }
    {
        Tic t(timers[9], stream);
        lastEnergyVal = computeEnergyVal(); // Optimizer.cpp:2681
    }
    {
        Tic t(timers[5], stream);
        HIP_CHECK(hipMemcpyAsync(d_x0.p, mesh.d_x.p, bytes, hipMemcpyDeviceToDevice, stream));
        stepForward(d_x0.p, stepSize);
        // (not stepFeasible(): a step size halved down to zero ends this loop with the positions at the last non-zero step, not back at d_x0)
        while (!checkInversion()) { // Optimizer.cpp:2710-2717
            stepSize /= 2.0;
            if (stepSize == 0.0) break;
            stepForward(d_x0.p, stepSize);
        }
        if (ipOn())
            while (anyIntersection()) { // Optimizer.cpp:2719-2736
                stepSize /= 2.0;
                stepForward(d_x0.p, stepSize);
            }
    }
    computeConstraintSets();
    double testingE;
    {
        Tic t(timers[9], stream);
        testingE = computeEnergyVal();
    }
    const double LFStepSize = stepSize;
    while (testingE > lastEnergyVal && stepSize > 0.0) { // Optimizer.cpp:2761-2797 (+infinity > finite: an infinite trial energy is halved away too)
        stepSize /= 2.0;
        if (stepSize == 0.0) break;
        {
            Tic t(timers[5], stream);
            stepForward(d_x0.p, stepSize);
        }
        computeConstraintSets();
        Tic t(timers[9], stream);
        testingE = computeEnergyVal();
    }
    if (stepSize < LFStepSize && ipOn()) { // Optimizer.cpp:2799-2811
        bool needRecomputeCS = false;
        while (anyIntersection()) {
            stepSize /= 2.0;
            stepForward(d_x0.p, stepSize);
            needRecomputeCS = true;
        }
        if (needRecomputeCS) computeConstraintSets(); // lastEnergyVal keeps the pre-halving value, as in the reference
    }
    lastEnergyVal = testingE;
}

void HipOptimizer::precompute()
{
    specAsmValid = false;
    // Optimizer.cpp:457-507
    if (!initialised) throw StateError("opt_precompute before opt_init");
    // Optimizer.cpp:258-263: the reference ends its process on an intersecting start (every line search after it would halve forever)
    if (anyIntersection()) throw StateError("intersection detected in initial configuration");
    {
        Tic t(timers[1], stream);
        lin.set_pattern(mesh, 0, nullptr);
        contactPattern = ContactPattern();
    }
    computeConstraintSets();
    computeDampingMtr(); // computePrecondMtr(..., updateDamping): Optimizer.cpp:470, 3598-3612
    {
        Tic t(timers[0], stream);
        computePrecondMtr(true, false); // re-patterns + analyses when contact pairs are already active
    }
    if (!lin.analyzed()) {
        Tic t(timers[2], stream);
        lin.analyze_pattern(&mesh);
    }
    lastEnergyVal = computeEnergyVal();
}

void HipOptimizer::beginTimestep()
{
    specAsmValid = false;
    if (!initialised) throw StateError("opt_begin_timestep before opt_init");
    if (!lin.analyzed()) throw StateError("opt_begin_timestep before opt_precompute");
    Tic t(timers[11], stream);
    refreshAeroLagged(); // normals, areas and centroids of the aerodynamic triangles: from the positions this step starts from, before any scripted move (aero_kernels.h)
    refreshChamberRef(); // r_c of the pressure chambers follows the body: from the positions this step starts from, fixed until the next step (chamber_kernels.h)
    // The contact-free twist (BASELINE configs[1]; round 6): everything the set-up of a time step asks the device -- inverted before the motion? the filter's bound
    // on the scripted step, the step, inverted after it? the energy there -- is enqueued as ONE batch and read back with one synchronisation (seven before: each
    // question waited for its answer).  Any answer but the usual one ("no", "no") falls back to the general sequence below from the state it left off.
    // (a strain limit or a rubber membrane takes the general sequence: its scripted step is shortened by stepFeasible)
    const bool batched = BEGIN_BATCHED && fastPath() && nHandles && dbcGroups.empty() && !selfCollision && colliders.empty() && !(warmStart >= 1 && warmStart <= 5)
        && !mesh.shell.nLimited() && !mesh.shell.nRubber();
    // With a strain limit the stepper never accepts a state with a stretch at or over it, so a time step may only start from a feasible one.  The energy the
    // stepper holds on the host tells: it is +infinity exactly then (or at the fold of a rod node, which the count below tells apart) -- no device query on
    // the usual path.  Positions or a limit set from outside since then are asked for once.  Nothing has been changed yet when this throws.
    if (mesh.shell.nLimited() && (mesh.shell.limitUnchecked || !(lastEnergyVal < INFINITY))) requireShellLimitFeasible();
    if (mesh.shell.nRubber() && (mesh.shell.rubberUnchecked || !(lastEnergyVal < INFINITY))) requireShellRubberFeasible(); // the same for a degenerate rubber triangle
    if (!rounds.empty()) requireRoundsFeasible(); // a start state on or inside a round collider is refused; nothing has been changed yet
    if (batched) {
        const bool guard = mesh.needElemInvSafeGuard(); // Optimizer.cpp:252, 517: only under getNeedElemInvSafeGuard()
        d_flag.zero(stream);
        if (guard) launch_check_inversion(view(), d_flag.p, stream);
        d_searchDir.zero(stream);
        stepStartTime = stepEndTime; // AnimScripter.cpp:1406-1407
        stepEndTime += dt;
        setDBCVertices();
        launch_twist_dir(nHandles, d_handleIds.p, d_handleAng.p, rotCenter[1], rotCenter[2], mesh.d_x.p, d_searchDir.p, stream);
        buildTargetPositions(/*deferTolerance=*/true);
        launch_fill(slot(S_STEP_FILTER), 1, 1e20, stream);
        if (guard) launch_inversion_step(view(), d_searchDir.p, 0.2, 1.0, slot(S_STEP_FILTER), stream); // filterStepSize(p, 1.0) ...
        launch_trial_step_fused(3 * mesh.nV, mesh.d_x.p, d_x0.p, d_searchDir.p, slot(S_STEP_FILTER), guard, slot(S_TRIAL_ALPHA), stream); // ... applied by its rule; x0 = x, x += step p
        if (guard) launch_check_inversion(view(), d_flag.p + 1, stream);
        enqueueElasticEnergy(true, slot(S_E_ITERATE)); // computeEnergyVal() of this configuration: elasticity + inertia
        launch_publish2(d_flag.p, h_flag.dev, 2, slot(S_E_ITERATE), slotMapped(S_E_ITERATE), slotSpan(S_E_ITERATE, S_TRIAL_ALPHA), stream);
        HIP_CHECK(hipStreamSynchronize(stream));
        if (h_flag.p[0]) throw StateError("element inversion before scripted motion (Optimizer.cpp:517-522)");
        finishTolerance();
        double stepSize = published(S_TRIAL_ALPHA);
        bool energyKnown = true;
        if (h_flag.p[1]) { // inverted behind the filtered step: the halving loop (AnimScripter.cpp:2172-2180) from here
            energyKnown = false;
            stepSize /= 2.0;
            stepFeasible(stepSize);
        }
        if (stepSize < 1.0) dbcIncomplete++;
        completedStep = stepSize;
        d_searchDir.zero(stream);
        initSubProblem();
        lastEnergyVal = energyKnown ? published(S_E_ITERATE) : computeEnergyVal(); // Optimizer.cpp:1609
        k = 0;
        return;
    }
    if (!checkInversion()) throw StateError("element inversion before scripted motion (Optimizer.cpp:517-522)");
    d_searchDir.zero(stream);
    stepStartTime = stepEndTime; // AnimScripter.cpp:1406-1407
    stepEndTime += dt;
    setDBCVertices();
    // stepAnimScript, AST_TWIST (AnimScripter.cpp:1674-1684, 2140-2215)
    if (nHandles) launch_twist_dir(nHandles, d_handleIds.p, d_handleAng.p, rotCenter[1], rotCenter[2], mesh.d_x.p, d_searchDir.p, stream);
    const bool groupMotion = dbcGroupMotion(); // AST_NULL: Dirichlet groups / scripted components (:1413-1462)
    buildTargetPositions();
    completedStep = 1.0;
    if (nHandles || groupMotion) {
        double stepSize = filterStepSize(d_searchDir.p, 1.0);
        if (selfCollision) // CCD of the scripted motion with slackness 0.5 (AnimScripter.cpp:2158-2171)
            stepSize = fullCcd(0.5, stepSize);
        HIP_CHECK(hipMemcpyAsync(d_x0.p, mesh.d_x.p, 3 * (size_t)mesh.nV * sizeof(double), hipMemcpyDeviceToDevice, stream));
        stepFeasible(stepSize);
        if (stepSize < 1.0) dbcIncomplete++; // the penalty solve of newtonIter() takes the nodes the rest of the way
        completedStep = stepSize; // AnimScripter::getCompletedStepSize
        d_searchDir.zero(stream); // initX(0), Optimizer.cpp:930-934
    }
    if (warmStart >= 1 && warmStart <= 5) {
        // initX options 1-4 (Optimizer.cpp:936-1080): explicit Euler / xHat / symplectic Euler / uniformly accelerated motion as the
        // first iterate, then the feasibility filters of a Newton step with "always full CCD" (:1117-1215)
        if (warmStart == 5) {
            // option 5 (:1082-1110), "Jacobi": -g_i / H_ii with the gradient of the projected and the matrix of the UNprojected Dirichlet rows,
            // zero on every Dirichlet node; sets, kappa and dHat are whatever the previous time step left
            computeGradient(true);
            computePrecondMtr(false, false);
            launch_negate(3 * mesh.nV, d_gradient.p, d_minusG.p, stream);
            completeMatrix();
            lin.precondition_diag(d_minusG.p, d_searchDir.p);
            launch_clear_projected(mesh.nV, mesh.d_dbc.p, 1, d_searchDir.p, stream); // isDBCVertex: ZERO and NONZERO alike
        }
        else {
        static const double CG[2][5] = { { 0, 0, 1, 1, 1 }, { 0, 0, 0.5, 0.5, 0.5 } }, CE[2][5] = { { 0, 0, 0, 1, 0.5 }, { 0, 0, 0, 2, 1 } };
        const double cg = CG[timeIntegration][warmStart], ce = CE[timeIntegration][warmStart];
        const double g3[3] = { cg * (dtSq * gravity[0]), cg * (dtSq * gravity[1]), cg * (dtSq * gravity[2]) };
        launch_warm_dir(mesh.nV, mesh.d_dbc.p, d_vel.p, d_dxElastic.p, dt, g3, ce, d_searchDir.p, stream);
        }
        double stepSize = filterStepSize(d_searchDir.p, 1.0);
        if (ipOn()) {
            for (auto* h : colliders) stepSize = h->stepBound(contact->nSVI, contact->d_SVI.p, mesh.d_x.p, mesh.d_dbc.p, d_searchDir.p, 0.9, stepSize);
            if (selfCollision) stepSize = fullCcd(0.8, stepSize);
        }
        HIP_CHECK(hipMemcpyAsync(d_x0.p, mesh.d_x.p, 3 * (size_t)mesh.nV * sizeof(double), hipMemcpyDeviceToDevice, stream));
        stepFeasible(stepSize);
        warmStepSize = stepSize;
    }
    if (ipOn()) {
        // fullyImplicit_IP head (Optimizer.cpp:1534-1550, 2316-2322): dHat, constraint sets, kappa, empty close-pair list
        dHat = dHatEps * dHatEps * lenScale2();
        computeConstraintSets();
        // tuning[0] when the script gives one, bounded from above; 0 -> suggestKappa (Optimizer.cpp:1540-1547)
        kappa = kappaConfig > 0.0 ? std::min(kappaConfig, 100 * kappaFloor()) : kappaFloor();
        initKappa();
        closeHS.clear();
        closeHSVal.clear();
        closeID.clear();
        closeVal.clear();
        // friction: lagged sets reset, eps_v^2 h^2 (Optimizer.cpp:1525-1533, 286-304), then lagged at x^n (:1553-1600)
        if (contact) contact->frictionLagClear();
        for (auto* h : colliders) h->lagClear();
        fricDHat0 = epsV * epsV * (ctorDt * ctorDt) * lenScale2(); // Optimizer.cpp:290-303: set once in the constructor, see (ctorDt * ctorDt)
        fricDHatTarget = epsVTarget > 0.0 ? epsVTarget * epsVTarget * (ctorDt * ctorDt) * lenScale2() : fricDHat0;
        fricDHat = solveFric() ? fricDHat0 : -1.0;
        fricIterI = 0;
        updateFrictionLag();
    }
    initSubProblem();
    lastEnergyVal = computeEnergyVal(); // Optimizer.cpp:1609
    k = 0;
}

void HipOptimizer::initSubProblem()
{
    specAsmValid = false;
    projDBC = true;
    rhoDBC = 0.0;
    lastMove = completedStep;
}

// targetPos / dist2Tol of stepAnimScript (AnimScripter.cpp:2150-2157).  Every scripted node is a Dirichlet node here (twist
// handles, Dirichlet groups, scripted components), so the keys are the Dirichlet nodes.  Per time step, a few KB.
void HipOptimizer::buildTargetPositions(bool deferTolerance)
{
    tpIds.clear();
    for (int v = 0; v < mesh.nV; ++v)
        if (mesh.dbcType[v] != 0) tpIds.push_back(v);
    dist2Tol = 0.0;
    tolPending = false;
    if (tpIds.empty()) return;
    const int n = (int)tpIds.size();
    if (tpIds != tpIdsOnDevice) { // (the same nodes step after step unless a Dirichlet group starts or ends)
        d_tpIds.uploadGrow(tpIds, stream);
        tpIdsOnDevice = tpIds;
    }
    d_tpPos.ensure(3 * (size_t)n);
    d_tpLam.ensure(3 * (size_t)n); // (cleared by the kernel below, which walks the same 3 n entries)
    // targets x + p formed on the device (round 6: x and p of the scripted nodes used to travel to the host, their sum back); the host only needs p for the tolerance,
    // summed there in index order as before.  deferTolerance: p goes to pinned host memory and finishTolerance() sums it behind the caller's next synchronisation
    // (through a device buffer and ONE copy into pinned memory: thousands of 8-byte stores of a kernel into mapped host memory are thousands of bus transactions --
    // 7 ms for the Dirichlet nodes of 4_rodsTwist when this was first written that way)
    if (h_tpStage.n < 3 * (size_t)n) h_tpStage.alloc(3 * (size_t)n + 3 * (size_t)n / 2 + 16);
    d_tpStage.ensure(3 * (size_t)n);
    launch_target_positions(n, d_tpIds.p, mesh.d_x.p, d_searchDir.p, d_tpPos.p, d_tpStage.p, d_tpLam.p, stream);
    HIP_CHECK(hipMemcpyAsync(h_tpStage.p, d_tpStage.p, 3 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream));
    tolPending = true;
    if (!deferTolerance) {
        HIP_CHECK(hipStreamSynchronize(stream));
        finishTolerance();
    }
}

void HipOptimizer::finishTolerance()
{
    if (!tolPending) return;
    tolPending = false;
    double sq = 0.0;
    for (size_t i = 0, m = 3 * tpIds.size(); i < m; ++i) sq += h_tpStage.p[i] * h_tpStage.p[i];
    dist2Tol = sq * 1.0e-6;
}

double HipOptimizer::computeCompletedStepSize()
{
    if (dist2Tol == 0.0 || tpIds.empty()) return completedStep = 1.0;
    launch_mdbc_reduce(mdbc(), mesh.d_x.p, 0.0, 1, slot(S_SCRATCH), stream);
    const double sqNorm = readScalar(S_SCRATCH);
    return completedStep = 1.0 - std::sqrt(sqNorm / (dist2Tol * 1.0e6));
}

// after postLineSearch (Optimizer.cpp:2168-2203)
void HipOptimizer::dirichletPenaltyUpdate()
{
    if (projDBC) {
        if (completedStep < 1.0 - 1.0e-3) { // setup penalty solve
            projDBC = false;
            rhoDBC = 1.0e6;
        }
        return;
    }
    const double completed = computeCompletedStepSize();
    if (completed > 1.0 - 1.0e-3) projDBC = true; // penalty solve finished
    else if (completed < lastMove && rhoDBC < 1.0e8) rhoDBC *= 2.0;
    else {
        enqueueDirNorm();
        if (readScalar(S_DIR_NORM) < CN_MBC) { // safeToPull
            if (completed < 0.99 && rhoDBC < 1.0e8) rhoDBC *= 2.0;
            else launch_mdbc_lambda(mdbc(), mesh.d_x.p, rhoDBC, stream); // updateLambda (AnimScripter.cpp:2339-2346)
        }
    }
}

bool HipOptimizer::newtonIter()
{
    // convergence test (Optimizer.cpp:1869-1879) looks at the search direction of the previous pass
    double distToOpt_PN;
    if (k && cachedDistValid) distToOpt_PN = cachedDist; // read back with the last solve
    else if (k) {
        enqueueDirNorm();
        distToOpt_PN = readScalar(S_DIR_NORM);
    }
    else distToOpt_PN = 0.0; // (the test needs k > 0: nothing to measure in the first pass of a time step)
    cachedDistValid = false;
    if (k && distToOpt_PN < targetGRes && completedStep > 1.0 - 1.0e-3) { // :1874-1879
        specAsmValid = false; // (the one assembly per time step that goes unused)
        Tic t(timers[12], stream);
        t.nosync = fastPath(); // (nobody on the host waits for this gradient: whoever reads it synchronises)
        computeGradient(projDBC); // the reference leaves the gradient of the converged state behind (:1861)
        return true;
    }
    innerIterAmt++;
    if (fastPath()) {
        // the assembly is timed with events: no host synchronisation between it and the factorisation
        if (!evAsm0) {
            HIP_CHECK(hipEventCreate(&evAsm0));
            HIP_CHECK(hipEventCreate(&evAsm1));
        }
        if (specAsmValid && projDBC && d_aSpec.n == lin.d_a.n && d_gradSpec.n == d_gradient.n) {
            // the assembly of exactly this state is already there (enqueued behind the last pass's trial, timed by its own events): swap it in
            std::swap(lin.d_a.p, d_aSpec.p);
            std::swap(d_gradient.p, d_gradSpec.p);
            matrixComplete = true;
        }
        else {
            resolveEventTimers();
            HIP_CHECK(hipEventRecord(evAsm0, stream));
            computePrecondMtr(projDBC, true);
            HIP_CHECK(hipEventRecord(evAsm1, stream));
            evAsmPending = true;
            evAsmWeight = 1; // (an assembly of its own: the first iteration of a time step, a rejected trial)
        }
        specAsmValid = false;
    }
    else {
        // gradient (:1861) and Hessian (:2327) come out of one fused element pass
        specAsmValid = false; // an assembly enqueued ahead by an earlier fast-path pass describes a state this branch has left behind
        Tic t(timers[0], stream);
        computePrecondMtr(projDBC, true);
    }
    cachedE0Valid = false;
    computeSearchDir();
    double alpha = 1.0;
    {
        Tic t(timers[13], stream);
        t.nosync = specAsmValid && cachedTrialValid; // nothing is enqueued in here on that path, and the stream carries the assembly enqueued ahead
        // (one process, self-contact, no half-spaces between the filter and the CCD: the three bounds come back with one synchronisation, HipContact::stepBounds)
        const bool batchedBounds = !cachedTrialValid && !cachedE0Valid && selfCollision && colliders.empty() && worldSize == 1;
        if (cachedTrialValid) alpha = cachedAlpha; // decided on the device by the same rule, the trial step is already taken with it
        else if (cachedE0Valid) { // Optimizer.cpp:1887 with the value the solve's batch brought back
            if (mesh.needElemInvSafeGuard() && cachedFilter > 0.0 && cachedFilter < alpha) alpha = cachedFilter;
        }
        else if (!batchedBounds)
        alpha = filterStepSize(d_searchDir.p, alpha); // Optimizer.cpp:1887
        for (auto* h : colliders) // slackness_a = 0.9 (:1886-1890)
            alpha = h->stepBound(contact->nSVI, contact->d_SVI.p, mesh.d_x.p, mesh.d_dbc.p, d_searchDir.p, 0.9, alpha);
        if (selfCollision) {
            // step-size pipeline of Optimizer.cpp:1884-2040: partial CCD over the candidates of the current
            // constraint set, CFL bound, full CCD only when the step leaves the CFL ball
            const double slackness_m = 0.8;
            double pMax;
            if (batchedBounds) {
                // inversion filter, partial CCD and surface speed in one batch: the filter's root stays on the device and bounds the CCD there
                const bool filter = mesh.needElemInvSafeGuard(); // Energy.cpp:567 needElemInvSafeGuard
                if (filter) {
                    launch_fill(slot(S_STEP_FILTER), 1, 1e20, stream);
                    launch_inversion_step(view(), d_searchDir.p, 0.2, alpha, slot(S_STEP_FILTER), stream);
                }
                contact->stepBounds(mesh.d_x.p, d_searchDir.p, slackness_m, alpha, filter ? slot(S_STEP_FILTER) : nullptr, &alpha, lastCCDPair, &pMax);
            }
            else {
                alpha = contact->ccdPartial(mesh.d_x.p, d_searchDir.p, slackness_m, alpha, lastCCDPair);
                pMax = contact->maxSurfaceSpeed(d_searchDir.p);
            }
            const double alpha_CFL = std::sqrt(dHat) / (pMax * 2.0);
            if ((!k && alpha > alpha_CFL) || alpha > 2.0 * alpha_CFL) {
                alpha = fullCcd(slackness_m, alpha);
                nFullCCD++;
                if (alpha < alpha_CFL) alpha = alpha_CFL;
            }
            else alpha = std::min(alpha, alpha_CFL);
        }
    }
    lastAlphaFeasible = alpha;
    lineSearch(alpha);
    lastStepSize = alpha;
    postLineSearch();
    dirichletPenaltyUpdate();
    ++k;
    return false;
}

void HipOptimizer::endTimestep()
{
    specAsmValid = false;
    Tic t(timers[11], stream);
    t.nosync = fastPath(); // (the update is one kernel on the stream; the next time step's batch synchronises)
    // the update writes x^t of the next step into the second array: what d_xPrev held, the positions this step started from, stays for the system report
    std::swap(d_xPrev.p, d_xStepStart.p);
    if (timeIntegration == 1)
        launch_nm_update(mesh.nV, mesh.d_dbc.p, mesh.d_x.p, d_xPrev.p, d_vel.p, d_acc.p, d_dxElastic.p, mesh.d_xTilde.p, dt, betaNM, gammaNM,
            gravity[0], gravity[1], gravity[2], stream);
    else
        launch_be_update(mesh.nV, mesh.d_dbc.p, mesh.d_x.p, d_xStepStart.p, d_xPrev.p, d_vel.p, d_acc.p, d_dxElastic.p, mesh.d_xTilde.p, dt, gravity[0],
            gravity[1], gravity[2], stream);
    // plastic flow at the end-of-step positions (plastic_kernels.h): before the lagged damping matrix, which is then the stiffness of the rest shape the
    // next step sees.  Nothing derived from A outlives it: specAsmValid is cleared above, the patch plan and the stress plan hold topology only.
    if (mesh.plastic.on()) plasticFlow(mesh.d_x.p, dt);
    if (mesh.shell.plastic.on()) shellPlasticFlow(mesh.d_x.p, dt); // (shell_plastic_kernels.h: the same place, for the same reason)
    computeDampingMtr(); // Optimizer.cpp:593-595
    globalIterNum++;
}

// ---- system report (Optimizer::computeSystemEnergy, Optimizer.cpp:3746-3778) ----------------------------------------------------
void HipOptimizer::setComponents(int nComp, const int* nodeEnd, const int* tetEnd_)
{
    if (!reportEndsValid(nComp, nodeEnd, mesh.nV) || !reportEndsValid(nComp, tetEnd_, mesh.nT))
        throw ArgError("set_components: the accumulated ends must be non-decreasing and end at the node / element count");
    compNodeEnd.assign(nodeEnd, nodeEnd + nComp);
    compTetEnd.assign(tetEnd_, tetEnd_ + nComp);
    reportPlanValid = false;
}

void HipOptimizer::ensureReportPlan()
{
    if (reportPlanValid) return;
    if (compNodeEnd.empty() || compNodeEnd.back() != mesh.nV || compTetEnd.back() != mesh.nT) { // no table (or one of another mesh): the whole mesh
        compNodeEnd.assign(1, mesh.nV);
        compTetEnd.assign(1, mesh.nT);
    }
    const int nComp = (int)compNodeEnd.size();
    std::vector<ReportSlice> slices;
    std::vector<int> nodeStart, tetStart;
    buildReportSlices(nComp, compNodeEnd.data(), 256, slices, nodeStart);
    nReportNodeSlices = (int)slices.size();
    buildReportSlices(nComp, compTetEnd.data(), 256, slices, tetStart);
    nReportSlices = (int)slices.size();
    static_assert(sizeof(ReportSlice) == 3 * sizeof(int), "the kernel reads the list as int triples");
    std::vector<int> flat(3 * slices.size() + 1);
    std::memcpy(flat.data(), slices.data(), slices.size() * sizeof(ReportSlice));
    d_reportSlices.upload(flat, stream);
    d_reportNodeStart.upload(nodeStart, stream);
    d_reportTetStart.upload(tetStart, stream);
    d_reportRec.alloc(7 * slices.size() + 1);
    h_report.alloc(7 * (size_t)nComp);
    HIP_CHECK(hipStreamSynchronize(stream)); // the staging vectors go out of scope
    reportPlanValid = true;
}

void HipOptimizer::systemReport(double* sysE, double* sysM, double* sysL)
{
    if (worldSize > 1) throw UnsupportedError("system report on a sharded context (multi-rank reports are not implemented)");
    ensureReportPlan();
    const int nComp = (int)compNodeEnd.size();
    launch_system_report(view(), d_xStepStart.p, d_reportSlices.p, nReportNodeSlices, nReportSlices, d_reportNodeStart.p, d_reportTetStart.p, nComp, dt,
        gravity, d_reportRec.p, h_report.dev, stream);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(stream));
    for (int c = 0; c < nComp; ++c) {
        const double* r = h_report.p + 7 * (size_t)c;
        if (sysE) sysE[c] = r[0];
        for (int i = 0; i < 3; ++i) {
            if (sysM) sysM[3 * (size_t)c + i] = r[1 + i];
            if (sysL) sysL[3 * (size_t)c + i] = r[4 + i];
        }
    }
}

int HipOptimizer::solveTimestep(int maxIter)
{
    beginTimestep();
    int it = 0;
    for (;;) {
        while (it < maxIter) {
            if (newtonIter()) break;
            ++it;
        }
        if (it >= maxIter || !nextSubproblem()) break; // friction lagging iterations (fricIterAmt)
    }
    endTimestep();
    return it;
}

} // namespace ipcgpu
