// extern "C" boundary of libipcgpu.so (include/ipcgpu.h).  No exception leaves this file.
#include "../../include/ipcgpu.h"
#include "hip_ipc.h"
#include "msh_io.h"
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>

using namespace ipcgpu;

namespace {
thread_local std::string g_err;

template <class Fn>
int guarded(Fn&& fn)
{
    try {
        return fn();
    }
    catch (const ArgError& e) {
        g_err = e.what();
        return IPCGPU_ERR_ARG;
    }
    catch (const StateError& e) {
        g_err = e.what();
        return IPCGPU_ERR_STATE;
    }
    catch (const UnsupportedError& e) {
        g_err = e.what();
        return IPCGPU_ERR_UNSUPPORTED;
    }
    catch (const HipError& e) {
        g_err = e.what();
        return IPCGPU_ERR_HIP;
    }
    catch (const std::exception& e) {
        g_err = e.what();
        return IPCGPU_ERR_HIP;
    }
    catch (...) {
        g_err = "unknown error";
        return IPCGPU_ERR_HIP;
    }
}

void need(bool cond, const char* what)
{
    if (!cond) throw StateError(what);
}
void needArg(bool cond, const char* what)
{
    if (!cond) throw ArgError(what);
}
HipMesh& M(ipcgpu_ctx* c)
{
    needArg(c != nullptr, "null context");
    need(c->mesh && c->mesh->nV > 0, "no mesh: call ipcgpu_set_mesh first");
    return *c->mesh;
}
HipLinSysSolver& L(ipcgpu_ctx* c)
{
    needArg(c != nullptr, "null context");
    return *c->lin;
}
HipOptimizer& O(ipcgpu_ctx* c)
{
    M(c);
    return *c->opt;
}
void bind(ipcgpu_ctx* c) { HIP_CHECK(hipSetDevice(c->device)); }
// Every entry point that changes what the next assembly depends on (positions, constraints, material, time step, ...) calls this first: the stepper
// may hold an assembly it enqueued ahead for the state it had (HipOptimizer::speculativeAssembly), and that one must not be swapped in afterwards.
void specChanged(ipcgpu_ctx* c)
{
    if (c && c->opt) c->opt->specAsmValid = false;
}
// After an owner-computes assembly on a sharded context (HipOptimizer::ownerMode) a[] holds this rank's rows only.  Entry points that consume the WHOLE
// matrix refuse to work on such a partial one instead of returning a rank's share silently; ipcgpu_opt_complete_matrix (a collective: never called
// implicitly) completes it.  ADVICE round 4.
void needWholeMatrix(ipcgpu_ctx* c)
{
    need(!(c->opt && c->opt->ownerMode() && !c->opt->matrixComplete),
        "the matrix holds this rank's rows only (owner-computes assembly): call ipcgpu_opt_complete_matrix on every rank first");
}
// contact-pair lists shard with the elements (ipcgpu_ctx_set_shard): the handler is created lazily, so both places call this
void applyContactShard(ipcgpu_ctx* c)
{
    if (!c->contact) return;
    c->contact->shardRank = c->rank;
    c->contact->shardWorld = c->worldSize;
    HipOptimizer* o = c->opt.get();
    c->contact->shardReduce = [o](double* d, long long n) { o->reduceSum(d, n); };
}

// column-major nV x 3 (host) <-> xyz interleaved (device)
void uploadColMajor(ipcgpu_ctx* c, const double* Vcm, DevBuf<double>& dst)
{
    const int nV = c->mesh->nV;
    std::vector<double> aos(3 * (size_t)nV);
    for (int v = 0; v < nV; ++v)
        for (int k = 0; k < 3; ++k) aos[3 * (size_t)v + k] = Vcm[v + (size_t)nV * k];
    dst.upload(aos, c->stream);
    HIP_CHECK(hipStreamSynchronize(c->stream));
}
void downloadColMajor(ipcgpu_ctx* c, const DevBuf<double>& src, double* Vcm)
{
    const int nV = c->mesh->nV;
    std::vector<double> aos(3 * (size_t)nV);
    src.download(aos.data(), aos.size(), c->stream);
    for (int v = 0; v < nV; ++v)
        for (int k = 0; k < 3; ++k) Vcm[v + (size_t)nV * k] = aos[3 * (size_t)v + k];
}

// ---- what the entry points of the codimensional energies (shells, their strain limit, rods) share -------------------------------------------
// `which` is a mask of HipOptimizer::CODIM_*: ipcgpu_shell_* mean the shell with its rubber membrane, its woven cloth and its limit, ipcgpu_shell_limit_* the limit alone,
// ipcgpu_shell_rubber_* the rubber membrane alone, ipcgpu_shell_weave_* the woven cloth alone, ipcgpu_rod_* the rod, ipcgpu_attach_* the attachments, ipcgpu_chamber_* the pressure chambers, ipcgpu_aero_* wind and air drag, ipcgpu_fiber_* the fibres of the tetrahedra.
constexpr unsigned SHELL_AND_LIMIT = HipOptimizer::CODIM_SHELL | HipOptimizer::CODIM_SHELL_RUBBER | HipOptimizer::CODIM_SHELL_WEAVE | HipOptimizer::CODIM_SHELL_LIMIT, LIMIT_ALONE = HipOptimizer::CODIM_SHELL_LIMIT,
                   RUBBER_ALONE = HipOptimizer::CODIM_SHELL_RUBBER, WEAVE_ALONE = HipOptimizer::CODIM_SHELL_WEAVE, ROD = HipOptimizer::CODIM_ROD,
                   ATTACH = HipOptimizer::CODIM_ATTACH, CHAMBER = HipOptimizer::CODIM_CHAMBER, AERO = HipOptimizer::CODIM_AERO, FIBER = HipOptimizer::CODIM_FIBER;
const char* const SHELL_MISS = "the pattern lacks a block of the shell Hessian: build it after ipcgpu_set_shell";
const char* const ROD_MISS = "the pattern lacks a block of the rod Hessian: build it after ipcgpu_set_rod";
const char* const ATTACH_MISS = "the pattern lacks a block of the attachment Hessian: build it after ipcgpu_set_attachments";
const char* const CHAMBER_MISS = "the pattern lacks a block of the chamber Hessian: build it after ipcgpu_set_chambers";
const char* const AERO_MISS = "the pattern lacks a block of the air-drag Hessian: build it after ipcgpu_set_aero";
const char* const FIBER_MISS = "the pattern lacks a block of the fibre Hessian: it does not hold the node pairs of the tetrahedra";
// What an entry point returns early on: no triangle, no limited triangle, no rubber triangle, no woven triangle, no segment, no attachment, no chamber triangle, no aerodynamic triangle, no fibred element.
int codimCount(const HipMesh& m, unsigned which)
{
    return (which & HipOptimizer::CODIM_SHELL) ? m.shell.nTri()
        : (which & HipOptimizer::CODIM_SHELL_LIMIT) ? m.shell.nLimited()
        : (which & HipOptimizer::CODIM_SHELL_RUBBER) ? m.shell.nRubber()
        : (which & HipOptimizer::CODIM_SHELL_WEAVE) ? m.shell.nWoven()
        : (which & HipOptimizer::CODIM_ROD)         ? m.rod.nSeg()
        : (which & HipOptimizer::CODIM_ATTACH)      ? m.attach.n()
        : (which & HipOptimizer::CODIM_CHAMBER)     ? m.chamber.nTri()
        : (which & HipOptimizer::CODIM_AERO)        ? m.aero.nTri()
                                                    : m.fiber.n();
}
int codimEnergy(ipcgpu_ctx* c, unsigned which, double coef, double* E)
{
    HipOptimizer& o = O(c);
    bind(c);
    needArg(E != nullptr, "null argument");
    // (ipcgpu_shell_limit_energy alone asks for this: its +infinity must keep its sign)
    needArg(which != HipOptimizer::CODIM_SHELL_LIMIT || coef > 0.0, "the coefficient of the strain-limit energy must be positive");
    needArg(which != HipOptimizer::CODIM_SHELL_RUBBER || coef > 0.0, "the coefficient of the rubber-membrane energy must be positive");
    need(o.initialised, "call ipcgpu_opt_init first");
    *E = 0.0;
    if (!codimCount(*c->mesh, which)) return IPCGPU_OK;
    o.codimEnergyAdd(c->mesh->d_x.p, coef, o.slot(S_SCRATCH), /*accumulate=*/false, which);
    *E = o.readScalar(S_SCRATCH);
    return IPCGPU_OK;
}
int codimGradientAdd(ipcgpu_ctx* c, unsigned which, double coef, int projectDBC, double* g)
{
    HipOptimizer& o = O(c);
    bind(c);
    needArg(g != nullptr, "null argument");
    if (!codimCount(*c->mesh, which)) return IPCGPU_OK;
    DevBuf<double> dg;
    dg.upload(g, 3 * (size_t)c->mesh->nV, c->stream);
    o.codimAssembleAdd(coef, projectDBC != 0, dg.p, nullptr, nullptr, which);
    HIP_CHECK(hipGetLastError());
    dg.download(g, 3 * (size_t)c->mesh->nV, c->stream);
    return IPCGPU_OK;
}
int codimHessianAdd(ipcgpu_ctx* c, unsigned which, double coef, int projectDBC, const char* missMessage)
{
    HipOptimizer& o = O(c);
    bind(c);
    if (!codimCount(*c->mesh, which)) return IPCGPU_OK;
    need(!c->lin->rowBase.empty(), "call ipcgpu_linsys_set_pattern first");
    o.codimAssembleAdd(coef, projectDBC != 0, nullptr, c->lin->d_a.p, nullptr, which);
    HIP_CHECK(hipGetLastError());
    int err = 0;
    c->mesh->d_codimErr.download(&err, 1, c->stream);
    if (err) {
        c->mesh->d_codimErr.zero(c->stream);
        HIP_CHECK(hipStreamSynchronize(c->stream));
        throw StateError(missMessage);
    }
    return IPCGPU_OK;
}
// ipcgpu_set_shell / ipcgpu_set_rod / ipcgpu_set_attachments / ipcgpu_set_chambers / ipcgpu_set_aero (which: CODIM_SHELL / CODIM_ROD / CODIM_ATTACH /
// CODIM_CHAMBER / CODIM_AERO): n elements, set(mesh) the call that differs
template <class Set>
int setCodimBody(ipcgpu_ctx* c, unsigned which, bool argsOk, int n, Set&& set)
{
    specChanged(c);
    return guarded([&] {
        const bool aero = which == HipOptimizer::CODIM_AERO;
        const std::string what = which == HipOptimizer::CODIM_SHELL ? "shell" : which == HipOptimizer::CODIM_ROD ? "rod" : which == HipOptimizer::CODIM_ATTACH ? "attachment" : aero ? "aerodynamic surface" : "chamber";
        const bool plural = which == HipOptimizer::CODIM_ATTACH || which == HipOptimizer::CODIM_CHAMBER;
        HipMesh& m = M(c);
        bind(c);
        needArg(argsOk, ("bad " + what + " arguments").c_str());
        if (n == 0 && codimCount(m, which) == 0) return IPCGPU_OK; // nothing to remove
        if (c->worldSize > 1) throw UnsupportedError(what + "s on a sharded context");
        need(!c->opt->initialised, ("ipcgpu_set_" + (aero ? std::string("aero") : what) + (plural ? "s" : "") + " must come before ipcgpu_opt_init (masses, dHat and kappa derive from it) and before the pattern is built").c_str());
        set(m);
        if (!c->lin->rowBase.empty()) c->lin->set_pattern(m, 0, nullptr); // (a pattern built before this call lacks the new body's node pairs)
        return IPCGPU_OK;
    });
}
} // namespace

extern "C" {

const char* ipcgpu_last_error(void) { return g_err.c_str(); }
int ipcgpu_version(void) { return 100; }

int ipcgpu_ctx_create(int device_id, ipcgpu_ctx** out)
{
    return guarded([&] {
        needArg(out != nullptr, "null out pointer");
        int count = 0;
        hipError_t e = hipGetDeviceCount(&count);
        if (e != hipSuccess || count <= 0) throw HipError("no HIP device visible (this library has no CPU fallback)");
        needArg(device_id >= 0 && device_id < count, "device id out of range");
        HIP_CHECK(hipSetDevice(device_id));
        auto* c = new ipcgpu_ctx;
        c->device = device_id;
        {
            // the context's stream carries the dependent chain of every Newton iteration (pivot steps of the top separators): highest priority, so that its
            // workgroups are placed ahead of the bulk work the solver keeps on its own streams beside it (Schur passes, forward sweep)
            int lo = 0, hi = 0;
            HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
            HIP_CHECK(hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, hi));
        }
        c->mesh.reset(new HipMesh);
        c->lin.reset(new HipLinSysSolver(c->stream));
        c->opt.reset(new HipOptimizer(*c->mesh, *c->lin, c->stream));
        *out = c;
        return IPCGPU_OK;
    });
}
int ipcgpu_ctx_destroy(ipcgpu_ctx* c)
{
    return guarded([&] {
        if (!c) return IPCGPU_OK;
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        c->contact.reset();
        c->stress.reset();
        c->opt.reset();
        c->lin.reset();
        c->mesh.reset();
        (void)hipStreamDestroy(c->stream);
        delete c;
        return IPCGPU_OK;
    });
}
int ipcgpu_ctx_set_solver(ipcgpu_ctx* c, int type)
{
    specChanged(c);
    return guarded([&] {
        needArg(c && (type == IPCGPU_SOLVER_MULTIFRONTAL || type == IPCGPU_SOLVER_ROCSOLVER_CSRRF || type == IPCGPU_SOLVER_PCG), "unknown solver type"); // LinSysSolver.cpp:24-26
        if (type == IPCGPU_SOLVER_PCG && c->lin->solverWorld() > 1) {
            g_err = "the iterative solver is not sharded";
            return IPCGPU_ERR_UNSUPPORTED;
        }
        if (type == IPCGPU_SOLVER_PCG && c->mesh->chamber.nGas()) throw UnsupportedError("the iterative solver with a gas chamber (its operator lacks the rank-k term of the gas law)");
        if (type != c->lin->solverType) c->lin->invalidateAnalysis();
        c->lin->solverType = type;
        return IPCGPU_OK;
    });
}
int ipcgpu_ctx_set_shard(ipcgpu_ctx* c, int rank, int world)
{
    specChanged(c);
    return guarded([&] {
        needArg(c && world >= 1 && rank >= 0 && rank < world, "bad shard");
        if (world > 1 && c->mesh->shell.nTri()) throw UnsupportedError("shells on a sharded context");
        if (world > 1 && c->mesh->rod.nSeg()) throw UnsupportedError("rods on a sharded context");
        if (world > 1 && c->mesh->attach.n()) throw UnsupportedError("attachments on a sharded context");
        if (world > 1 && c->mesh->chamber.n()) throw UnsupportedError("chambers on a sharded context");
        if (world > 1 && c->mesh->aero.n()) throw UnsupportedError("aerodynamic surfaces on a sharded context");
        if (world > 1 && !c->opt->rounds.empty()) throw UnsupportedError("round colliders on a sharded context");
        if (world > 1 && c->mesh->plastic.on()) throw UnsupportedError("plasticity on a sharded context");
        if (world > 1 && c->mesh->shell.plastic.on()) throw UnsupportedError("shell plasticity on a sharded context");
        if (world > 1 && c->mesh->fiber.n()) throw UnsupportedError("fibres on a sharded context");
        c->rank = rank;
        c->worldSize = world;
        c->opt->rank = rank;
        c->opt->worldSize = world;
        applyContactShard(c);
        if (c->mesh->nT) {
            c->opt->tetBegin = (int)((long long)c->mesh->nT * rank / world);
            c->opt->tetEnd = (int)((long long)c->mesh->nT * (rank + 1) / world);
        }
        return IPCGPU_OK;
    });
}

int ipcgpu_set_mesh(ipcgpu_ctx* c, int nV, int nT, const double* Vr, const int* F, double YM, double PR, double rho)
{
    return guarded([&] {
        needArg(c && Vr && (F || nT == 0), "null argument");
        bind(c);
        c->mesh->computeFeatures(nV, nT, Vr, F, YM, PR, rho, c->stream);
        c->opt->tetBegin = (int)((long long)nT * c->rank / c->worldSize);
        c->opt->tetEnd = (int)((long long)nT * (c->rank + 1) / c->worldSize);
        c->opt->initialised = false;
        c->opt->compNodeEnd.clear(); // the component table belongs to the previous mesh: back to one component
        c->opt->compTetEnd.clear();
        c->opt->reportPlanValid = false;
        c->opt->selfCollision = false; // surface + contact state belong to the previous mesh
        c->opt->contact = nullptr;
        c->opt->planes.clear();
        c->opt->rounds.clear();
        c->opt->listColliders();
        c->contact.reset();
        c->stress.reset(); // the incidence list belongs to the previous mesh
        return IPCGPU_OK;
    });
}
int ipcgpu_set_component_material(ipcgpu_ctx* c, int nodeBegin, int nodeEnd, int tetBegin, int tetEnd, double rho, double YM, double PR)
{
    specChanged(c);
    return guarded([&] {
        HipMesh& m = M(c);
        bind(c);
        needArg(0 <= nodeBegin && nodeBegin <= nodeEnd && nodeEnd <= m.nV && 0 <= tetBegin && tetBegin <= tetEnd && tetEnd <= m.nT, "range out of bounds");
        needArg(rho > 0 && YM > 0 && PR > -1.0 && PR < 0.5, "bad material");
        m.setComponentMaterial(nodeBegin, nodeEnd, tetBegin, tetEnd, rho, YM, PR, c->stream);
        return IPCGPU_OK;
    });
}
struct ipcgpu_tetmesh {
    ipcgpu::TetMeshFile m;
};
int ipcgpu_read_tet_mesh(const char* path, ipcgpu_tetmesh** mesh, int* nV, int* nT, int* nSF)
{
    return guarded([&] {
        needArg(path && mesh && nV && nT && nSF, "null argument");
        std::unique_ptr<ipcgpu_tetmesh> h(new ipcgpu_tetmesh);
        readTetMesh(path, h->m, true);
        *nV = (int)(h->m.V.size() / 3);
        *nT = (int)(h->m.T.size() / 4);
        *nSF = (int)(h->m.SF.size() / 3);
        *mesh = h.release();
        return IPCGPU_OK;
    });
}
int ipcgpu_tet_mesh_get(const ipcgpu_tetmesh* h, double* V, int* T, int* SF)
{
    return guarded([&] {
        needArg(h != nullptr, "null mesh");
        const size_t nV = h->m.V.size() / 3, nT = h->m.T.size() / 4, nSF = h->m.SF.size() / 3;
        if (V)
            for (size_t v = 0; v < nV; ++v)
                for (int c = 0; c < 3; ++c) V[v + nV * c] = h->m.V[3 * v + c];
        if (T)
            for (size_t t = 0; t < nT; ++t)
                for (int k = 0; k < 4; ++k) T[t + nT * k] = h->m.T[4 * t + k];
        if (SF)
            for (size_t t = 0; t < nSF; ++t)
                for (int k = 0; k < 3; ++k) SF[t + nSF * k] = h->m.SF[3 * t + k];
        return IPCGPU_OK;
    });
}
void ipcgpu_tet_mesh_free(ipcgpu_tetmesh* h) { delete h; }
int ipcgpu_save_tet_mesh(const char* path, int nV, int nT, const double* V, const int* T)
{
    return guarded([&] {
        needArg(path && V && T && nV >= 4 && nT >= 1, "bad argument");
        std::vector<double> v(3 * (size_t)nV);
        std::vector<int> t(4 * (size_t)nT), sf;
        for (int i = 0; i < nV; ++i)
            for (int c = 0; c < 3; ++c) v[3 * (size_t)i + c] = V[i + (size_t)nV * c];
        for (int i = 0; i < nT; ++i)
            for (int k = 0; k < 4; ++k) {
                const int n = T[i + (size_t)nT * k];
                needArg(n >= 0 && n < nV, "element refers to a node that does not exist");
                t[4 * (size_t)i + k] = n;
            }
        findSurfaceTris(nT, t.data(), sf);
        saveTetMesh(path, nV, nT, v.data(), t.data(), sf);
        return IPCGPU_OK;
    });
}
int ipcgpu_set_energy_type(ipcgpu_ctx* c, int energyType)
{
    specChanged(c);
    return guarded([&] {
        HipMesh& m = M(c);
        needArg(energyType >= 0 && energyType <= 2, "energy type: 0 = NH, 1 = FCR, 2 = SNH");
        m.energyType = energyType;
        return IPCGPU_OK;
    });
}
int ipcgpu_set_dbc(ipcgpu_ctx* c, int n, const int* ids, int type)
{
    specChanged(c);
    return guarded([&] {
        HipMesh& m = M(c);
        bind(c);
        needArg(type >= 0 && type <= 2, "bad DirichletBCType");
        for (int i = 0; i < n; ++i) {
            needArg(ids[i] >= 0 && ids[i] < m.nV, "vertex id out of range");
            m.dbcType[ids[i]] = type;
        }
        m.uploadDBC(c->stream);
        return IPCGPU_OK;
    });
}
int ipcgpu_clear_dbc(ipcgpu_ctx* c)
{
    specChanged(c);
    return guarded([&] {
        HipMesh& m = M(c);
        bind(c);
        std::fill(m.dbcType.begin(), m.dbcType.end(), 0);
        m.uploadDBC(c->stream);
        return IPCGPU_OK;
    });
}
int ipcgpu_set_positions(ipcgpu_ctx* c, const double* V)
{
    specChanged(c);
    return guarded([&] {
        M(c);
        bind(c);
        needArg(V != nullptr, "null V");
        uploadColMajor(c, V, c->mesh->d_x);
        c->mesh->shell.limitUnchecked = c->mesh->shell.nLimited() > 0; // the stepper's last energy no longer describes these positions
        c->mesh->shell.rubberUnchecked = c->mesh->shell.nRubber() > 0;
        return IPCGPU_OK;
    });
}
int ipcgpu_get_positions(ipcgpu_ctx* c, double* V)
{
    return guarded([&] {
        M(c);
        bind(c);
        needArg(V != nullptr, "null V");
        downloadColMajor(c, c->mesh->d_x, V);
        return IPCGPU_OK;
    });
}
int ipcgpu_set_xtilde(ipcgpu_ctx* c, const double* V)
{
    specChanged(c);
    return guarded([&] {
        M(c);
        bind(c);
        needArg(V != nullptr, "null xTilta");
        uploadColMajor(c, V, c->mesh->d_xTilde);
        return IPCGPU_OK;
    });
}
int ipcgpu_get_features(ipcgpu_ctx* c, double* A, double* vol, double* mass, double* mu, double* lam)
{
    return guarded([&] {
        HipMesh& m = M(c);
        if (A && m.plastic.allocated()) { // the flow rewrites d_A on the device: the host copy is stale from the first flow on
            bind(c);
            m.d_A.download(m.restTriInv.data(), m.restTriInv.size(), c->stream);
        }
        if (A)
            for (int t = 0; t < m.nT; ++t)
                for (int k = 0; k < 9; ++k) A[9 * (size_t)t + k] = m.restTriInv[(size_t)k * m.nT + t];
        if (vol) std::memcpy(vol, m.triArea.data(), sizeof(double) * m.nT);
        if (mass) std::memcpy(mass, m.mass.data(), sizeof(double) * m.nV);
        if (mu) std::memcpy(mu, m.mu.data(), sizeof(double) * m.nT);
        if (lam) std::memcpy(lam, m.lam.data(), sizeof(double) * m.nT);
        return IPCGPU_OK;
    });
}
int ipcgpu_get_mesh_dims(ipcgpu_ctx* c, int* nV, int* nT)
{
    return guarded([&] {
        need(c != nullptr, "null context");
        if (nV) *nV = c->mesh ? c->mesh->nV : 0;
        if (nT) *nT = c->mesh ? c->mesh->nT : 0;
        return IPCGPU_OK;
    });
}
int ipcgpu_set_mesh_features(ipcgpu_ctx* c, const double* A, const double* vol, const double* mass, const double* mu, const double* lam)
{
    specChanged(c);
    return guarded([&] {
        bind(c);
        HipMesh& m = M(c);
        need(m.nV > 0 && m.nT > 0, "call ipcgpu_set_mesh first");
        if (A) {
            for (int t = 0; t < m.nT; ++t)
                for (int k = 0; k < 9; ++k) m.restTriInv[(size_t)k * m.nT + t] = A[9 * (size_t)t + k];
            m.d_A.upload(m.restTriInv, c->stream);
            m.resetPlasticHistory(c->stream); // a new rest shape has no plastic history: A0 = A, alpha = 0
        }
        if (vol) {
            m.triArea.assign(vol, vol + m.nT);
            m.d_vol.upload(m.triArea, c->stream);
        }
        if (A || vol) m.uploadFibers(c->stream); // b = A_t a and vol k of the fibred elements follow (fiber_plan.h)
        if (mass) {
            m.mass.assign(mass, mass + m.nV);
            m.d_mass.upload(m.mass, c->stream);
        }
        if (mu) {
            m.mu.assign(mu, mu + m.nT);
            m.d_mu.upload(m.mu, c->stream);
        }
        if (lam) {
            m.lam.assign(lam, lam + m.nT);
            m.d_lam.upload(m.lam, c->stream);
        }
        HIP_CHECK(hipStreamSynchronize(c->stream));
        return IPCGPU_OK;
    });
}
int ipcgpu_check_inversion(ipcgpu_ctx* c, int* ok)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(o.initialised, "call ipcgpu_opt_init first");
        *ok = o.checkInversion(M(c).energyType == 2) ? 1 : 0; // SNH: the plain mesh query (FCR keeps answering 1, as before)
        return IPCGPU_OK;
    });
}

// ---- Energy ------------------------------------------------------------------------------------------
int ipcgpu_elastic_energy(ipcgpu_ctx* c, double coef, double* E)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(o.initialised, "call ipcgpu_opt_init first");
        launch_energy(o.view(), coef, false, o.rank == 0, o.d_partial.p, (int)o.d_partial.n, o.slot(S_SCRATCH), c->stream);
        o.reduceSum(o.slot(S_SCRATCH), 1);
        *E = o.readScalar(S_SCRATCH);
        return IPCGPU_OK;
    });
}
int ipcgpu_elastic_energy_per_elem(ipcgpu_ctx* c, double* out)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(o.initialised, "call ipcgpu_opt_init first");
        DevBuf<double> tmp;
        tmp.alloc(c->mesh->nT);
        launch_energy_per_elem(o.view(), tmp.p, c->stream);
        tmp.download(out, c->mesh->nT, c->stream);
        return IPCGPU_OK;
    });
}
int ipcgpu_elastic_stress(ipcgpu_ctx* c, double* perElem, double* perNode, int* nInvalid)
{
    return guarded([&] {
        HipMesh& m = M(c);
        bind(c);
        if (c->worldSize > 1) throw UnsupportedError("stress fields on a sharded context (multi-rank fields are not implemented)");
        if (!c->stress) {
            c->stress.reset(new StressFields);
            c->stress->d_invalid.alloc(1);
            c->stress->h_invalid.alloc(1);
        }
        StressFields& sf = *c->stress;
        const size_t nT = (size_t)m.nT, nV = (size_t)m.nV;
        sf.d_elem.alloc(8 * nT);
        sf.d_invalid.zero(c->stream);
        launch_stress_elements(c->opt->view(), sf.d_elem.p, sf.d_invalid.p, c->stream);
        launch_publish(sf.d_invalid.p, sf.h_invalid.dev, 1, c->stream);
        if (perNode) {
            if (!sf.planValid) {
                std::vector<int> ptr, elems;
                if (!buildNodeElementIncidence(m.nV, m.nT, m.F.data(), ptr, elems)) throw StateError("the mesh has an element index out of range");
                sf.d_ptr.upload(ptr, c->stream);
                sf.d_elems.upload(elems, c->stream);
                HIP_CHECK(hipStreamSynchronize(c->stream)); // the staging vectors go out of scope
                sf.planValid = true;
            }
            sf.d_node.alloc(8 * nV);
            launch_stress_nodes(m.nV, m.nT, sf.d_ptr.p, sf.d_elems.p, m.d_vol.p, sf.d_elem.p, sf.d_node.p, c->stream);
        }
        HIP_CHECK(hipGetLastError());
        if (perElem && nT) HIP_CHECK(hipMemcpyAsync(perElem, sf.d_elem.p, 8 * nT * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (perNode) HIP_CHECK(hipMemcpyAsync(perNode, sf.d_node.p, 8 * nV * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_CHECK(hipStreamSynchronize(c->stream));
        if (nInvalid) *nInvalid = sf.h_invalid.p[0];
        return IPCGPU_OK;
    });
}
int ipcgpu_elastic_gradient(ipcgpu_ctx* c, double coef, int projectDBC, double* g)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(o.initialised, "call ipcgpu_opt_init first");
        o.d_gradient.zero(c->stream);
        launch_assemble(o.view(), coef, projectDBC, o.d_gradient.p, nullptr, c->stream);
        o.reduceSum(o.d_gradient.p, 3LL * c->mesh->nV);
        o.d_gradient.download(g, 3 * (size_t)c->mesh->nV, c->stream);
        return IPCGPU_OK;
    });
}
int ipcgpu_elastic_hessian_add(ipcgpu_ctx* c, double coef, int projectDBC)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(o.initialised, "call ipcgpu_opt_init first");
        need(!c->lin->rowBase.empty(), "call ipcgpu_linsys_set_pattern first");
        launch_assemble(o.view(), coef, projectDBC, nullptr, c->lin->d_a.p, c->stream);
        HIP_CHECK(hipStreamSynchronize(c->stream));
        return IPCGPU_OK;
    });
}
int ipcgpu_filter_step_size(ipcgpu_ctx* c, const double* p, double* step)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(o.initialised, "call ipcgpu_opt_init first");
        DevBuf<double> dp;
        dp.upload(p, 3 * (size_t)c->mesh->nV, c->stream);
        *step = o.filterStepSize(dp.p, *step);
        return IPCGPU_OK;
    });
}

// ---- LinSysSolver ------------------------------------------------------------------------------------
int ipcgpu_linsys_set_pattern(ipcgpu_ctx* c, int nExtra, const int* pairs)
{
    return guarded([&] {
        HipMesh& m = M(c);
        bind(c);
        c->lin->set_pattern(m, nExtra, pairs);
        return IPCGPU_OK;
    });
}
int ipcgpu_linsys_set_pattern_csr(ipcgpu_ctx* c, int n, const int* ia, const int* ja)
{
    return guarded([&] {
        needArg(c && ia && ja, "null argument");
        bind(c);
        c->lin->set_pattern_csr(n, ia, ja);
        return IPCGPU_OK;
    });
}
int ipcgpu_linsys_get_dims(ipcgpu_ctx* c, int* n, int* nnz)
{
    return guarded([&] {
        if (n) *n = L(c).getNumRows();
        if (nnz) *nnz = L(c).getNumNonzeros();
        return IPCGPU_OK;
    });
}
int ipcgpu_linsys_get_pattern(ipcgpu_ctx* c, int* ia, int* ja)
{
    return guarded([&] {
        HipLinSysSolver& l = L(c);
        if (ia) std::memcpy(ia, l.ia.data(), sizeof(int) * l.ia.size());
        if (ja) std::memcpy(ja, l.ja.data(), sizeof(int) * l.ja.size());
        return IPCGPU_OK;
    });
}
int ipcgpu_linsys_set_zero(ipcgpu_ctx* c)
{
    return guarded([&] {
        bind(c);
        L(c).setZero();
        if (c->opt) c->opt->matrixComplete = true; // whatever the caller adds from here on is whole on every rank (the handler's entry points return whole sums)
        specChanged(c);
        return IPCGPU_OK;
    });
}
int ipcgpu_linsys_get_values(ipcgpu_ctx* c, double* a)
{
    return guarded([&] {
        bind(c);
        needWholeMatrix(c);
        L(c).d_a.download(a, L(c).ja.size(), c->stream);
        return IPCGPU_OK;
    });
}
int ipcgpu_linsys_set_values(ipcgpu_ctx* c, const double* a)
{
    return guarded([&] {
        bind(c);
        HipLinSysSolver& l = L(c);
        need(l.numRows > 0, "no pattern");
        HIP_CHECK(hipMemcpyAsync(l.d_a.p, a, sizeof(double) * l.ja.size(), hipMemcpyHostToDevice, c->stream));
        HIP_CHECK(hipStreamSynchronize(c->stream));
        return IPCGPU_OK;
    });
}
int ipcgpu_linsys_apply_host_updates(ipcgpu_ctx* c, const double* delta, const unsigned char* isSet, const double* setVal)
{
    return guarded([&] {
        bind(c);
        HipLinSysSolver& l = L(c);
        need(l.numRows > 0, "no pattern");
        need(delta != nullptr, "delta must not be NULL");
        need((isSet == nullptr) == (setVal == nullptr), "isSet and setVal go together");
        const size_t nnz = l.ja.size();
        l.hostDelta.upload(delta, nnz, c->stream);
        if (isSet) {
            l.hostSetMask.upload(isSet, nnz, c->stream);
            l.hostSetVal.upload(setVal, nnz, c->stream);
        }
        launch_apply_host_updates((long long)nnz, l.hostDelta.p, isSet ? l.hostSetMask.p : nullptr, isSet ? l.hostSetVal.p : nullptr, l.d_a.p,
            c->stream);
        HIP_CHECK(hipStreamSynchronize(c->stream));
        return IPCGPU_OK;
    });
}
static int coeff(ipcgpu_ctx* c, int row, int col, double v, bool add)
{
    return guarded([&] {
        bind(c);
        HipLinSysSolver& l = L(c);
        if (row > col) return IPCGPU_OK; // LinSysSolver.hpp:331-339, 402-410: lower-triangle writes are ignored
        const int k = l.findEntry(row, col);
        needArg(k >= 0, "entry not in the sparsity pattern");
        double cur = 0.0;
        if (add) {
            HIP_CHECK(hipMemcpyAsync(&cur, l.d_a.p + k, sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HIP_CHECK(hipStreamSynchronize(c->stream));
        }
        cur = add ? cur + v : v;
        HIP_CHECK(hipMemcpyAsync(l.d_a.p + k, &cur, sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_CHECK(hipStreamSynchronize(c->stream));
        return IPCGPU_OK;
    });
}
int ipcgpu_linsys_add_coeff(ipcgpu_ctx* c, int row, int col, double v) { return coeff(c, row, col, v, true); }
int ipcgpu_linsys_set_coeff(ipcgpu_ctx* c, int row, int col, double v) { return coeff(c, row, col, v, false); }
int ipcgpu_linsys_multiply(ipcgpu_ctx* c, const double* x, double* y)
{
    return guarded([&] {
        bind(c);
        HipLinSysSolver& l = L(c);
        need(l.numRows > 0, "no pattern");
        needWholeMatrix(c);
        DevBuf<double> dx, dy;
        dx.upload(x, l.numRows, c->stream);
        dy.alloc(l.numRows);
        l.multiply(dx.p, dy.p);
        dy.download(y, l.numRows, c->stream);
        return IPCGPU_OK;
    });
}
int ipcgpu_linsys_multiply_sym(ipcgpu_ctx* c, const double* x, double* y)
{
    return guarded([&] {
        bind(c);
        HipLinSysSolver& l = L(c);
        need(l.numRows > 0, "no pattern");
        needWholeMatrix(c);
        DevBuf<double> dx, dy;
        dx.upload(x, l.numRows, c->stream);
        dy.alloc(l.numRows);
        l.multiplySym(dx.p, dy.p);
        dy.download(y, l.numRows, c->stream);
        return IPCGPU_OK;
    });
}
int ipcgpu_linsys_set_iterative(ipcgpu_ctx* c, double rel_tol, int max_iter, int precond, int max_factor_age)
{
    specChanged(c);
    return guarded([&] {
        L(c).setIterative(rel_tol, max_iter, precond, max_factor_age);
        return IPCGPU_OK;
    });
}
int ipcgpu_linsys_iter_stats(ipcgpu_ctx* c, double* out6)
{
    return guarded([&] {
        needArg(c && out6, "null argument");
        L(c).iterStats(out6);
        return IPCGPU_OK;
    });
}
int ipcgpu_linsys_coarse_stats(ipcgpu_ctx* c, double* out5)
{
    return guarded([&] {
        needArg(c && out5, "null argument");
        L(c).coarseStats(out5);
        return IPCGPU_OK;
    });
}
int ipcgpu_linsys_coarse_dims(ipcgpu_ctx* c, int* n_agg, int* n_rows, int* nnz)
{
    return guarded([&] {
        L(c).coarseDims(n_agg, n_rows, nnz);
        return IPCGPU_OK;
    });
}
int ipcgpu_linsys_coarse_get(ipcgpu_ctx* c, int* agg_of_node, int* coarse_ia, int* coarse_ja, double* coarse_a)
{
    return guarded([&] {
        bind(c);
        L(c).coarseGet(agg_of_node, coarse_ia, coarse_ja, coarse_a);
        return IPCGPU_OK;
    });
}
int ipcgpu_linsys_analyze_pattern(ipcgpu_ctx* c)
{
    return guarded([&] {
        bind(c);
        L(c).analyze_pattern(c->mesh->nV ? c->mesh.get() : nullptr);
        return IPCGPU_OK;
    });
}
int ipcgpu_linsys_factorize(ipcgpu_ctx* c)
{
    return guarded([&] {
        bind(c);
        return L(c).factorize() ? IPCGPU_OK : IPCGPU_NOT_PD;
    });
}
int ipcgpu_linsys_solve(ipcgpu_ctx* c, const double* rhs, double* x)
{
    return guarded([&] {
        bind(c);
        HipLinSysSolver& l = L(c);
        DevBuf<double> db, dx;
        db.upload(rhs, l.numRows, c->stream);
        dx.alloc(l.numRows);
        const bool ok = l.solve(db.p, dx.p);
        dx.download(x, l.numRows, c->stream);
        return ok ? IPCGPU_OK : IPCGPU_NOT_PD;
    });
}
int ipcgpu_linsys_factorize_solve(ipcgpu_ctx* c, const double* rhs, double* x, int negateRhs, int wait, int* flags2)
{
    return guarded([&] {
        bind(c);
        HipLinSysSolver& l = L(c);
        needArg(rhs && x, "null argument");
        DevBuf<double> db, dx;
        db.upload(rhs, l.numRows, c->stream);
        dx.upload(x, l.numRows, c->stream);
        bool ok = l.factorizeSolve(db.p, dx.p, wait != 0, negateRhs != 0);
        HIP_CHECK(hipStreamSynchronize(c->stream));
        ok = ok && l.lastPivotsOk();
        if (flags2) {
            flags2[0] = ok ? 0 : 1;
            flags2[1] = l.solverType == 0 ? l.devicePivotFlag() : flags2[0];
        }
        dx.download(x, l.numRows, c->stream);
        return ok ? IPCGPU_OK : IPCGPU_NOT_PD;
    });
}
int ipcgpu_linsys_precondition_diag(ipcgpu_ctx* c, const double* in, double* out)
{
    return guarded([&] {
        bind(c);
        HipLinSysSolver& l = L(c);
        needWholeMatrix(c);
        DevBuf<double> di, dout;
        di.upload(in, l.numRows, c->stream);
        dout.alloc(l.numRows);
        l.precondition_diag(di.p, dout.p);
        dout.download(out, l.numRows, c->stream);
        return IPCGPU_OK;
    });
}
int ipcgpu_linsys_set_shard(ipcgpu_ctx* c, int rank, int world)
{
    specChanged(c);
    return guarded([&] {
        needArg(c && world >= 1 && rank >= 0 && rank < world, "bad shard");
        if (world > 1 && c->lin->solverType == IPCGPU_SOLVER_PCG) {
            g_err = "the iterative solver is not sharded";
            return IPCGPU_ERR_UNSUPPORTED;
        }
        need(world == 1 || c->opt->allreduce != nullptr || c->opt->allreduceStream != nullptr, "set the all-reduce hook first (ipcgpu_opt_set_allreduce)");
        need(world == 1 || c->lin->hasExchangeHook(), "set the exchange hook first (ipcgpu_opt_set_exchange / ipcgpu_opt_set_exchange_stream): the sharded solver sends point to point");
        c->lin->setShard(rank, world, c->opt->allreduce, c->opt->allreduceUser, c->opt->allreduceStream, c->opt->allreduceStreamUser);
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_comm_stats(ipcgpu_ctx* c, double* out6)
{
    return guarded([&] {
        needArg(c && out6, "null argument");
        HipOptimizer& o = O(c);
        out6[0] = (double)o.commBytes;
        out6[1] = (double)o.commCalls;
        out6[2] = (double)L(c).exchangedBytes();
        out6[3] = (double)L(c).exchangeCalls();
        out6[4] = (double)(o.ownerMode() ? o.ownerNeededNodes : c->mesh->nV);
        out6[5] = (double)c->mesh->nV;
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_complete_matrix(ipcgpu_ctx* c)
{
    return guarded([&] {
        bind(c);
        O(c).completeMatrix();
        return IPCGPU_OK;
    });
}
int ipcgpu_linsys_exchange_stats(ipcgpu_ctx* c, double* out4)
{
    return guarded([&] {
        needArg(c && out4, "null argument");
        out4[0] = (double)L(c).sentBytes();
        out4[1] = (double)L(c).receivedBytes();
        out4[2] = (double)L(c).exchangeCalls();
        out4[3] = L(c).exchangeWaitMs();
        return IPCGPU_OK;
    });
}
int ipcgpu_linsys_entry_destinations(ipcgpu_ctx* c, long long* dst_nnz)
{
    return guarded([&] {
        bind(c);
        needArg(c && dst_nnz, "null argument");
        need(L(c).solverType == IPCGPU_SOLVER_MULTIFRONTAL && L(c).analyzed(), "the multifrontal solver has not analysed a pattern yet");
        L(c).entryDestinations(dst_nnz);
        return IPCGPU_OK;
    });
}
int ipcgpu_linsys_shard_stats(ipcgpu_ctx* c, double* out2)
{
    return guarded([&] {
        out2[0] = L(c).solverWorld();
        out2[1] = L(c).sharedFlopFraction();
        return IPCGPU_OK;
    });
}
int ipcgpu_linsys_set_tuning(ipcgpu_ctx* c, double bulk_min_mb, int bulk_block)
{
    return guarded([&] {
        needArg(c != nullptr, "null context");
        needArg(bulk_min_mb >= 0.0 && bulk_block >= 64 && bulk_block <= 4096, "set_tuning: bulk_min_mb >= 0, 64 <= bulk_block <= 4096");
        L(c).setBulkTuning(bulk_min_mb, bulk_block);
        return IPCGPU_OK;
    });
}
int ipcgpu_linsys_critical_path(ipcgpu_ctx* c, double* out5)
{
    return guarded([&] {
        needArg(c && out5, "null argument");
        L(c).criticalPath(out5);
        return IPCGPU_OK;
    });
}
int ipcgpu_linsys_stats(ipcgpu_ctx* c, double* st)
{
    return guarded([&] {
        const MfSymbolic& s = L(c).symbolic();
        st[0] = (double)s.nnzL;
        st[1] = s.flops;
        st[2] = s.ns;
        st[3] = (double)s.levelPtr.size() - 1;
        return IPCGPU_OK;
    });
}

// ---- SelfCollisionHandler ----------------------------------------------------------------------------
static HipContact& CT(ipcgpu_ctx* c)
{
    M(c);
    if (!c->contact) {
        c->contact.reset(new HipContact(c->stream));
        applyContactShard(c);
    }
    return *c->contact;
}
int ipcgpu_set_surface(ipcgpu_ctx* c, int nSF, const int* SF)
{
    specChanged(c);
    return guarded([&] {
        HipMesh& m = M(c);
        bind(c);
        needArg(nSF >= 0 && (SF || nSF == 0), "bad surface");
        m.addSurfaceEdges(nSF, SF);
        CT(c).setSurface(m, nSF, SF);
        return IPCGPU_OK;
    });
}
int ipcgpu_set_surface_codim(ipcgpu_ctx* c, int nSF, const int* SF, int nCE, const int* CE)
{
    specChanged(c);
    return guarded([&] {
        HipMesh& m = M(c);
        bind(c);
        needArg(nSF >= 0 && (SF || nSF == 0), "bad surface");
        needArg(nCE >= 0 && (CE || nCE == 0), "bad codimensional segments");
        m.addSurfaceEdges(nSF, SF, nCE, CE);
        CT(c).setSurface(m, nSF, SF, nCE, CE);
        return IPCGPU_OK;
    });
}
int ipcgpu_set_exact_predicates(ipcgpu_ctx* c, int on)
{
    specChanged(c);
    return guarded([&] {
        CT(c).exactPredicates = on != 0;
        return IPCGPU_OK;
    });
}
int ipcgpu_get_surface(ipcgpu_ctx* c, int* counts, int* SVI, int* SFE)
{
    return guarded([&] {
        HipContact& k = CT(c);
        if (counts) {
            counts[0] = k.nSVI;
            counts[1] = k.nSF;
            counts[2] = k.nSFE;
        }
        if (SVI) std::memcpy(SVI, k.SVI.data(), sizeof(int) * k.SVI.size());
        if (SFE)
            for (size_t i = 0; i < k.SFEdges.size(); ++i) {
                SFE[2 * i] = k.SFEdges[i].first;
                SFE[2 * i + 1] = k.SFEdges[i].second;
            }
        return IPCGPU_OK;
    });
}
int ipcgpu_contact_build(ipcgpu_ctx* c, double dHat, int* counts)
{
    return guarded([&] {
        HipMesh& m = M(c);
        bind(c);
        needArg(dHat > 0, "dHat must be positive");
        HipContact& k = CT(c);
        k.buildConstraintSet(m, m.d_x.p, m.d_dbc.p, dHat);
        if (counts) {
            counts[0] = k.nActive();
            counts[1] = k.nPara();
            counts[2] = k.nCand();
        }
        return IPCGPU_OK;
    });
}
int ipcgpu_set_codim_nodes(ipcgpu_ctx* c, int n, const int* ids, const double* mass)
{
    specChanged(c);
    return guarded([&] {
        HipMesh& m = M(c);
        bind(c);
        needArg(n >= 0 && ((ids && mass) || !n), "bad codimensional node list");
        need(!c->opt->initialised, "ipcgpu_set_codim_nodes must come before ipcgpu_opt_init (dHat and kappa derive from the mesh extent and mass)");
        m.setCodimNodes(n, ids, mass, c->stream);
        return IPCGPU_OK;
    });
}
// ---- Elastic shells -----------------------------------------------------------------------------------
int ipcgpu_set_shell(ipcgpu_ctx* c, int nTri, const int* tri, const double* thickness, const double* YM, const double* PR, const double* rho, double bendScale)
{
    return setCodimBody(c, HipOptimizer::CODIM_SHELL, nTri >= 0 && ((tri && thickness && YM && PR && rho) || !nTri), nTri,
        // a pattern built before this call lacks the opposite pairs of the hinges: setCodimBody rebuilds it from the new vNeighbor (without extra pairs)
        [&](HipMesh& m) { m.setShell(nTri, tri, thickness, YM, PR, rho, bendScale, c->stream); });
}
int ipcgpu_shell_get(ipcgpu_ctx* c, int* counts2, int* hinge, double* restAngle, double* hingeWeight, double* area, double* mass)
{
    return guarded([&] {
        const ShellPlan& p = M(c).shell.plan;
        if (counts2) {
            counts2[0] = p.nTri;
            counts2[1] = p.nHinge;
        }
        if (hinge) std::copy(p.hinge.begin(), p.hinge.end(), hinge);
        if (restAngle) std::copy(p.restAngle.begin(), p.restAngle.end(), restAngle);
        if (hingeWeight) std::copy(p.hingeWeight.begin(), p.hingeWeight.end(), hingeWeight);
        if (area) std::copy(p.area.begin(), p.area.end(), area);
        if (mass) {
            std::fill(mass, mass + c->mesh->nV, 0.0);
            std::copy(p.mass.begin(), p.mass.end(), mass);
        }
        return IPCGPU_OK;
    });
}
int ipcgpu_shell_energy(ipcgpu_ctx* c, double coef, double* E)
{
    return guarded([&] { return codimEnergy(c, SHELL_AND_LIMIT, coef, E); });
}
int ipcgpu_shell_energy_per_elem(ipcgpu_ctx* c, double* perTri, double* perHinge)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        const HipShell& sh = c->mesh->shell;
        if (!sh.nTri()) return IPCGPU_OK;
        DevBuf<double> t, h;
        t.alloc(sh.nTri());
        h.alloc(sh.nHinge());
        launch_shell_energy_per_elem(o.shellView(c->mesh->d_x.p), perTri ? t.p : nullptr, perHinge ? h.p : nullptr, c->stream);
        HIP_CHECK(hipGetLastError());
        if (perTri) t.download(perTri, sh.nTri(), c->stream);
        if (perHinge) h.download(perHinge, sh.nHinge(), c->stream);
        return IPCGPU_OK;
    });
}
int ipcgpu_shell_gradient_add(ipcgpu_ctx* c, double coef, int projectDBC, double* g)
{
    return guarded([&] { return codimGradientAdd(c, SHELL_AND_LIMIT, coef, projectDBC, g); });
}
int ipcgpu_shell_hessian_add(ipcgpu_ctx* c, double coef, int projectDBC)
{
    specChanged(c);
    return guarded([&] { return codimHessianAdd(c, SHELL_AND_LIMIT, coef, projectDBC, SHELL_MISS); });
}
// ---- Strain limit of the shells -----------------------------------------------------------------------
int ipcgpu_shell_set_strain_limit(ipcgpu_ctx* c, const double* limit, const double* onset, const double* stiff)
{
    specChanged(c);
    return guarded([&] {
        HipMesh& m = M(c);
        bind(c);
        m.setShellStrainLimit(limit, onset, stiff, c->stream);
        return IPCGPU_OK;
    });
}
int ipcgpu_shell_limit_energy(ipcgpu_ctx* c, double coef, double* E)
{
    return guarded([&] { return codimEnergy(c, LIMIT_ALONE, coef, E); });
}
int ipcgpu_shell_limit_energy_per_elem(ipcgpu_ctx* c, double* perTri)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        const HipShell& sh = c->mesh->shell;
        if (!sh.nTri() || !perTri) return IPCGPU_OK;
        DevBuf<double> t;
        t.alloc(sh.nTri());
        launch_shell_limit_energy_per_elem(o.shellLimitView(c->mesh->d_x.p), t.p, c->stream);
        HIP_CHECK(hipGetLastError());
        t.download(perTri, sh.nTri(), c->stream);
        return IPCGPU_OK;
    });
}
int ipcgpu_shell_limit_gradient_add(ipcgpu_ctx* c, double coef, int projectDBC, double* g)
{
    return guarded([&] { return codimGradientAdd(c, LIMIT_ALONE, coef, projectDBC, g); });
}
int ipcgpu_shell_limit_hessian_add(ipcgpu_ctx* c, double coef, int projectDBC)
{
    specChanged(c);
    return guarded([&] { return codimHessianAdd(c, LIMIT_ALONE, coef, projectDBC, SHELL_MISS); });
}
int ipcgpu_shell_stretch(ipcgpu_ctx* c, double* sigma, double* maxRatio)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        o.shellStretch(sigma, maxRatio, nullptr);
        return IPCGPU_OK;
    });
}
// ---- Rubber membrane of the shells --------------------------------------------------------------------
int ipcgpu_shell_set_membrane(ipcgpu_ctx* c, const int* model, const double* alpha)
{
    specChanged(c);
    return guarded([&] {
        HipMesh& m = M(c);
        bind(c);
        m.setShellMembrane(model, alpha, c->stream);
        return IPCGPU_OK;
    });
}
int ipcgpu_shell_membrane_get(ipcgpu_ctx* c, int* model, double* alpha)
{
    return guarded([&] {
        const HipShell& sh = M(c).shell;
        if (model) std::fill(model, model + sh.nTri(), 0);
        if (alpha) std::fill(alpha, alpha + sh.nTri(), 0.0);
        if (!sh.nRubber()) return IPCGPU_OK;
        if (model) std::copy(sh.rubber.model.begin(), sh.rubber.model.end(), model);
        if (alpha) std::copy(sh.rubber.alpha.begin(), sh.rubber.alpha.end(), alpha);
        return IPCGPU_OK;
    });
}
int ipcgpu_shell_rubber_energy(ipcgpu_ctx* c, double coef, double* E)
{
    return guarded([&] { return codimEnergy(c, RUBBER_ALONE, coef, E); });
}
int ipcgpu_shell_rubber_energy_per_elem(ipcgpu_ctx* c, double* perTri)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        const HipShell& sh = c->mesh->shell;
        if (!sh.nTri() || !perTri) return IPCGPU_OK;
        DevBuf<double> t;
        t.alloc(sh.nTri());
        launch_shell_rubber_energy_per_elem(o.shellRubberView(c->mesh->d_x.p), t.p, c->stream);
        HIP_CHECK(hipGetLastError());
        t.download(perTri, sh.nTri(), c->stream);
        return IPCGPU_OK;
    });
}
int ipcgpu_shell_rubber_gradient_add(ipcgpu_ctx* c, double coef, int projectDBC, double* g)
{
    return guarded([&] { return codimGradientAdd(c, RUBBER_ALONE, coef, projectDBC, g); });
}
int ipcgpu_shell_rubber_hessian_add(ipcgpu_ctx* c, double coef, int projectDBC)
{
    specChanged(c);
    return guarded([&] { return codimHessianAdd(c, RUBBER_ALONE, coef, projectDBC, SHELL_MISS); });
}
int ipcgpu_shell_thickness(ipcgpu_ctx* c, double* h)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        const HipShell& sh = c->mesh->shell;
        if (!sh.nTri() || !h) return IPCGPU_OK;
        std::copy(sh.plan.thickness.begin(), sh.plan.thickness.end(), h);
        if (!sh.nRubber()) return IPCGPU_OK;
        std::vector<double> sigma(2 * (size_t)sh.nTri());
        o.shellStretch(sigma.data(), nullptr, nullptr);
        for (int t : sh.rubber.tri) h[t] = sh.plan.thickness[(size_t)t] / (sigma[2 * (size_t)t] * sigma[2 * (size_t)t + 1]); // incompressible: lambda_3 = 1 / (sigma1 sigma2)
        return IPCGPU_OK;
    });
}
// ---- Woven cloth of the shells (shell_weave_kernels.h; the reference has no counterpart) ----------------------------------------------------------
int ipcgpu_shell_set_weave(ipcgpu_ctx* c, const int* woven, const double* dir, const double* E1, const double* E2, const double* G12, const double* nu12,
    const double* bendWarp, const double* bendWeft)
{
    specChanged(c);
    return guarded([&] {
        HipMesh& m = M(c);
        bind(c);
        m.setShellWeave(woven, dir, E1, E2, G12, nu12, bendWarp, bendWeft, c->stream);
        return IPCGPU_OK;
    });
}
int ipcgpu_shell_weave_get(ipcgpu_ctx* c, int* woven, double* a, double* const4, double* hingeFactor)
{
    return guarded([&] {
        const HipShell& sh = M(c).shell;
        if (woven) std::fill(woven, woven + sh.nTri(), 0);
        if (a) std::fill(a, a + 2 * (size_t)sh.nTri(), 0.0);
        if (const4) std::fill(const4, const4 + 4 * (size_t)sh.nTri(), 0.0);
        if (hingeFactor) std::fill(hingeFactor, hingeFactor + sh.nHinge(), 1.0);
        if (!sh.nWoven()) return IPCGPU_OK;
        if (woven) std::copy(sh.weave.woven.begin(), sh.weave.woven.end(), woven);
        if (a) std::copy(sh.weave.a.begin(), sh.weave.a.end(), a);
        if (const4) std::copy(sh.weave.const4.begin(), sh.weave.const4.end(), const4);
        if (hingeFactor) std::copy(sh.weave.hingeFactor.begin(), sh.weave.hingeFactor.end(), hingeFactor);
        return IPCGPU_OK;
    });
}
int ipcgpu_shell_weave_energy(ipcgpu_ctx* c, double coef, double* E)
{
    return guarded([&] { return codimEnergy(c, WEAVE_ALONE, coef, E); });
}
int ipcgpu_shell_weave_energy_per_elem(ipcgpu_ctx* c, double* perTri)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        const HipShell& sh = c->mesh->shell;
        if (!sh.nTri() || !perTri) return IPCGPU_OK;
        DevBuf<double> t;
        t.alloc(sh.nTri());
        launch_shell_weave_energy_per_elem(o.shellWeaveView(c->mesh->d_x.p), t.p, c->stream);
        HIP_CHECK(hipGetLastError());
        t.download(perTri, sh.nTri(), c->stream);
        return IPCGPU_OK;
    });
}
int ipcgpu_shell_weave_gradient_add(ipcgpu_ctx* c, double coef, int projectDBC, double* g)
{
    return guarded([&] { return codimGradientAdd(c, WEAVE_ALONE, coef, projectDBC, g); });
}
int ipcgpu_shell_weave_hessian_add(ipcgpu_ctx* c, double coef, int projectDBC)
{
    specChanged(c);
    return guarded([&] { return codimHessianAdd(c, WEAVE_ALONE, coef, projectDBC, SHELL_MISS); });
}
int ipcgpu_shell_weave_state(ipcgpu_ctx* c, double* perTri6)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        const HipShell& sh = c->mesh->shell;
        if (!sh.nTri() || !perTri6) return IPCGPU_OK;
        DevBuf<double> t;
        t.alloc(6 * (size_t)sh.nTri());
        launch_shell_weave_state(o.shellWeaveView(c->mesh->d_x.p), t.p, c->stream);
        HIP_CHECK(hipGetLastError());
        t.download(perTri6, 6 * (size_t)sh.nTri(), c->stream);
        return IPCGPU_OK;
    });
}
// ---- Plastic flow of the shells (shell_plastic_kernels.h; the reference has no counterpart) ------------------------------------------------------
int ipcgpu_shell_set_plasticity(ipcgpu_ctx* c, int triBegin, int triEnd, double yield, double bendYield, double creep, double harden)
{
    specChanged(c);
    return guarded([&] {
        HipMesh& m = M(c);
        bind(c);
        if (c->worldSize > 1) throw UnsupportedError("shell plasticity on a sharded context"); // (first: a sharded context cannot hold a shell at all)
        need(m.shell.nTri() > 0, "shell_set_plasticity: no shell is set (call ipcgpu_set_shell first)");
        m.setShellPlasticity(triBegin, triEnd, yield, bendYield, creep, harden, c->stream);
        return IPCGPU_OK;
    });
}
int ipcgpu_shell_plastic_get(ipcgpu_ctx* c, double* yield, double* bendYield, double* creep, double* harden, double* alpha, double* triConst, double* B0,
    double* hingePar, double* alphaB, double* thetaBar, double* thetaBar0)
{
    return guarded([&] {
        HipMesh& m = M(c);
        bind(c);
        const HipShell& sh = m.shell;
        const HipShellPlastic& h = sh.plastic;
        const size_t nTri = (size_t)sh.nTri(), nH = (size_t)sh.nHinge();
        if (!nTri) return IPCGPU_OK;
        if (triConst) sh.d_triConst.download(triConst, 6 * nTri, c->stream);
        if (thetaBar) sh.d_hingeConst.download(thetaBar, nH, c->stream);
        if (!h.allocated()) { // never set: everything elastic, no history, the rest records are the device's own
            for (size_t t = 0; t < nTri; ++t) {
                if (yield) yield[t] = INFINITY;
                if (bendYield) bendYield[t] = INFINITY;
                if (creep) creep[t] = INFINITY;
                if (harden) harden[t] = 0.0;
                if (alpha) alpha[t] = 0.0;
            }
            if (B0) sh.d_triConst.download(B0, 4 * nTri, c->stream);
            if (thetaBar0) sh.d_hingeConst.download(thetaBar0, nH, c->stream);
            for (size_t i = 0; i < nH; ++i) {
                if (hingePar) {
                    hingePar[i] = hingePar[nH + i] = INFINITY;
                    hingePar[2 * nH + i] = 0.0;
                    hingePar[3 * nH + i] = NAN; // (g is computed with the plan)
                }
                if (alphaB) alphaB[i] = 0.0;
            }
            return IPCGPU_OK;
        }
        if (yield) std::memcpy(yield, h.plan.yield.data(), sizeof(double) * nTri);
        if (bendYield) std::memcpy(bendYield, h.plan.bendYield.data(), sizeof(double) * nTri);
        if (creep) std::memcpy(creep, h.plan.creep.data(), sizeof(double) * nTri);
        if (harden) std::memcpy(harden, h.plan.harden.data(), sizeof(double) * nTri);
        if (alpha) h.d_alpha.download(alpha, nTri, c->stream);
        if (B0) h.d_B0.download(B0, 4 * nTri, c->stream);
        if (hingePar && nH) {
            std::memcpy(hingePar, h.plan.hingeYield.data(), sizeof(double) * nH);
            std::memcpy(hingePar + nH, h.plan.hingeCreep.data(), sizeof(double) * nH);
            std::memcpy(hingePar + 2 * nH, h.plan.hingeHarden.data(), sizeof(double) * nH);
            std::memcpy(hingePar + 3 * nH, h.plan.hingeG.data(), sizeof(double) * nH);
        }
        if (alphaB) h.d_alphaB.download(alphaB, nH, c->stream);
        if (thetaBar0) h.d_thetaBar0.download(thetaBar0, nH, c->stream);
        return IPCGPU_OK;
    });
}
int ipcgpu_shell_plastic_update(ipcgpu_ctx* c, double dt, int* counts4)
{
    specChanged(c);
    return guarded([&] {
        HipMesh& m = M(c);
        bind(c);
        needArg(dt > 0.0 && std::isfinite(dt), "shell_plastic_update: the time step must be positive and finite");
        int cnt[SPC_COUNT] = { 0, 0, 0, 0 };
        if (m.shell.plastic.on()) {
            c->opt->shellPlasticFlow(m.d_x.p, dt);
            HIP_CHECK(hipGetLastError());
            m.shell.plastic.d_count.download(cnt, SPC_COUNT, c->stream);
        }
        if (counts4) std::copy(cnt, cnt + SPC_COUNT, counts4);
        return IPCGPU_OK;
    });
}
int ipcgpu_shell_plastic_state(ipcgpu_ctx* c, double* perTri, double* perHinge, double* totals7)
{
    return guarded([&] {
        HipMesh& m = M(c);
        bind(c);
        HipShell& sh = m.shell;
        HipShellPlastic& h = sh.plastic;
        const size_t nTri = (size_t)sh.nTri(), nH = (size_t)sh.nHinge();
        if (totals7) std::fill(totals7, totals7 + 7, 0.0);
        if (!h.allocated()) {
            for (size_t t = 0; t < nTri && perTri; ++t) {
                perTri[t] = NAN; // (n is not evaluated without the state arrays)
                perTri[nTri + t] = INFINITY;
                perTri[2 * nTri + t] = 0.0;
                perTri[3 * nTri + t] = 1.0;
            }
            for (size_t i = 0; i < nH && perHinge; ++i) {
                perHinge[i] = NAN;
                perHinge[nH + i] = INFINITY;
                perHinge[2 * nH + i] = perHinge[3 * nH + i] = 0.0;
            }
            return IPCGPU_OK;
        }
        if (!perTri && !perHinge && !totals7) return IPCGPU_OK;
        const ShellPlasticView v = c->opt->shellPlasticView(m.d_x.p, 1.0);
        if (perTri) h.d_stateTri.ensure(4 * nTri);
        if (perHinge) h.d_stateHinge.ensure(4 * nH);
        h.d_partial.ensure(SPT_COUNT * (size_t)shell_plastic_state_blocks(v));
        launch_shell_plastic_state(v, perTri ? h.d_stateTri.p : nullptr, perHinge && nH ? h.d_stateHinge.p : nullptr, h.d_partial.p, totals7 ? h.d_totals.p : nullptr, c->stream);
        HIP_CHECK(hipGetLastError());
        if (perTri) h.d_stateTri.download(perTri, 4 * nTri, c->stream);
        if (perHinge) h.d_stateHinge.download(perHinge, 4 * nH, c->stream);
        if (totals7) {
            int cnt[SPC_COUNT];
            double tot[SPT_COUNT];
            h.d_count.download(cnt, SPC_COUNT, c->stream);
            h.d_totals.download(tot, SPT_COUNT, c->stream);
            for (int k = 0; k < SPC_COUNT; ++k) totals7[k] = cnt[k];
            for (int k = 0; k < SPT_COUNT; ++k) totals7[SPC_COUNT + k] = tot[k];
        }
        return IPCGPU_OK;
    });
}
int ipcgpu_shell_plastic_set_state(ipcgpu_ctx* c, const double* B, const double* alpha, const double* thetaBar, const double* alphaB)
{
    specChanged(c);
    return guarded([&] {
        HipMesh& m = M(c);
        bind(c);
        HipShell& sh = m.shell;
        need(sh.plastic.allocated(), "call ipcgpu_shell_set_plasticity first");
        const size_t nTri = (size_t)sh.nTri(), nH = (size_t)sh.nHinge();
        for (size_t t = 0; t < nTri && alpha; ++t) needArg(alpha[t] >= 0.0 && std::isfinite(alpha[t]), "shell_plastic_set_state: the accumulated plastic strain must be finite and not negative");
        for (size_t i = 0; i < nH && alphaB; ++i) needArg(alphaB[i] >= 0.0 && std::isfinite(alphaB[i]), "shell_plastic_set_state: the accumulated plastic strain must be finite and not negative");
        for (size_t k = 0; k < 4 * nTri && B; ++k) needArg(std::isfinite(B[k]), "shell_plastic_set_state: B is not finite");
        for (size_t i = 0; i < nH && thetaBar; ++i) needArg(std::isfinite(thetaBar[i]), "shell_plastic_set_state: thetaBar is not finite");
        if (B) HIP_CHECK(hipMemcpyAsync(sh.d_triConst.p, B, 4 * nTri * sizeof(double), hipMemcpyHostToDevice, c->stream));
        if (alpha) HIP_CHECK(hipMemcpyAsync(sh.plastic.d_alpha.p, alpha, nTri * sizeof(double), hipMemcpyHostToDevice, c->stream));
        if (thetaBar && nH) HIP_CHECK(hipMemcpyAsync(sh.d_hingeConst.p, thetaBar, nH * sizeof(double), hipMemcpyHostToDevice, c->stream));
        if (alphaB && nH) HIP_CHECK(hipMemcpyAsync(sh.plastic.d_alphaB.p, alphaB, nH * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_CHECK(hipStreamSynchronize(c->stream));
        return IPCGPU_OK;
    });
}
int ipcgpu_shell_plastic_reset(ipcgpu_ctx* c)
{
    specChanged(c);
    return guarded([&] {
        HipMesh& m = M(c);
        bind(c);
        HipShell& sh = m.shell;
        if (!sh.plastic.allocated()) return IPCGPU_OK; // no history to forget
        const size_t nTri = (size_t)sh.nTri(), nH = (size_t)sh.nHinge();
        HIP_CHECK(hipMemcpyAsync(sh.d_triConst.p, sh.plastic.d_B0.p, 4 * nTri * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        if (nH) HIP_CHECK(hipMemcpyAsync(sh.d_hingeConst.p, sh.plastic.d_thetaBar0.p, nH * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        sh.plastic.d_alpha.zero(c->stream);
        sh.plastic.d_alphaB.zero(c->stream);
        sh.plastic.d_count.zero(c->stream);
        HIP_CHECK(hipStreamSynchronize(c->stream));
        return IPCGPU_OK;
    });
}
// ---- Elastic rods -------------------------------------------------------------------------------------
int ipcgpu_set_rod(ipcgpu_ctx* c, int nSeg, const int* seg, const double* radius, const double* YM, const double* rho, double bendScale)
{
    return setCodimBody(c, HipOptimizer::CODIM_ROD, nSeg >= 0 && ((seg && radius && YM && rho) || !nSeg), nSeg,
        // a pattern built before this call lacks the outer pairs of the bending triples: setCodimBody rebuilds it from the new vNeighbor (without extra pairs)
        [&](HipMesh& m) { m.setRod(nSeg, seg, radius, YM, rho, bendScale, c->stream); });
}
int ipcgpu_rod_get(ipcgpu_ctx* c, int* counts2, int* bend, double* restLen, double* ks, double* kb, double* restKb, double* mass)
{
    return guarded([&] {
        const RodPlan& p = M(c).rod.plan;
        if (counts2) {
            counts2[0] = p.nSeg;
            counts2[1] = p.nBend;
        }
        if (bend) std::copy(p.bend.begin(), p.bend.end(), bend);
        if (restLen) std::copy(p.segConst.begin(), p.segConst.begin() + p.nSeg, restLen);
        if (ks) std::copy(p.segConst.begin() + p.nSeg, p.segConst.end(), ks);
        if (kb) std::copy(p.bendK.begin(), p.bendK.end(), kb);
        if (restKb) std::copy(p.restKb.begin(), p.restKb.end(), restKb);
        if (mass) {
            std::fill(mass, mass + c->mesh->nV, 0.0);
            std::copy(p.mass.begin(), p.mass.end(), mass);
        }
        return IPCGPU_OK;
    });
}
int ipcgpu_rod_energy(ipcgpu_ctx* c, double coef, double* E)
{
    return guarded([&] { return codimEnergy(c, ROD, coef, E); });
}
int ipcgpu_rod_energy_per_elem(ipcgpu_ctx* c, double* perSeg, double* perBend)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        const HipRod& r = c->mesh->rod;
        if (!r.nSeg()) return IPCGPU_OK;
        DevBuf<double> t, h;
        t.alloc(r.nSeg());
        h.alloc(r.nBend());
        h.zero(c->stream); // (with `bend 0` no triple is evaluated: its terms are 0)
        launch_rod_energy_per_elem(o.rodView(c->mesh->d_x.p), perSeg ? t.p : nullptr, perBend ? h.p : nullptr, c->stream);
        HIP_CHECK(hipGetLastError());
        if (perSeg) t.download(perSeg, r.nSeg(), c->stream);
        if (perBend) h.download(perBend, r.nBend(), c->stream);
        return IPCGPU_OK;
    });
}
int ipcgpu_rod_gradient_add(ipcgpu_ctx* c, double coef, int projectDBC, double* g)
{
    return guarded([&] { return codimGradientAdd(c, ROD, coef, projectDBC, g); });
}
int ipcgpu_rod_hessian_add(ipcgpu_ctx* c, double coef, int projectDBC)
{
    specChanged(c);
    return guarded([&] { return codimHessianAdd(c, ROD, coef, projectDBC, ROD_MISS); });
}
// ---- Attachments ---------------------------------------------------------------------------------------
int ipcgpu_set_attachments(ipcgpu_ctx* c, int n, const int* nodesA, const double* weightsA, const int* nodesB, const double* weightsB, const double* k, const double* L)
{
    return setCodimBody(c, HipOptimizer::CODIM_ATTACH, n >= 0 && ((nodesA && weightsA && nodesB && weightsB && k && L) || !n), n,
        // a pattern built before this call lacks the node pairs of the attachments: setCodimBody rebuilds it from the new vNeighbor (without extra pairs)
        [&](HipMesh& m) { m.setAttachments(n, nodesA, weightsA, nodesB, weightsB, k, L, c->stream); });
}
int ipcgpu_attach_get(ipcgpu_ctx* c, int* count, int* counts, int* nodes, double* coefs, double* k, double* L, double* restDist)
{
    return guarded([&] {
        const HipMesh& m = M(c);
        const AttachPlan& p = m.attach.plan;
        if (count) *count = p.n;
        if (counts) std::copy(p.count.begin(), p.count.end(), counts);
        if (nodes) std::copy(p.node.begin(), p.node.end(), nodes);
        if (coefs) std::copy(p.coef.begin(), p.coef.end(), coefs);
        if (k) std::copy(p.kL.begin(), p.kL.begin() + p.n, k);
        if (L) std::copy(p.kL.begin() + p.n, p.kL.end(), L);
        if (restDist)
            for (int i = 0; i < p.n; ++i) restDist[i] = attachRestDistance(p, i, m.nV, m.V_rest.data());
        return IPCGPU_OK;
    });
}
int ipcgpu_attach_energy(ipcgpu_ctx* c, double coef, double* E)
{
    return guarded([&] { return codimEnergy(c, ATTACH, coef, E); });
}
int ipcgpu_attach_energy_per_elem(ipcgpu_ctx* c, double* perAttach)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        const int n = c->mesh->attach.n();
        if (!n || !perAttach) return IPCGPU_OK;
        DevBuf<double> e;
        e.alloc(n);
        launch_attach_energy_per_elem(o.attachView(c->mesh->d_x.p), e.p, c->stream);
        HIP_CHECK(hipGetLastError());
        e.download(perAttach, n, c->stream);
        return IPCGPU_OK;
    });
}
int ipcgpu_attach_gradient_add(ipcgpu_ctx* c, double coef, int projectDBC, double* g)
{
    return guarded([&] { return codimGradientAdd(c, ATTACH, coef, projectDBC, g); });
}
int ipcgpu_attach_hessian_add(ipcgpu_ctx* c, double coef, int projectDBC)
{
    specChanged(c);
    return guarded([&] { return codimHessianAdd(c, ATTACH, coef, projectDBC, ATTACH_MISS); });
}
int ipcgpu_attach_state(ipcgpu_ctx* c, double* length, double* force)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        const int n = c->mesh->attach.n();
        if (!n) return IPCGPU_OK;
        DevBuf<double> l, f;
        if (length) l.alloc(n);
        if (force) f.alloc(n);
        launch_attach_state(o.attachView(c->mesh->d_x.p), length ? l.p : nullptr, force ? f.p : nullptr, c->stream);
        HIP_CHECK(hipGetLastError());
        if (length) l.download(length, n, c->stream);
        if (force) f.download(force, n, c->stream);
        return IPCGPU_OK;
    });
}
// ---- Pressure chambers ---------------------------------------------------------------------------------
int ipcgpu_set_chambers(ipcgpu_ctx* c, int nCh, const int* triEnd, const int* tri, const double* pressure)
{
    // (setCodimBody counts triangles: nCh == 0 with no chamber set is "nothing to remove")
    return setCodimBody(c, HipOptimizer::CODIM_CHAMBER, nCh >= 0 && ((triEnd && tri && pressure) || !nCh), nCh,
        // a pattern built before this call lacks the edges of the chambers' triangles: setCodimBody rebuilds it from the new vNeighbor (without extra pairs)
        [&](HipMesh& m) { m.setChambers(nCh, triEnd, tri, pressure, c->stream); });
}
int ipcgpu_chamber_set_pressure(ipcgpu_ctx* c, const double* pressure)
{
    specChanged(c);
    return guarded([&] {
        HipMesh& m = M(c);
        bind(c);
        m.setChamberPressure(pressure, c->stream);
        return IPCGPU_OK;
    });
}
int ipcgpu_chamber_get(ipcgpu_ctx* c, int* counts2, int* triEnd, int* tri, double* restVolume, double* pressure)
{
    return guarded([&] {
        const ChamberPlan& p = M(c).chamber.plan;
        if (counts2) {
            counts2[0] = p.n;
            counts2[1] = p.nTri;
        }
        if (triEnd) std::copy(p.triEnd.begin(), p.triEnd.end(), triEnd);
        if (tri) std::copy(p.tri.begin(), p.tri.end(), tri);
        if (restVolume) std::copy(p.restVolume.begin(), p.restVolume.end(), restVolume);
        if (pressure) std::copy(p.pressure.begin(), p.pressure.end(), pressure);
        return IPCGPU_OK;
    });
}
int ipcgpu_chamber_state(ipcgpu_ctx* c, double* volume, double* area, double* refPoint)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        const HipChamber& h = c->mesh->chamber;
        const int n = h.n();
        if (!n) return IPCGPU_OK;
        DevBuf<double> v, a;
        if (volume) v.alloc(n);
        if (area) a.alloc(n);
        launch_chamber_state(o.chamberView(c->mesh->d_x.p), volume ? v.p : nullptr, area ? a.p : nullptr, nullptr, c->stream);
        HIP_CHECK(hipGetLastError());
        if (volume) v.download(volume, n, c->stream);
        if (area) a.download(area, n, c->stream);
        if (refPoint) h.d_ref.download(refPoint, 3 * (size_t)n, c->stream); // r_c as the evaluations use it now, not the centroid mean of the current positions
        return IPCGPU_OK;
    });
}
int ipcgpu_chamber_energy(ipcgpu_ctx* c, double coef, double* E)
{
    return guarded([&] { return codimEnergy(c, CHAMBER, coef, E); });
}
int ipcgpu_chamber_energy_per_elem(ipcgpu_ctx* c, double* perTri)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        const int n = c->mesh->chamber.nTri();
        if (!n || !perTri) return IPCGPU_OK;
        DevBuf<double> e;
        e.alloc(n);
        const HipChamber& h = c->mesh->chamber;
        launch_chamber_energy_per_elem(o.chamberView(c->mesh->d_x.p, HipOptimizer::CHAMBER_P_CONSTANT), e.p, c->stream);
        if (h.nGas()) { // a gas chamber's triangle gets the share W_c V_t / V_c
            launch_chamber_gas_update(o.chamberView(c->mesh->d_x.p), h.gasView(), 0.0, nullptr, false, c->stream);
            launch_chamber_gas_energy_per_elem(o.chamberView(c->mesh->d_x.p), h.d_isGas.p, h.d_gasState.p, e.p, c->stream);
        }
        HIP_CHECK(hipGetLastError());
        e.download(perTri, n, c->stream);
        return IPCGPU_OK;
    });
}
int ipcgpu_chamber_gradient_add(ipcgpu_ctx* c, double coef, int projectDBC, double* g)
{
    return guarded([&] { return codimGradientAdd(c, CHAMBER, coef, projectDBC, g); });
}
int ipcgpu_chamber_hessian_add(ipcgpu_ctx* c, double coef, int projectDBC)
{
    specChanged(c);
    return guarded([&] { return codimHessianAdd(c, CHAMBER, coef, projectDBC, CHAMBER_MISS); });
}
int ipcgpu_chamber_set_gas(ipcgpu_ctx* c, const int* isGas, const double* ambient, const double* gamma, const double* fillVolume)
{
    specChanged(c);
    return guarded([&] {
        HipMesh& m = M(c);
        bind(c);
        if (!m.chamber.n()) throw StateError("ipcgpu_chamber_set_gas without chambers: call ipcgpu_set_chambers first");
        needArg(isGas && ambient && gamma, "null argument");
        bool any = false;
        for (int i = 0; i < m.chamber.n(); ++i) any = any || isGas[i] != 0;
        if (any && c->lin->solverType == IPCGPU_SOLVER_PCG) throw UnsupportedError("a gas chamber with the iterative solver (its operator lacks the rank-k term of the gas law)");
        m.setChamberGas(isGas, ambient, gamma, fillVolume, c->stream);
        return IPCGPU_OK;
    });
}
int ipcgpu_chamber_gas_get(ipcgpu_ctx* c, int* isGas, double* ambient, double* gamma, double* fillVolume)
{
    return guarded([&] {
        const HipChamber& h = M(c).chamber;
        for (int i = 0; i < h.n(); ++i) {
            const bool g = h.nGas() && h.gas.isGas[i];
            if (isGas) isGas[i] = g ? 1 : 0;
            if (ambient) ambient[i] = g ? h.gas.ambient[i] : 0.0;
            if (gamma) gamma[i] = g ? h.gas.gamma[i] : 1.0;
            if (fillVolume) fillVolume[i] = g ? h.gas.fillVolume[i] : h.plan.restVolume[i];
        }
        return IPCGPU_OK;
    });
}
int ipcgpu_chamber_gas_state(ipcgpu_ctx* c, double* volume, double* gauge, double* beta)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        const HipChamber& h = c->mesh->chamber;
        const int n = h.n();
        if (!n) return IPCGPU_OK;
        // a constant chamber: its volume from the segmented reduction of ipcgpu_chamber_state, gauge = p_c, beta = 0
        std::vector<double> v((size_t)n, 0.0), st;
        if (volume && h.nGas() < n) {
            DevBuf<double> dv;
            dv.alloc(n);
            launch_chamber_state(o.chamberView(c->mesh->d_x.p), dv.p, nullptr, nullptr, c->stream);
            HIP_CHECK(hipGetLastError());
            dv.download(v.data(), n, c->stream);
        }
        if (h.nGas()) {
            st.resize(4 * (size_t)n);
            launch_chamber_gas_update(o.chamberView(c->mesh->d_x.p), h.gasView(), 0.0, nullptr, false, c->stream);
            HIP_CHECK(hipGetLastError());
            h.d_gasState.download(st.data(), st.size(), c->stream);
        }
        for (int i = 0; i < n; ++i) {
            const bool g = h.nGas() && h.gas.isGas[i];
            if (volume) volume[i] = g ? st[4 * (size_t)i] : v[i];
            if (gauge) gauge[i] = g ? st[4 * (size_t)i + 1] : h.plan.pressure[i];
            if (beta) beta[i] = g ? st[4 * (size_t)i + 2] : 0.0;
        }
        return IPCGPU_OK;
    });
}
int ipcgpu_chamber_volume_gradient(ipcgpu_ctx* c, int chamber, int projectDBC, double* u)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        const HipChamber& h = c->mesh->chamber;
        if (!h.n()) throw StateError("ipcgpu_chamber_volume_gradient without chambers: call ipcgpu_set_chambers first");
        needArg(u != nullptr, "null argument");
        needArg(chamber >= 0 && chamber < h.n(), "chamber index out of range");
        const size_t n3 = 3 * (size_t)c->mesh->nV;
        std::vector<double> sel((size_t)h.n(), 0.0);
        sel[(size_t)chamber] = 1.0;
        DevBuf<double> ds, du;
        ds.upload(sel, c->stream);
        du.alloc(n3);
        launch_chamber_volume_gradient(o.chamberView(c->mesh->d_x.p), ds.p, projectDBC ? 1 : 0, du.p, n3, c->stream);
        HIP_CHECK(hipGetLastError());
        du.download(u, n3, c->stream);
        return IPCGPU_OK;
    });
}
int ipcgpu_chamber_gas_solve(ipcgpu_ctx* c, double coef, const double* rhs, double* x)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        HipLinSysSolver& l = L(c);
        needArg(rhs && x, "null argument");
        need(l.numRows == 3 * c->mesh->nV && l.analyzed(), "ipcgpu_chamber_gas_solve needs the node pattern, analysed and factorised");
        if (l.solverType == IPCGPU_SOLVER_PCG) throw UnsupportedError("ipcgpu_chamber_gas_solve with the iterative solver");
        DevBuf<double> db, dx;
        db.upload(rhs, l.numRows, c->stream);
        dx.alloc(l.numRows);
        const bool ok = l.solve(db.p, dx.p);
        o.chamberGasCorrect(coef, /*projectDBC=*/true, dx.p); // the routine of the stepper (HipOptimizer::computeSearchDir)
        dx.download(x, l.numRows, c->stream);
        return ok ? IPCGPU_OK : IPCGPU_NOT_PD;
    });
}
// ---- Wind and air drag -----------------------------------------------------------------------------------
int ipcgpu_set_aero(ipcgpu_ctx* c, int nSurf, const int* triEnd, const int* tri, const double* cn, const double* ct, const int* oneSided)
{
    // (setCodimBody counts triangles: nSurf == 0 with no surface set is "nothing to remove"; it rebuilds a pattern built before this call)
    return setCodimBody(c, HipOptimizer::CODIM_AERO, nSurf >= 0 && ((triEnd && tri && cn && ct && oneSided) || !nSurf), nSurf,
        [&](HipMesh& m) { m.setAero(nSurf, triEnd, tri, cn, ct, oneSided, c->stream); });
}
int ipcgpu_aero_set_wind(ipcgpu_ctx* c, const double* wind3, double density)
{
    specChanged(c);
    return guarded([&] {
        M(c).setAeroWind(wind3, density);
        return IPCGPU_OK;
    });
}
int ipcgpu_aero_get(ipcgpu_ctx* c, int* counts2, int* triEnd, int* tri, double* cn, double* ct, int* oneSided, double* wind3, double* density)
{
    return guarded([&] {
        const HipAero& h = M(c).aero;
        const AeroPlan& p = h.plan;
        if (counts2) {
            counts2[0] = p.n;
            counts2[1] = p.nTri;
        }
        if (triEnd) std::copy(p.triEnd.begin(), p.triEnd.end(), triEnd);
        if (tri) std::copy(p.tri.begin(), p.tri.end(), tri);
        if (cn) std::copy(p.cn.begin(), p.cn.end(), cn);
        if (ct) std::copy(p.ct.begin(), p.ct.end(), ct);
        if (oneSided) std::copy(p.oneSided.begin(), p.oneSided.end(), oneSided);
        if (wind3) std::copy(h.wind, h.wind + 3, wind3);
        if (density) *density = h.density;
        return IPCGPU_OK;
    });
}
int ipcgpu_aero_state(ipcgpu_ctx* c, double* force, double* lagged, double* total5)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        HipAero& h = c->mesh->aero;
        const size_t n = (size_t)h.nTri();
        if (!n) return IPCGPU_OK;
        if (force || total5) {
            need(o.initialised, "call ipcgpu_opt_init first (it supplies dt)");
            const AeroView v = o.aeroView(c->mesh->d_x.p);
            if (force) h.d_force.alloc(3 * n);
            h.d_statePartial.ensure(5 * (size_t)aero_energy_blocks(v));
            h.d_stateOut.alloc(5);
            launch_aero_state(v, force ? h.d_force.p : nullptr, h.d_statePartial.p, total5 ? h.d_stateOut.p : nullptr, c->stream);
            HIP_CHECK(hipGetLastError());
            if (force) h.d_force.download(force, 3 * n, c->stream);
            if (total5) h.d_stateOut.download(total5, 5, c->stream);
        }
        if (lagged) h.d_lagged.download(lagged, 8 * n, c->stream); // the records the evaluations use now, not those of the current positions
        return IPCGPU_OK;
    });
}
int ipcgpu_aero_energy(ipcgpu_ctx* c, double coef, double* E)
{
    return guarded([&] {
        if (E && !M(c).aero.n()) { // without a surface: nothing, whatever the state
            *E = 0.0;
            return (int)IPCGPU_OK;
        }
        return codimEnergy(c, AERO, coef, E);
    });
}
int ipcgpu_aero_energy_per_elem(ipcgpu_ctx* c, double* perTri)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        const int n = c->mesh->aero.nTri();
        if (!n || !perTri) return IPCGPU_OK;
        need(o.initialised, "call ipcgpu_opt_init first (it supplies dt)");
        DevBuf<double> e;
        e.alloc(n);
        launch_aero_energy_per_elem(o.aeroView(c->mesh->d_x.p), e.p, c->stream);
        HIP_CHECK(hipGetLastError());
        e.download(perTri, n, c->stream);
        return IPCGPU_OK;
    });
}
int ipcgpu_aero_gradient_add(ipcgpu_ctx* c, double coef, int projectDBC, double* g)
{
    return guarded([&] {
        need(!M(c).aero.n() || O(c).initialised, "call ipcgpu_opt_init first (it supplies dt)");
        return codimGradientAdd(c, AERO, coef, projectDBC, g);
    });
}
int ipcgpu_aero_hessian_add(ipcgpu_ctx* c, double coef, int projectDBC)
{
    specChanged(c);
    return guarded([&] {
        need(!M(c).aero.n() || O(c).initialised, "call ipcgpu_opt_init first (it supplies dt)");
        return codimHessianAdd(c, AERO, coef, projectDBC, AERO_MISS);
    });
}
// ---- Fibre reinforcement (fiber_kernels.h; the reference has no counterpart) ---------------------------------------------------------------------
int ipcgpu_set_fibers(ipcgpu_ctx* c, int tetBegin, int tetEnd, const double* dir, int dirPerElement, double k, int law, double k2, int tensionOnly, int group)
{
    specChanged(c);
    return guarded([&] {
        HipMesh& m = M(c);
        bind(c);
        if (c->worldSize > 1) throw UnsupportedError("fibres on a sharded context");
        m.setFibers(tetBegin, tetEnd, dir, dirPerElement != 0, k, law, k2, tensionOnly != 0, group, c->stream);
        return IPCGPU_OK;
    });
}
int ipcgpu_fiber_set_activation(ipcgpu_ctx* c, int group, double act)
{
    specChanged(c);
    return guarded([&] {
        HipMesh& m = M(c);
        bind(c);
        m.setFiberActivation(group, act, c->stream);
        return IPCGPU_OK;
    });
}
int ipcgpu_fiber_get(ipcgpu_ctx* c, int* nFibred, double* k, double* k2, int* law, int* tensionOnly, int* group, double* dir, double* act)
{
    return guarded([&] {
        const HipMesh& m = M(c);
        const FiberPlan& p = m.fiber.plan;
        const size_t nT = (size_t)m.nT;
        const bool set = p.nT > 0;
        if (nFibred) *nFibred = p.nF;
        for (size_t t = 0; t < nT; ++t) {
            if (k) k[t] = set ? p.k[t] : 0.0;
            if (k2) k2[t] = set ? p.k2[t] : 0.0;
            if (law) law[t] = set && (p.flags[t] & FIBER_FLAG_EXP) ? FIBER_LAW_EXP : FIBER_LAW_SPRING;
            if (tensionOnly) tensionOnly[t] = set && p.flags[t] != 0 ? 1 : 0; // (the exp law is always tension only)
            if (group) group[t] = set ? p.group[t] : 0;
            if (dir)
                for (int r = 0; r < 3; ++r) dir[3 * t + r] = set ? p.dir[r * nT + t] : 0.0;
        }
        if (act)
            for (int g = 0; g < FIBER_MAX_GROUPS; ++g) act[g] = set ? p.act[g] : 0.0;
        return IPCGPU_OK;
    });
}
int ipcgpu_fiber_energy(ipcgpu_ctx* c, double coef, double* E)
{
    return guarded([&] { return codimEnergy(c, FIBER, coef, E); });
}
int ipcgpu_fiber_energy_per_elem(ipcgpu_ctx* c, double* perTet)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        if (!perTet) return IPCGPU_OK;
        const HipFiber& f = c->mesh->fiber;
        std::fill(perTet, perTet + c->mesh->nT, 0.0);
        const int n = f.n();
        if (!n) return IPCGPU_OK;
        DevBuf<double> e;
        e.alloc(n);
        launch_fiber_energy_per_elem(o.fiberView(c->mesh->d_x.p), e.p, c->stream);
        HIP_CHECK(hipGetLastError());
        std::vector<double> h(n);
        e.download(h.data(), n, c->stream);
        for (int i = 0; i < n; ++i) perTet[f.plan.fibTet[i]] = h[i];
        return IPCGPU_OK;
    });
}
int ipcgpu_fiber_gradient_add(ipcgpu_ctx* c, double coef, int projectDBC, double* g)
{
    return guarded([&] { return codimGradientAdd(c, FIBER, coef, projectDBC, g); });
}
int ipcgpu_fiber_hessian_add(ipcgpu_ctx* c, double coef, int projectDBC)
{
    specChanged(c);
    return guarded([&] { return codimHessianAdd(c, FIBER, coef, projectDBC, FIBER_MISS); });
}
int ipcgpu_fiber_state(ipcgpu_ctx* c, double* perElem, double* totals3)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        HipMesh& m = *c->mesh;
        HipFiber& f = m.fiber;
        const size_t nT = (size_t)m.nT, n = (size_t)f.n();
        if (perElem) // an element without fibres: stretch 1, no tension, no direction
            for (size_t t = 0; t < nT; ++t) {
                perElem[t] = 1.0;
                for (int q = 1; q < FIBER_STATE_COLS; ++q) perElem[q * nT + t] = 0.0;
            }
        if (totals3) {
            totals3[0] = totals3[1] = 1.0;
            totals3[2] = 0.0;
        }
        if (!n || (!perElem && !totals3)) return IPCGPU_OK;
        const FiberView v = o.fiberView(m.d_x.p);
        if (perElem) f.d_state.ensure(FIBER_STATE_COLS * n);
        f.d_partial.ensure(3 * (size_t)fiber_energy_blocks(v));
        f.d_totals.ensure(3);
        launch_fiber_state(v, m.d_vol.p, perElem ? f.d_state.p : nullptr, f.d_partial.p, totals3 ? f.d_totals.p : nullptr, c->stream);
        HIP_CHECK(hipGetLastError());
        if (perElem) {
            std::vector<double> h(FIBER_STATE_COLS * n);
            f.d_state.download(h.data(), h.size(), c->stream);
            for (size_t i = 0; i < n; ++i)
                for (int q = 0; q < FIBER_STATE_COLS; ++q) perElem[q * nT + (size_t)f.plan.fibTet[i]] = h[q * n + i];
        }
        if (totals3) f.d_totals.download(totals3, 3, c->stream);
        return IPCGPU_OK;
    });
}
// ---- Plastic flow (plastic_kernels.h; the reference has no counterpart) -------------------------------------------------------------------------
int ipcgpu_set_plasticity(ipcgpu_ctx* c, int tetBegin, int tetEnd, double yield, double creep, double harden)
{
    specChanged(c);
    return guarded([&] {
        HipMesh& m = M(c);
        bind(c);
        if (c->worldSize > 1) throw UnsupportedError("plasticity on a sharded context");
        m.setPlasticity(tetBegin, tetEnd, yield, creep, harden, c->stream);
        return IPCGPU_OK;
    });
}
int ipcgpu_plastic_get(ipcgpu_ctx* c, double* yield, double* creep, double* harden, double* alpha, double* restTriInv0)
{
    return guarded([&] {
        HipMesh& m = M(c);
        bind(c);
        const HipPlastic& h = m.plastic;
        const size_t nT = (size_t)m.nT;
        if (!h.allocated()) { // never set: every element elastic, no history, A0 is the mesh's restTriInv
            for (size_t t = 0; t < nT; ++t) {
                if (yield) yield[t] = INFINITY;
                if (creep) creep[t] = INFINITY;
                if (harden) harden[t] = 0.0;
                if (alpha) alpha[t] = 0.0;
            }
            if (restTriInv0)
                for (size_t t = 0; t < nT; ++t)
                    for (int k = 0; k < 9; ++k) restTriInv0[9 * t + k] = m.restTriInv[k * nT + t];
            return IPCGPU_OK;
        }
        if (yield) std::memcpy(yield, h.plan.yield.data(), sizeof(double) * nT);
        if (creep) std::memcpy(creep, h.plan.creep.data(), sizeof(double) * nT);
        if (harden) std::memcpy(harden, h.plan.harden.data(), sizeof(double) * nT);
        if (alpha) h.d_alpha.download(alpha, nT, c->stream);
        if (restTriInv0) {
            std::vector<double> soa(9 * nT);
            h.d_A0.download(soa.data(), soa.size(), c->stream);
            for (size_t t = 0; t < nT; ++t)
                for (int k = 0; k < 9; ++k) restTriInv0[9 * t + k] = soa[k * nT + t];
        }
        return IPCGPU_OK;
    });
}
int ipcgpu_plastic_update(ipcgpu_ctx* c, double dt, int* nYielded, int* nSkipped)
{
    specChanged(c);
    return guarded([&] {
        HipMesh& m = M(c);
        bind(c);
        needArg(dt > 0.0 && std::isfinite(dt), "plastic_update: the time step must be positive and finite");
        int cnt[PC_COUNT] = { 0, 0 };
        if (m.plastic.on()) {
            c->opt->plasticFlow(m.d_x.p, dt);
            HIP_CHECK(hipGetLastError());
            m.plastic.d_count.download(cnt, PC_COUNT, c->stream);
        }
        if (nYielded) *nYielded = cnt[PC_YIELDED];
        if (nSkipped) *nSkipped = cnt[PC_SKIPPED];
        return IPCGPU_OK;
    });
}
int ipcgpu_plastic_state(ipcgpu_ctx* c, double* perElem, double* totals4)
{
    return guarded([&] {
        HipMesh& m = M(c);
        bind(c);
        const size_t nT = (size_t)m.nT;
        HipPlastic& h = m.plastic;
        if (totals4) totals4[0] = totals4[1] = totals4[2] = totals4[3] = 0.0;
        if (!h.allocated()) {
            if (perElem)
                for (size_t t = 0; t < nT; ++t) {
                    perElem[t] = NAN; // (n is not evaluated without the state arrays)
                    perElem[nT + t] = INFINITY;
                    perElem[2 * nT + t] = 0.0;
                }
            return IPCGPU_OK;
        }
        if (!perElem && !totals4) return IPCGPU_OK;
        const PlasticView v = c->opt->plasticView(m.d_x.p, 1.0);
        if (perElem) h.d_state.ensure(3 * nT);
        h.d_partial.ensure(2 * (size_t)plastic_state_blocks(v));
        launch_plastic_state(v, perElem ? h.d_state.p : nullptr, h.d_partial.p, totals4 ? h.d_totals.p : nullptr, c->stream);
        HIP_CHECK(hipGetLastError());
        if (perElem) h.d_state.download(perElem, 3 * nT, c->stream);
        if (totals4) {
            int cnt[PC_COUNT];
            double tot[PT_COUNT];
            h.d_count.download(cnt, PC_COUNT, c->stream);
            h.d_totals.download(tot, PT_COUNT, c->stream);
            totals4[0] = cnt[PC_YIELDED];
            totals4[1] = cnt[PC_SKIPPED];
            totals4[2] = tot[PT_MAX_ALPHA];
            totals4[3] = tot[PT_VOL_ALPHA];
        }
        return IPCGPU_OK;
    });
}
int ipcgpu_plastic_set_state(ipcgpu_ctx* c, const double* restTriInv, const double* alpha)
{
    specChanged(c);
    return guarded([&] {
        HipMesh& m = M(c);
        bind(c);
        need(m.plastic.allocated(), "call ipcgpu_set_plasticity first");
        const size_t nT = (size_t)m.nT;
        if (alpha)
            for (size_t t = 0; t < nT; ++t) needArg(alpha[t] >= 0.0 && std::isfinite(alpha[t]), "plastic_set_state: the accumulated plastic strain must be finite and not negative");
        if (restTriInv) {
            std::vector<double> soa(9 * nT);
            for (size_t t = 0; t < nT; ++t)
                for (int k = 0; k < 9; ++k) {
                    needArg(std::isfinite(restTriInv[9 * t + k]), "plastic_set_state: restTriInv is not finite");
                    soa[k * nT + t] = restTriInv[9 * t + k];
                }
            HIP_CHECK(hipMemcpyAsync(m.d_A.p, soa.data(), soa.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
            HIP_CHECK(hipStreamSynchronize(c->stream)); // (soa leaves scope)
        }
        if (alpha) HIP_CHECK(hipMemcpyAsync(m.plastic.d_alpha.p, alpha, nT * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIP_CHECK(hipStreamSynchronize(c->stream));
        return IPCGPU_OK;
    });
}
int ipcgpu_plastic_reset(ipcgpu_ctx* c)
{
    specChanged(c);
    return guarded([&] {
        HipMesh& m = M(c);
        bind(c);
        if (!m.plastic.allocated()) return IPCGPU_OK; // no history to forget
        HIP_CHECK(hipMemcpyAsync(m.d_A.p, m.plastic.d_A0.p, 9 * (size_t)m.nT * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        m.plastic.d_alpha.zero(c->stream);
        m.plastic.d_count.zero(c->stream);
        HIP_CHECK(hipStreamSynchronize(c->stream));
        return IPCGPU_OK;
    });
}
int ipcgpu_set_obstacle_nodes(ipcgpu_ctx* c, int n, const int* ids, int only)
{
    specChanged(c);
    return guarded([&] {
        bind(c);
        HipContact& k = CT(c);
        need(k.surfaceSet, "call ipcgpu_set_surface first");
        needArg(n >= 0 && (ids || !n), "bad obstacle node list");
        k.setObstacle(M(c).nV, n, ids, only != 0);
        return IPCGPU_OK;
    });
}
int ipcgpu_set_contact_groups(ipcgpu_ctx* c, int nComp, const int* group, int nGroups, const unsigned char* collide, const double* fricScale)
{
    specChanged(c);
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        if (c->worldSize > 1) throw UnsupportedError("contact groups on a sharded context (not implemented)");
        needArg(nComp >= 0, "contact groups: negative component count");
        const int nV = c->mesh->nV;
        if (nComp == 0) { // back to the default: one group that collides with itself, all scales 1
            if (c->contact) c->contact->setGroups(nV, {}, {}, 1);
            return IPCGPU_OK;
        }
        std::vector<int> ends = o.compNodeEnd; // no table (or one of another mesh): the whole mesh, as the reports have it
        if (ends.empty() || ends.back() != nV) ends.assign(1, nV);
        std::vector<int> words;
        std::vector<double> scale16;
        std::string err;
        if (!buildContactGroupWords(nV, (int)ends.size(), ends.data(), nComp, group, nGroups, collide, fricScale, words, scale16, err)) throw ArgError(err);
        CT(c).setGroups(nV, words, scale16, nGroups);
        return IPCGPU_OK;
    });
}
int ipcgpu_get_contact_groups(ipcgpu_ctx* c, int* nGroups, int* nodeWord)
{
    return guarded([&] {
        HipMesh& m = M(c);
        if (c->worldSize > 1) throw UnsupportedError("contact groups on a sharded context (not implemented)");
        const bool on = c->contact && c->contact->hasGroups;
        if (nGroups) *nGroups = on ? c->contact->nGroups : 1;
        for (int v = 0; nodeWord && v < m.nV; ++v) nodeWord[v] = on ? c->contact->groupWord[v] : (int)CONTACT_GROUP_DEFAULT_WORD;
        return IPCGPU_OK;
    });
}
int ipcgpu_contact_get(ipcgpu_ctx* c, int* a4, int* p4, int* pe2, int* cs2)
{
    return guarded([&] {
        bind(c);
        HipContact& k = CT(c);
        k.syncHost();
        for (size_t i = 0; a4 && i < k.active.size(); ++i)
            for (int j = 0; j < 4; ++j) a4[4 * i + j] = k.active[i][j];
        for (size_t i = 0; i < k.para.size(); ++i) {
            for (int j = 0; p4 && j < 4; ++j) p4[4 * i + j] = k.para[i][j];
            if (pe2) {
                pe2[2 * i] = k.paraEIEJ[i][0];
                pe2[2 * i + 1] = k.paraEIEJ[i][1];
            }
        }
        for (size_t i = 0; cs2 && i < k.csPTEE.size(); ++i) {
            cs2[2 * i] = k.csPTEE[i][0];
            cs2[2 * i + 1] = k.csPTEE[i][1];
        }
        return IPCGPU_OK;
    });
}
int ipcgpu_contact_set(ipcgpu_ctx* c, int nA, const int* a4, int nP, const int* p4, const int* pe2)
{
    return guarded([&] {
        bind(c);
        HipContact& k = CT(c);
        need(k.surfaceSet, "call ipcgpu_set_surface first");
        needArg(nA >= 0 && nP >= 0 && (a4 || !nA) && ((p4 && pe2) || !nP), "bad constraint set");
        k.setSets(nA, a4, nP, p4, pe2);
        return IPCGPU_OK;
    });
}
int ipcgpu_contact_counts(ipcgpu_ctx* c, int* counts3)
{
    return guarded([&] {
        needArg(c != nullptr && counts3 != nullptr, "null argument");
        HipContact& k = CT(c);
        counts3[0] = k.nActive();
        counts3[1] = k.nPara();
        counts3[2] = k.nCand();
        return IPCGPU_OK;
    });
}
int ipcgpu_contact_energy(ipcgpu_ctx* c, double dHat, double kappa, double* E)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(o.initialised, "call ipcgpu_opt_init first");
        *E = CT(c).energy(c->mesh->d_x.p, dHat, kappa, o.d_partial, o.slot(S_CONTACT_E));
        return IPCGPU_OK;
    });
}
// every node a kernel will read, checked per stencil kind exactly as the device decodes the tuple (hip_contact.hip decode()): c[0] >= 0: an edge-edge tuple, four
// nodes; else -c[0] - 1 and c[1] are nodes, c[2] is one unless negative (point-point), c[3] is one when c[2] and c[3] are non-negative (point-triangle); a negative
// c[3] behind a node c[2] is the multiplicity of a point-edge tuple
static void checkTuples(ipcgpu_ctx* c, int n, const int* t)
{
    const int nV = c->mesh->nV;
    auto node = [&](int v) { return v >= 0 && v < nV; };
    for (int i = 0; i < n; ++i) {
        const int* q = t + 4 * (size_t)i;
        bool ok;
        if (q[0] >= 0) ok = node(q[0]) && node(q[1]) && node(q[2]) && node(q[3]);
        else ok = node(-q[0] - 1) && node(q[1]) && (q[2] < 0 || (node(q[2]) && (q[3] < 0 || node(q[3]))));
        needArg(ok, "MMCVID node id out of range");
    }
}
int ipcgpu_contact_evaluate(ipcgpu_ctx* c, int n, const int* mmcvid_4n, double* val_n)
{
    return guarded([&] {
        needArg(c != nullptr, "null context");
        bind(c);
        needArg(n >= 0 && (n == 0 || (mmcvid_4n && val_n)), "null argument");
        checkTuples(c, n, mmcvid_4n);
        CT(c).evaluateTuples(c->mesh->d_x.p, n, mmcvid_4n, val_n);
        return IPCGPU_OK;
    });
}
int ipcgpu_contact_jt_multiply(ipcgpu_ctx* c, int n, const int* mmcvid_4n, const double* input_n, double coef, double* out_3nV_inout)
{
    return guarded([&] {
        needArg(c != nullptr, "null context");
        bind(c);
        needArg(n >= 0 && out_3nV_inout && (n == 0 || (mmcvid_4n && input_n)), "null argument");
        checkTuples(c, n, mmcvid_4n);
        CT(c).jtMultiplyTuples(c->mesh->d_x.p, c->mesh->nV, n, mmcvid_4n, input_n, coef, out_3nV_inout);
        return IPCGPU_OK;
    });
}
int ipcgpu_contact_gradient_add(ipcgpu_ctx* c, double dHat, double kappa, int projectDBC, double* g)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(o.initialised, "call ipcgpu_opt_init first");
        const size_t n3 = 3 * (size_t)c->mesh->nV;
        HIP_CHECK(hipMemcpyAsync(o.d_gradient.p, g, n3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
        CT(c).gradientAdd(c->mesh->d_x.p, c->mesh->d_dbc.p, c->mesh->nV, dHat, kappa, projectDBC, o.d_gradient.p);
        o.d_gradient.download(g, n3, c->stream);
        return IPCGPU_OK;
    });
}
int ipcgpu_contact_report(ipcgpu_ctx* c, double dHat, double kappa, const double* Vt, double eps2, double coef, int capacity, int* nRows, int* rowsI,
    double* rowsD)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(c->contact && c->contact->surfaceSet, "call ipcgpu_set_surface first");
        if (c->worldSize > 1) throw UnsupportedError("contact report on a sharded context (multi-rank reports are not implemented)");
        needArg(nRows != nullptr && capacity >= 0 && (capacity == 0 || (rowsI && rowsD)), "contact report: null output");
        needArg(dHat > 0.0 && (!Vt || coef <= 0.0 || eps2 > 0.0), "contact report: dHat and eps2 must be positive");
        const int nV = c->mesh->nV;
        std::vector<int> ends = o.compNodeEnd; // no table (or one of another mesh): the whole mesh, as the system report has it
        if (ends.empty() || ends.back() != nV) ends.assign(1, nV);
        std::vector<HipContact::ReportPlane> planes;
        for (const auto& h : o.planes) planes.push_back({ { h->n[0], h->n[1], h->n[2] }, h->D, h->d_set.p, (int)h->set.size() });
        *nRows = c->contact->contactReport(c->mesh->d_x.p, nV, ends, planes, dHat, kappa, Vt, eps2, coef, capacity, rowsI, rowsD);
        needArg(capacity >= *nRows, "contact report: capacity is smaller than the number of rows (*nRows is set)");
        return IPCGPU_OK;
    });
}
int ipcgpu_contact_hessian_add(ipcgpu_ctx* c, double dHat, double kappa, int projectDBC)
{
    return guarded([&] {
        M(c);
        bind(c);
        need(c->lin->numRows == 3 * c->mesh->nV, "call ipcgpu_linsys_set_pattern first");
        CT(c).hessianAdd(c->mesh->d_x.p, c->mesh->d_dbc.p, *c->lin, dHat, kappa, projectDBC, c->lin->d_a.p);
        return IPCGPU_OK;
    });
}
int ipcgpu_contact_connectivity(ipcgpu_ctx* c, int cap, int* pairs, int* n)
{
    return guarded([&] {
        std::vector<std::pair<int, int>> p;
        CT(c).connectivity(p);
        if (n) *n = (int)p.size();
        for (size_t i = 0; pairs && i < p.size() && (int)i < cap; ++i) {
            pairs[2 * i] = p[i].first;
            pairs[2 * i + 1] = p[i].second;
        }
        return IPCGPU_OK;
    });
}

int ipcgpu_ccd_partial(ipcgpu_ctx* c, const double* p, double slackness, double* step, int* pair2)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(o.initialised, "call ipcgpu_opt_init first");
        needArg(p && step && slackness > 0 && slackness < 1, "bad ccd argument");
        HIP_CHECK(hipMemcpyAsync(o.d_searchDir.p, p, 3 * (size_t)c->mesh->nV * sizeof(double), hipMemcpyHostToDevice, c->stream));
        *step = CT(c).ccdPartial(c->mesh->d_x.p, o.d_searchDir.p, slackness, *step, pair2);
        return IPCGPU_OK;
    });
}
int ipcgpu_ccd_full(ipcgpu_ctx* c, const double* p, double slackness, double* step, int* pair2, int* nCand)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(o.initialised, "call ipcgpu_opt_init first");
        needArg(p && step && slackness > 0 && slackness < 1, "bad ccd argument");
        HIP_CHECK(hipMemcpyAsync(o.d_searchDir.p, p, 3 * (size_t)c->mesh->nV * sizeof(double), hipMemcpyHostToDevice, c->stream));
        *step = CT(c).ccdFull(*c->mesh, c->mesh->d_x.p, o.d_searchDir.p, c->mesh->d_dbc.p, slackness, *step, pair2, nCand);
        return IPCGPU_OK;
    });
}
int ipcgpu_ccd_full_reference(ipcgpu_ctx* c, const double* p, double slackness, double* step, double* alphaCapped, int* arg3, int* nCand)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(o.initialised, "call ipcgpu_opt_init first");
        needArg(p && step && slackness > 0 && slackness < 1, "bad ccd argument");
        HIP_CHECK(hipMemcpyAsync(o.d_searchDir.p, p, 3 * (size_t)c->mesh->nV * sizeof(double), hipMemcpyHostToDevice, c->stream));
        *step = CT(c).ccdFullReference(*c->mesh, c->mesh->d_x.p, o.d_searchDir.p, c->mesh->d_dbc.p, slackness, *step, alphaCapped, arg3, nCand);
        return IPCGPU_OK;
    });
}
int ipcgpu_set_ccd_mode(ipcgpu_ctx* c, int mode)
{
    specChanged(c);
    return guarded([&] {
        needArg(mode == 0 || mode == 1, "ccd mode is 0 (swept boxes, PT / EE pairs) or 1 (the reference's sweep)");
        CT(c).ccdMode = mode;
        return IPCGPU_OK;
    });
}
int ipcgpu_is_intersected(ipcgpu_ctx* c, int* flag)
{
    return guarded([&] {
        M(c);
        bind(c);
        *flag = CT(c).isIntersected(*c->mesh, c->mesh->d_x.p, c->mesh->d_dbc.p) ? 1 : 0;
        return IPCGPU_OK;
    });
}

// ---- Optimizer building blocks ----------------------------------------------------------------------
int ipcgpu_assemble_newton(ipcgpu_ctx* c, double dtSq, int projectDBC, double* grad)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(o.initialised, "call ipcgpu_opt_init first");
        const double keep = o.dtSq;
        o.dtSq = dtSq;
        o.computePrecondMtr(projectDBC != 0, grad != nullptr);
        o.dtSq = keep;
        if (grad) o.d_gradient.download(grad, 3 * (size_t)c->mesh->nV, c->stream);
        else HIP_CHECK(hipStreamSynchronize(c->stream));
        if (o.selfCollision && o.contact) o.contact->takeHessianError(); // (the stepper leaves the barrier Hessian's "pair outside the pattern" flag to its next synchronisation: here)
        return IPCGPU_OK;
    });
}
int ipcgpu_incremental_potential(ipcgpu_ctx* c, double dtSq, double* E)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(o.initialised, "call ipcgpu_opt_init first");
        const double keep = o.dtSq;
        o.dtSq = dtSq;
        *E = o.computeEnergyVal();
        o.dtSq = keep;
        return IPCGPU_OK;
    });
}
int ipcgpu_gradient(ipcgpu_ctx* c, double dtSq, int projectDBC, double* grad)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(o.initialised, "call ipcgpu_opt_init first");
        const double keep = o.dtSq;
        o.dtSq = dtSq;
        o.computeGradient(projectDBC != 0);
        o.dtSq = keep;
        o.d_gradient.download(grad, 3 * (size_t)c->mesh->nV, c->stream);
        return IPCGPU_OK;
    });
}

// ---- Optimizer --------------------------------------------------------------------------------------
int ipcgpu_opt_init(ipcgpu_ctx* c, double dt, int withGravity)
{
    specChanged(c);
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        needArg(dt > 0, "dt must be positive");
        o.rank = c->rank;
        o.worldSize = c->worldSize;
        o.init(dt, withGravity != 0);
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_set_rel_tol(ipcgpu_ctx* c, double tol)
{
    specChanged(c);
    return guarded([&] {
        needArg(tol > 0, "relTol must be positive"); // Optimizer.cpp:392
        O(c).setRelGL2Tol(tol);
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_set_twist(ipcgpu_ctx* c, int nL, const int* l, int nR, const int* r, double angVel)
{
    specChanged(c);
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(o.initialised, "call ipcgpu_opt_init first");
        for (int i = 0; i < nL; ++i) needArg(l[i] >= 0 && l[i] < c->mesh->nV, "handle id out of range");
        for (int i = 0; i < nR; ++i) needArg(r[i] >= 0 && r[i] < c->mesh->nV, "handle id out of range");
        o.setTwist(nL, l, nR, r, angVel);
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_enable_self_collision(ipcgpu_ctx* c, double dHatEps)
{
    specChanged(c);
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(o.initialised, "call ipcgpu_opt_init first");
        needArg(dHatEps > 0, "dHatEps must be positive");
        o.enableSelfCollision(&CT(c), dHatEps);
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_set_pattern_lookahead(ipcgpu_ctx* c, double pad)
{
    specChanged(c);
    return guarded([&] {
        HipOptimizer& o = O(c);
        needArg(pad >= 0.0 && pad <= 100.0, "pattern look-ahead: 0 <= pad <= 100 (in units of dHat)");
        o.patternPad = pad;
        return IPCGPU_OK;
    });
}
// ---- what the half-space and the round collider entry points share: one body each, the caller supplies the obstacle ------------------------------------
static int colliderBuild(ipcgpu_ctx* c, HipVertexCollider& h, double dHat, int cap, int* verts, int* n)
{
    bind(c);
    const int cnt = h.build(CT(c).nSVI, CT(c).d_SVI.p, c->mesh->d_x.p, c->mesh->d_dbc.p, dHat);
    if (n) *n = cnt;
    needArg(!verts || cap >= cnt, "verts buffer too small");
    if (verts) std::memcpy(verts, h.set.data(), sizeof(int) * cnt);
    return IPCGPU_OK;
}
static int colliderSet(ipcgpu_ctx* c, HipVertexCollider& h, int n, const int* verts)
{
    bind(c);
    needArg(n >= 0 && (verts || !n), "bad vertex list");
    for (int i = 0; i < n; ++i) needArg(verts[i] >= 0 && verts[i] < c->mesh->nV, "vertex id out of range");
    h.setSet(n, verts);
    return IPCGPU_OK;
}
static int colliderEnergy(ipcgpu_ctx* c, HipVertexCollider& h, double dHat, double kappa, double* E)
{
    bind(c);
    needArg(E != nullptr, "null result");
    *E = h.energy(c->mesh->d_x.p, dHat, kappa);
    return IPCGPU_OK;
}
static int colliderGradientAdd(ipcgpu_ctx* c, HipVertexCollider& h, double dHat, double kappa, double* g)
{
    HipOptimizer& o = O(c);
    bind(c);
    needArg(g != nullptr, "null gradient");
    const size_t n3 = 3 * (size_t)c->mesh->nV;
    HIP_CHECK(hipMemcpyAsync(o.d_gradient.p, g, n3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    h.gradientAdd(c->mesh->d_x.p, dHat, kappa, o.d_gradient.p);
    o.d_gradient.download(g, n3, c->stream);
    return IPCGPU_OK;
}
static int colliderHessianAdd(ipcgpu_ctx* c, HipVertexCollider& h, double dHat, double kappa, int projectDBC)
{
    bind(c);
    need(c->lin->numRows == 3 * c->mesh->nV, "call ipcgpu_linsys_set_pattern first");
    h.hessianAdd(c->mesh->d_x.p, c->mesh->d_dbc.p, c->lin->d_rowBase.p, c->lin->d_rowLen.p, dHat, kappa, projectDBC, c->lin->d_a.p);
    HIP_CHECK(hipStreamSynchronize(c->stream));
    return IPCGPU_OK;
}
// (the caller has announced the change with specChanged)
static int colliderMove(ipcgpu_ctx* c, HipVertexCollider& h, const double* delta3, double slackness, double* stepSizeLeft, const char* bad)
{
    bind(c);
    needArg(delta3 && slackness > 0.0 && slackness <= 1.0, bad);
    for (int k = 0; k < 3; ++k) needArg(std::isfinite(delta3[k]), bad);
    const double left = h.move(CT(c).nSVI, CT(c).d_SVI.p, c->mesh->d_x.p, delta3, slackness);
    if (stepSizeLeft) *stepSizeLeft = left;
    return IPCGPU_OK;
}
static int colliderStepBound(ipcgpu_ctx* c, HipVertexCollider& h, const double* p, double slackness, double* step)
{
    HipOptimizer& o = O(c);
    bind(c);
    needArg(p && step && slackness > 0 && slackness <= 1, "bad step-bound argument");
    HIP_CHECK(hipMemcpyAsync(o.d_searchDir.p, p, 3 * (size_t)c->mesh->nV * sizeof(double), hipMemcpyHostToDevice, c->stream));
    *step = h.stepBound(CT(c).nSVI, CT(c).d_SVI.p, c->mesh->d_x.p, c->mesh->d_dbc.p, o.d_searchDir.p, slackness, *step);
    return IPCGPU_OK;
}
int ipcgpu_opt_add_half_space(ipcgpu_ctx* c, const double* origin, const double* normal, double dHatEps, int* id)
{
    specChanged(c);
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(o.initialised, "call ipcgpu_opt_init first");
        needArg(origin && normal && dHatEps > 0, "bad half-space argument");
        const int k = o.addHalfSpace(&CT(c), origin, normal, dHatEps);
        if (id) *id = k;
        return IPCGPU_OK;
    });
}
static HipHalfSpace& HS(ipcgpu_ctx* c, int id)
{
    HipOptimizer& o = O(c);
    needArg(id >= 0 && id < (int)o.planes.size(), "half-space index out of range");
    return *o.planes[id];
}
int ipcgpu_halfspace_build(ipcgpu_ctx* c, int id, double dHat, int cap, int* verts, int* n)
{
    return guarded([&] { return colliderBuild(c, HS(c, id), dHat, cap, verts, n); });
}
int ipcgpu_halfspace_set(ipcgpu_ctx* c, int id, int n, const int* verts)
{
    return guarded([&] { return colliderSet(c, HS(c, id), n, verts); });
}
int ipcgpu_halfspace_energy(ipcgpu_ctx* c, int id, double dHat, double kappa, double* E)
{
    return guarded([&] { return colliderEnergy(c, HS(c, id), dHat, kappa, E); });
}
int ipcgpu_halfspace_gradient_add(ipcgpu_ctx* c, int id, double dHat, double kappa, double* g)
{
    return guarded([&] { return colliderGradientAdd(c, HS(c, id), dHat, kappa, g); });
}
int ipcgpu_halfspace_hessian_add(ipcgpu_ctx* c, int id, double dHat, double kappa, int projectDBC)
{
    return guarded([&] { return colliderHessianAdd(c, HS(c, id), dHat, kappa, projectDBC); });
}
int ipcgpu_halfspace_move(ipcgpu_ctx* c, int id, const double* delta3, double slackness, double* stepSizeLeft)
{
    specChanged(c);
    return guarded([&] { return colliderMove(c, HS(c, id), delta3, slackness, stepSizeLeft, "bad half-space move"); });
}
int ipcgpu_halfspace_step_bound(ipcgpu_ctx* c, int id, const double* p, double slackness, double* step)
{
    return guarded([&] { return colliderStepBound(c, HS(c, id), p, slackness, step); });
}
// ---- round colliders (round_collider_kernels.h): the half-space's list through the same bodies, plus the friction pieces and the state query ---------------------------------------
int ipcgpu_opt_add_round_collider(ipcgpu_ctx* c, const double* p0, const double* p1, double R, int hollow, double dHatEps, int* id)
{
    specChanged(c);
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(o.initialised, "call ipcgpu_opt_init first");
        needArg(p0 && p1 && dHatEps > 0, "bad round-collider argument");
        const int k = o.addRoundCollider(&CT(c), p0, p1, R, hollow, dHatEps);
        if (id) *id = k;
        return IPCGPU_OK;
    });
}
static HipRoundCollider& RC(ipcgpu_ctx* c, int id)
{
    HipOptimizer& o = O(c);
    needArg(id >= 0 && id < (int)o.rounds.size(), "round-collider index out of range");
    return *o.rounds[id];
}
int ipcgpu_round_build(ipcgpu_ctx* c, int id, double dHat, int cap, int* verts, int* n)
{
    return guarded([&] { return colliderBuild(c, RC(c, id), dHat, cap, verts, n); });
}
int ipcgpu_round_set(ipcgpu_ctx* c, int id, int n, const int* verts)
{
    return guarded([&] { return colliderSet(c, RC(c, id), n, verts); });
}
int ipcgpu_round_energy(ipcgpu_ctx* c, int id, double dHat, double kappa, double* E)
{
    return guarded([&] { return colliderEnergy(c, RC(c, id), dHat, kappa, E); });
}
int ipcgpu_round_gradient_add(ipcgpu_ctx* c, int id, double dHat, double kappa, double* g)
{
    return guarded([&] { return colliderGradientAdd(c, RC(c, id), dHat, kappa, g); });
}
int ipcgpu_round_hessian_add(ipcgpu_ctx* c, int id, double dHat, double kappa, int projectDBC)
{
    return guarded([&] { return colliderHessianAdd(c, RC(c, id), dHat, kappa, projectDBC); });
}
int ipcgpu_round_move(ipcgpu_ctx* c, int id, const double* delta3, double slackness, double* stepSizeLeft)
{
    specChanged(c);
    return guarded([&] { return colliderMove(c, RC(c, id), delta3, slackness, stepSizeLeft, "bad round-collider move"); });
}
int ipcgpu_round_step_bound(ipcgpu_ctx* c, int id, const double* p, double slackness, double* step)
{
    return guarded([&] { return colliderStepBound(c, RC(c, id), p, slackness, step); });
}
int ipcgpu_round_get(ipcgpu_ctx* c, int id, double* p0, double* p1, double* R, int* hollow)
{
    return guarded([&] {
        const RoundShape& s = RC(c, id).shape;
        for (int k = 0; k < 3; ++k) {
            if (p0) p0[k] = s.p0[k];
            if (p1) p1[k] = s.p1[k];
        }
        if (R) *R = s.R;
        if (hollow) *hollow = s.side < 0.0 ? 1 : 0;
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_set_round_collider_friction(ipcgpu_ctx* c, int id, double mu)
{
    specChanged(c);
    return guarded([&] {
        needArg(mu >= 0.0, "negative friction coefficient");
        RC(c, id).friction = mu;
        return IPCGPU_OK;
    });
}
int ipcgpu_round_lag_update(ipcgpu_ctx* c, int id, double dHat, double kappa, int* nLagged)
{
    return guarded([&] {
        HipRoundCollider& h = RC(c, id);
        bind(c);
        h.lagUpdate(c->mesh->d_x.p, dHat, kappa);
        HIP_CHECK(hipStreamSynchronize(c->stream));
        if (nLagged) *nLagged = (int)h.lagSet.size();
        return IPCGPU_OK;
    });
}
// x^t of the friction pieces: the caller's Vt in d_x0, as ipcgpu_friction_energy takes it
static const double* roundXt(ipcgpu_ctx* c, const double* Vt)
{
    HipOptimizer& o = O(c);
    needArg(Vt != nullptr, "null Vt");
    HIP_CHECK(hipMemcpyAsync(o.d_x0.p, Vt, 3 * (size_t)c->mesh->nV * sizeof(double), hipMemcpyHostToDevice, c->stream));
    return o.d_x0.p;
}
int ipcgpu_round_friction_energy(ipcgpu_ctx* c, int id, const double* Vt, double eps2, double* E)
{
    return guarded([&] {
        HipRoundCollider& h = RC(c, id);
        bind(c);
        needArg(E && eps2 > 0.0, "bad friction argument");
        *E = h.frictionEnergy(c->mesh->d_x.p, roundXt(c, Vt), eps2);
        return IPCGPU_OK;
    });
}
int ipcgpu_round_friction_gradient_add(ipcgpu_ctx* c, int id, const double* Vt, double eps2, double* g)
{
    return guarded([&] {
        HipRoundCollider& h = RC(c, id);
        HipOptimizer& o = O(c);
        bind(c);
        needArg(g && eps2 > 0.0, "bad friction argument");
        const size_t n3 = 3 * (size_t)c->mesh->nV;
        const double* xt = roundXt(c, Vt);
        HIP_CHECK(hipMemcpyAsync(o.d_gradient.p, g, n3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
        h.frictionGradientAdd(c->mesh->d_x.p, xt, eps2, o.d_gradient.p);
        o.d_gradient.download(g, n3, c->stream);
        return IPCGPU_OK;
    });
}
int ipcgpu_round_friction_hessian_add(ipcgpu_ctx* c, int id, const double* Vt, double eps2, int projectDBC)
{
    return guarded([&] {
        HipRoundCollider& h = RC(c, id);
        bind(c);
        needArg(eps2 > 0.0, "bad friction argument");
        need(c->lin->numRows == 3 * c->mesh->nV, "call ipcgpu_linsys_set_pattern first");
        h.frictionHessianAdd(c->mesh->d_x.p, roundXt(c, Vt), c->mesh->d_dbc.p, c->lin->d_rowBase.p, c->lin->d_rowLen.p, eps2, projectDBC, c->lin->d_a.p);
        HIP_CHECK(hipStreamSynchronize(c->stream));
        return IPCGPU_OK;
    });
}
int ipcgpu_round_state(ipcgpu_ctx* c, int id, double dHat, double kappa, int* nSet, double* out10)
{
    return guarded([&] {
        HipRoundCollider& h = RC(c, id);
        HipOptimizer& o = O(c);
        bind(c);
        needArg(out10 != nullptr, "null result");
        const int n = h.state(CT(c).nSVI, CT(c).d_SVI.p, c->mesh->d_x.p, o.d_xPrev.p, dHat > 0.0 ? dHat : o.dHat, kappa > 0.0 ? kappa : o.kappa, o.fricDHat, out10);
        if (nSet) *nSet = n;
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_set_friction(ipcgpu_ctx* c, double selfFric, int fricIterAmt, double epsV)
{
    specChanged(c);
    return guarded([&] {
        HipOptimizer& o = O(c);
        needArg(selfFric >= 0.0 && epsV > 0.0, "bad friction parameters");
        o.selfFric = selfFric;
        o.fricIterAmt = fricIterAmt;
        o.epsV = epsV;
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_set_friction_target(ipcgpu_ctx* c, double epsVTarget)
{
    specChanged(c);
    return guarded([&] {
        O(c).epsVTarget = epsVTarget > 0.0 ? epsVTarget : -1.0;
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_set_constructor_dt(ipcgpu_ctx* c, double h)
{
    specChanged(c);
    return guarded([&] {
        needArg(h > 0.0, "the step size must be positive");
        O(c).ctorDt = h;
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_set_parameter_scaling(ipcgpu_ctx* c, int useAbsParameters, double dTolRel, double kappaMinMultiplier)
{
    specChanged(c);
    return guarded([&] {
        O(c).setParameterScaling(useAbsParameters != 0, dTolRel, kappaMinMultiplier);
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_set_kappa(ipcgpu_ctx* c, double kappa)
{
    specChanged(c);
    return guarded([&] {
        needArg(kappa >= 0.0, "negative barrier stiffness");
        O(c).kappaConfig = kappa;
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_set_dhat_target(ipcgpu_ctx* c, double dHatTargetEps)
{
    specChanged(c);
    return guarded([&] {
        needArg(dHatTargetEps == dHatTargetEps, "dHat target is not a number");
        O(c).dHatTargetEps = dHatTargetEps;
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_set_damping(ipcgpu_ctx* c, double dampingStiff)
{
    specChanged(c);
    return guarded([&] {
        needArg(dampingStiff == dampingStiff, "damping stiffness is not a number");
        O(c).setDamping(dampingStiff);
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_set_friction_scales(ipcgpu_ctx* c, double scaleSelf, double scaleObstacle)
{
    specChanged(c);
    return guarded([&] {
        needArg(scaleSelf >= 0.0 && scaleObstacle >= 0.0, "friction scales must not be negative");
        CT(c).fricScaleSelf = scaleSelf;
        CT(c).fricScaleObst = scaleObstacle;
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_force_friction_loop(ipcgpu_ctx* c, int on)
{
    return guarded([&] {
        O(c).fricLoopForced = on != 0;
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_set_half_space_friction(ipcgpu_ctx* c, int id, double mu)
{
    specChanged(c);
    return guarded([&] {
        needArg(mu >= 0.0, "negative friction coefficient");
        HS(c, id).friction = mu;
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_next_subproblem(ipcgpu_ctx* c, int* more)
{
    specChanged(c);
    return guarded([&] {
        bind(c);
        const bool m = O(c).nextSubproblem();
        if (more) *more = m ? 1 : 0;
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_get_friction_state(ipcgpu_ctx* c, double* sc, double* lambda)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        const size_t n = (o.contact && o.selfCollision) ? o.contact->fricSet.size() : 0;
        if (sc) {
            sc[0] = o.fricDHat;
            sc[1] = (double)n;
            sc[2] = (double)o.fricIterI;
            size_t nh = 0;
            for (const auto& h : o.planes) nh += h->lagSet.size();
            sc[3] = (double)nh;
        }
        if (lambda && n) o.contact->d_fricLambda.download(lambda, n, c->stream);
        return IPCGPU_OK;
    });
}
int ipcgpu_friction_update(ipcgpu_ctx* c, double dHat, double kappa, int* nLagged)
{
    return guarded([&] {
        M(c);
        bind(c);
        CT(c).frictionLagUpdate(c->mesh->d_x.p, dHat, kappa);
        HIP_CHECK(hipStreamSynchronize(c->stream));
        if (nLagged) *nLagged = (int)CT(c).fricSet.size();
        return IPCGPU_OK;
    });
}
int ipcgpu_friction_get(ipcgpu_ctx* c, double* lambda, double* coord, double* basis)
{
    return guarded([&] {
        M(c);
        bind(c);
        needArg(lambda && coord && basis, "null output");
        CT(c).frictionGet(lambda, coord, basis);
        return IPCGPU_OK;
    });
}
int ipcgpu_friction_energy(ipcgpu_ctx* c, const double* Vt, double eps2, double coef, double* E)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(o.initialised, "call ipcgpu_opt_init first");
        needArg(Vt && E && eps2 > 0, "bad argument");
        uploadColMajor(c, Vt, o.d_x0);
        *E = CT(c).frictionEnergy(c->mesh->d_x.p, o.d_x0.p, eps2, coef, o.d_partial, o.slot(S_FRICTION_E));
        return IPCGPU_OK;
    });
}
int ipcgpu_friction_gradient_add(ipcgpu_ctx* c, const double* Vt, double eps2, double coef, double* g)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(o.initialised, "call ipcgpu_opt_init first");
        needArg(Vt && g && eps2 > 0, "bad argument");
        const size_t n3 = 3 * (size_t)c->mesh->nV;
        uploadColMajor(c, Vt, o.d_x0);
        HIP_CHECK(hipMemcpyAsync(o.d_gradient.p, g, n3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
        CT(c).frictionGradientAdd(c->mesh->d_x.p, o.d_x0.p, eps2, coef, o.d_gradient.p);
        o.d_gradient.download(g, n3, c->stream);
        return IPCGPU_OK;
    });
}
int ipcgpu_friction_hessian_add(ipcgpu_ctx* c, const double* Vt, double eps2, double coef, int projectDBC)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(o.initialised, "call ipcgpu_opt_init first");
        need(c->lin->numRows == 3 * c->mesh->nV, "call ipcgpu_linsys_set_pattern first");
        needArg(Vt && eps2 > 0, "bad argument");
        uploadColMajor(c, Vt, o.d_x0);
        CT(c).frictionHessianAdd(c->mesh->d_x.p, o.d_x0.p, c->mesh->d_dbc.p, *c->lin, eps2, coef, projectDBC, c->lin->d_a.p);
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_set_velocity(ipcgpu_ctx* c, const double* vel)
{
    specChanged(c);
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(o.initialised, "call ipcgpu_opt_init first");
        needArg(vel != nullptr, "null velocity");
        o.setVelocity(vel);
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_set_warm_start(ipcgpu_ctx* c, int option)
{
    specChanged(c);
    return guarded([&] {
        HipOptimizer& o = O(c);
        needArg(option >= 0 && option <= 5, "warmStart option must be 0..5");
        o.warmStart = option;
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_get_warm_step(ipcgpu_ctx* c, double* out)
{
    return guarded([&] {
        if (out) *out = O(c).warmStepSize;
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_set_time_integration(ipcgpu_ctx* c, int type, double beta, double gamma)
{
    specChanged(c);
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(o.initialised, "call ipcgpu_opt_init first");
        needArg(type == 0 || type == 1, "time integration: 0 = BE, 1 = NM");
        needArg(type == 0 || (beta > 0.0 && gamma >= 0.0), "Newmark needs beta > 0, gamma >= 0");
        o.setTimeIntegration(type, beta, gamma);
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_add_dirichlet(ipcgpu_ctx* c, int n, const int* ids, const double* lin3, const double* ang3, double t0, double t1)
{
    specChanged(c);
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(o.initialised, "call ipcgpu_opt_init first");
        needArg(n > 0 && ids && lin3 && ang3, "empty Dirichlet group");
        for (int i = 0; i < n; ++i) needArg(ids[i] >= 0 && ids[i] < c->mesh->nV, "vertex id out of range");
        o.addDirichletBC(n, ids, lin3, ang3, t0, t1);
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_end_dirichlet(ipcgpu_ctx* c, int group, double t_end)
{
    specChanged(c);
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        needArg(group >= 0 && group < (int)o.dbcGroups.size(), "no such Dirichlet group");
        o.dbcGroups[group]->t1 = std::min(o.dbcGroups[group]->t1, t_end);
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_set_dirichlet_motion(ipcgpu_ctx* c, int group, const double* lin3, const double* ang3, const double* center3, int forceNonzero)
{
    specChanged(c);
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        needArg(group >= 0 && group < (int)o.dbcGroups.size(), "no such Dirichlet group");
        needArg(lin3 && ang3, "null velocity");
        auto& g = *o.dbcGroups[group];
        for (int k = 0; k < 3; ++k) {
            g.lin[k] = lin3[k];
            g.ang[k] = ang3[k];
            if (center3) g.center[k] = center3[k];
        }
        g.hasCenter = center3 != nullptr;
        g.forceNonzero = forceNonzero != 0;
        o.setDBCVertices();
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_set_dirichlet_targets(ipcgpu_ctx* c, int group, int n, const double* targets)
{
    specChanged(c);
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        needArg(group >= 0 && group < (int)o.dbcGroups.size(), "no such Dirichlet group");
        auto& g = *o.dbcGroups[group];
        if (!targets) {
            g.hasTargets = false;
            return IPCGPU_OK;
        }
        needArg(n == (int)g.ids.size(), "one target position per node of the group");
        g.d_targets.upload(targets, 3 * (size_t)n, c->stream);
        HIP_CHECK(hipStreamSynchronize(c->stream));
        g.hasTargets = true;
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_add_neumann(ipcgpu_ctx* c, int n, const int* ids, const double* accel3, double t0, double t1)
{
    specChanged(c);
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(o.initialised, "call ipcgpu_opt_init first");
        needArg(n > 0 && ids && accel3, "empty Neumann group");
        for (int i = 0; i < n; ++i) needArg(ids[i] >= 0 && ids[i] < c->mesh->nV, "vertex id out of range");
        o.addNeumannBC(n, ids, accel3, t0, t1);
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_get_dbc_state(ipcgpu_ctx* c, double* out4)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        need(o.initialised, "call ipcgpu_opt_init first");
        needArg(out4 != nullptr, "null output");
        o.getDbcState(out4);
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_get_kinematics(ipcgpu_ctx* c, double* vel, double* acc, double* dx)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(o.initialised, "call ipcgpu_opt_init first");
        o.getKinematics(vel, acc, dx);
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_set_components(ipcgpu_ctx* c, int nComp, const int* nodeEnd, const int* tetEnd)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        needArg(nComp >= 1 && nodeEnd && tetEnd, "set_components: at least one component and both tables");
        o.setComponents(nComp, nodeEnd, tetEnd);
        if (c->contact && c->contact->hasGroups) { // the contact groups belong to the previous table: back to the default
            specChanged(c);
            bind(c);
            c->contact->setGroups(c->mesh->nV, {}, {}, 1);
        }
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_system_report(ipcgpu_ctx* c, double* sysE, double* sysM, double* sysL)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(o.initialised, "call ipcgpu_opt_init first");
        if (c->mesh->shell.nTri()) throw UnsupportedError("system report with a shell set (the report's slices do not know the shell energy)");
        if (c->mesh->rod.nSeg()) throw UnsupportedError("system report with a rod set (the report's slices do not know the rod energy)");
        if (c->mesh->attach.n()) throw UnsupportedError("system report with attachments set (their energy belongs to no single component)");
        if (c->mesh->chamber.n()) throw UnsupportedError("system report with chambers set (the report's slices do not know the pressure energy)");
        if (c->mesh->aero.n()) throw UnsupportedError("system report with aerodynamic surfaces set (the report's slices do not know the dissipation of the air drag)");
        if (!o.rounds.empty()) throw UnsupportedError("system report with a round collider set (the report's slices do not know its barrier and friction energy)");
        o.systemReport(sysE, sysM, sysL);
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_save_status(ipcgpu_ctx* c, const char* path)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(o.initialised, "call ipcgpu_opt_init first");
        needArg(path != nullptr && path[0] != 0, "empty path");
        o.saveStatus(path);
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_load_status(ipcgpu_ctx* c, const char* path)
{
    specChanged(c);
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(o.initialised, "call ipcgpu_opt_init first");
        needArg(path != nullptr && path[0] != 0, "empty path");
        o.loadStatus(path);
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_get_contact_state(ipcgpu_ctx* c, int* counts6, int* pair2)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        need(o.ipOn(), "neither self collision nor a half-space is enabled");
        if (counts6) {
            counts6[0] = o.selfCollision ? o.contact->nActive() : 0;
            counts6[1] = o.selfCollision ? o.contact->nPara() : 0;
            counts6[2] = o.selfCollision ? o.contact->nCand() : 0;
            counts6[3] = 0;
            for (const auto& h : o.planes) counts6[3] += (int)h->set.size();
            counts6[4] = o.nFullCCD;
            counts6[5] = o.nPatternChanges;
        }
        if (pair2) {
            pair2[0] = o.lastCCDPair[0];
            pair2[1] = o.lastCCDPair[1];
        }
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_precompute(ipcgpu_ctx* c)
{
    return guarded([&] {
        bind(c);
        O(c).precompute();
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_begin_timestep(ipcgpu_ctx* c)
{
    return guarded([&] {
        bind(c);
        O(c).beginTimestep();
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_newton_iter(ipcgpu_ctx* c, int* converged)
{
    return guarded([&] {
        bind(c);
        const bool cv = O(c).newtonIter();
        if (converged) *converged = cv ? 1 : 0;
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_end_timestep(ipcgpu_ctx* c)
{
    return guarded([&] {
        bind(c);
        O(c).endTimestep();
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_solve_timestep(ipcgpu_ctx* c, int maxIter, int* nIter)
{
    return guarded([&] {
        bind(c);
        const int n = O(c).solveTimestep(maxIter);
        if (nIter) *nIter = n;
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_get_state(ipcgpu_ctx* c, double* V, double* p, double* g, double* sc)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(o.initialised, "call ipcgpu_opt_init first");
        const size_t n3 = 3 * (size_t)c->mesh->nV;
        if (V) downloadColMajor(c, c->mesh->d_x, V);
        if (p) o.d_searchDir.download(p, n3, c->stream);
        if (g) o.d_gradient.download(g, n3, c->stream);
        if (sc) {
            sc[0] = o.lastEnergyVal;
            sc[1] = o.lastStepSize;
            sc[2] = o.targetGRes;
            sc[3] = o.innerIterAmt;
            sc[4] = o.globalIterNum;
            sc[5] = o.lastAlphaFeasible;
            sc[6] = o.kappa;
            sc[7] = o.dHat;
        }
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_get_timers(ipcgpu_ctx* c, double* t)
{
    return guarded([&] {
        O(c).resolveEventTimers();
        std::memcpy(t, O(c).timers, sizeof(double) * 16);
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_set_allreduce(ipcgpu_ctx* c, ipcgpu_allreduce_fn fn, void* user)
{
    return guarded([&] {
        needArg(c != nullptr, "null context");
        c->opt->allreduce = fn;
        c->opt->allreduceUser = user;
        // a solver that was sharded before keeps copies of the hooks: refresh them (no new analysis)
        c->lin->setHooks(c->opt->allreduce, c->opt->allreduceUser, c->opt->allreduceStream, c->opt->allreduceStreamUser);
        return IPCGPU_OK;
    });
}

int ipcgpu_opt_set_allreduce_stream(ipcgpu_ctx* c, ipcgpu_allreduce_stream_fn fn, void* user)
{
    return guarded([&] {
        needArg(c != nullptr, "null context");
        c->opt->allreduceStream = fn;
        c->opt->allreduceStreamUser = user; // its own slot: a host hook set earlier keeps its user pointer; detaching (fn = NULL) leaves that hook in charge
        c->lin->setHooks(c->opt->allreduce, c->opt->allreduceUser, c->opt->allreduceStream, c->opt->allreduceStreamUser);
        return IPCGPU_OK;
    });
}
static_assert(sizeof(ipcgpu_p2p_op) == sizeof(MfNumeric::P2POp), "ipcgpu_p2p_op and MfNumeric::P2POp must be one layout");
int ipcgpu_opt_set_exchange(ipcgpu_ctx* c, ipcgpu_exchange_fn fn, void* user)
{
    return guarded([&] {
        needArg(c != nullptr, "null context");
        c->exchange = reinterpret_cast<void*>(fn);
        c->exchangeUser = user;
        c->lin->setExchangeHooks(reinterpret_cast<MfNumeric::ExchangeFn>(c->exchange), c->exchangeUser, reinterpret_cast<MfNumeric::ExchangeStreamFn>(c->exchangeStream),
            c->exchangeStreamUser);
        return IPCGPU_OK;
    });
}
int ipcgpu_opt_set_exchange_stream(ipcgpu_ctx* c, ipcgpu_exchange_stream_fn fn, void* user)
{
    return guarded([&] {
        needArg(c != nullptr, "null context");
        c->exchangeStream = reinterpret_cast<void*>(fn);
        c->exchangeStreamUser = user;
        c->lin->setExchangeHooks(reinterpret_cast<MfNumeric::ExchangeFn>(c->exchange), c->exchangeUser, reinterpret_cast<MfNumeric::ExchangeStreamFn>(c->exchangeStream),
            c->exchangeStreamUser);
        return IPCGPU_OK;
    });
}
int ipcgpu_ctx_get_stream(ipcgpu_ctx* c, void** hipStream)
{
    return guarded([&] {
        needArg(c != nullptr && hipStream != nullptr, "null argument");
        *hipStream = (void*)c->stream;
        return IPCGPU_OK;
    });
}

// ---- measurement ------------------------------------------------------------------------------------
int ipcgpu_bench_assembly(ipcgpu_ctx* c, double dtSq, int reps, double* avg_ms, double* bytes)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(o.initialised && !c->lin->rowBase.empty(), "needs opt_init + a pattern");
        needArg(reps > 0, "reps must be positive");
        hipEvent_t e0, e1;
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
        const ElemView v = o.view();
        o.ensurePatchPlan();
        int pb, pe;
        o.patchShard(pb, pe);
        double total = 0.0;
        for (int r = 0; r < reps; ++r) {
            HIP_CHECK(hipEventRecord(e0, c->stream));
            launch_assemble_patches(v, o.patch, pb, pe, dtSq, 1, o.d_gradient.p, c->lin->d_a.p, c->stream);
            HIP_CHECK(hipEventRecord(e1, c->stream));
            HIP_CHECK(hipEventSynchronize(e1));
            float ms = 0;
            HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
            total += ms;
        }
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        *avg_ms = total / reps;
        const double nT = o.tetEnd - o.tetBegin;
        // B_asm = 112 nT + 84 nV + 8 nnz
        *bytes = 112.0 * nT + 84.0 * c->mesh->nV + 8.0 * (double)c->lin->ja.size();
        return IPCGPU_OK;
    });
}
int ipcgpu_bench_factor_solve(ipcgpu_ctx* c, int reps, double* fms, double* sms)
{
    return guarded([&] {
        HipOptimizer& o = O(c);
        bind(c);
        need(c->lin->analyzed(), "needs analyze_pattern");
        hipEvent_t e0, e1, e2;
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
        HIP_CHECK(hipEventCreate(&e2));
        double tf = 0, ts = 0;
        for (int r = 0; r < reps; ++r) {
            HIP_CHECK(hipEventRecord(e0, c->stream));
            c->lin->factorize();
            HIP_CHECK(hipEventRecord(e1, c->stream));
            c->lin->solve(o.d_gradient.p, o.d_minusG.p);
            HIP_CHECK(hipEventRecord(e2, c->stream));
            HIP_CHECK(hipEventSynchronize(e2));
            float a = 0, b = 0;
            HIP_CHECK(hipEventElapsedTime(&a, e0, e1));
            HIP_CHECK(hipEventElapsedTime(&b, e1, e2));
            tf += a;
            ts += b;
        }
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        (void)hipEventDestroy(e2);
        *fms = tf / reps;
        *sms = ts / reps;
        return IPCGPU_OK;
    });
}
int ipcgpu_bench_multiply_sym(ipcgpu_ctx* c, int reps, double* avg_ms, double* bytes)
{
    return guarded([&] {
        needArg(c && reps > 0 && avg_ms && bytes, "bad argument");
        bind(c);
        HipLinSysSolver& l = L(c);
        need(l.numRows > 0, "no pattern");
        DevBuf<double> x, y;
        x.alloc(l.numRows);
        y.alloc(l.numRows);
        launch_fill(x.p, l.numRows, 1.0, c->stream);
        l.multiplySym(x.p, y.p); // (builds the pattern's index; warm-up)
        hipEvent_t e0, e1;
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
        HIP_CHECK(hipEventRecord(e0, c->stream));
        for (int r = 0; r < reps; ++r) l.multiplySym(x.p, y.p);
        HIP_CHECK(hipEventRecord(e1, c->stream));
        HIP_CHECK(hipEventSynchronize(e1));
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        *avg_ms = ms / reps;
        *bytes = 12.0 * (double)l.ja.size() + 16.0 * l.numRows; // values + columns + the two vectors, each once
        return IPCGPU_OK;
    });
}
int ipcgpu_bench_stream(ipcgpu_ctx* c, long long bytes, int reps, double* gbps)
{
    return guarded([&] {
        needArg(c && bytes > 0 && reps > 0, "bad argument");
        bind(c);
        DevBuf<double> a, b;
        a.alloc((size_t)bytes / 8);
        b.alloc((size_t)bytes / 8);
        a.zero(c->stream);
        hipEvent_t e0, e1;
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
        HIP_CHECK(hipMemcpyAsync(b.p, a.p, bytes, hipMemcpyDeviceToDevice, c->stream));
        HIP_CHECK(hipEventRecord(e0, c->stream));
        for (int r = 0; r < reps; ++r) HIP_CHECK(hipMemcpyAsync(b.p, a.p, bytes, hipMemcpyDeviceToDevice, c->stream));
        HIP_CHECK(hipEventRecord(e1, c->stream));
        HIP_CHECK(hipEventSynchronize(e1));
        float ms = 0;
        HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        *gbps = 2.0 * (double)bytes * reps / (ms * 1e-3) / 1e9; // read + write
        return IPCGPU_OK;
    });
}
}
