"""ctypes binding of include/ipcgpu.h.

Method names follow the reference interfaces the C ABI replaces
(LinSysSolver.hpp:31-467, Energy.hpp:27-138, Optimizer.hpp:28-283) so that the
parity tests read like tests of the reference classes.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# IPCGPU_LIB_VARIANT selects an experiment build made by tools/ (ipc_amd/build.py variant=...); unset = the product library
_LIB_PATH = os.path.join(_HERE, "libipcgpu_%s.so" % os.environ["IPCGPU_LIB_VARIANT"] if os.environ.get("IPCGPU_LIB_VARIANT") else "libipcgpu.so")
_HEADER = os.path.join(_HERE, "..", "include", "ipcgpu.h")

c_dp = C.POINTER(C.c_double)
c_ip = C.POINTER(C.c_int)

IPCGPU_OK = 0
IPCGPU_NOT_PD = 1
SOLVER_MULTIFRONTAL = 0
SOLVER_ROCSOLVER_CSRRF = 1
SOLVER_PCG = 2  # the reference's `linearSolver AMGCL`: preconditioned CG (ipcgpu_linsys_set_iterative)
PRECOND_BLOCK_JACOBI = 0
PRECOND_LAGGED_CHOLESKY = 1
PRECOND_TWO_LEVEL = 2  # block Jacobi + an exact coarse solve on six rigid-body modes per node aggregate

ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int)


class P2POp(C.Structure):  # ipcgpu_p2p_op
    _fields_ = [("buf_dev", C.c_void_p), ("count", C.c_longlong), ("peer", C.c_int), ("send", C.c_int)]


EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(P2POp))


class IpcGpuError(RuntimeError):
    pass


class NotPositiveDefinite(IpcGpuError):
    pass


def lib_path() -> str:
    return _LIB_PATH


def declared_symbols():
    """Every function declared in include/ipcgpu.h (used by the CPU-side export test)."""
    txt = open(_HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(ipcgpu_[a-z0-9_]+)\s*\(", txt)) - {"ipcgpu_allreduce_fn", "ipcgpu_allreduce_stream_fn"})


_RCCL_PATH = os.path.join(os.path.dirname(_LIB_PATH), os.path.basename(_LIB_PATH).replace("libipcgpu", "libipcgpu_rccl", 1) if "libipcgpu_" not in os.path.basename(_LIB_PATH)
                          else os.path.basename(_LIB_PATH).replace(".so", "_rccl.so"))
_RCCL_HEADER = os.path.join(os.path.dirname(_HEADER), "ipcgpu_rccl.h")
_rccl = None


def rccl_declared_symbols():
    """Every function include/ipcgpu_rccl.h declares (the caller-side RCCL binding, libipcgpu_rccl.so)."""
    txt = re.sub(r"/\*.*?\*/", "", open(_RCCL_HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ipcgpu_rccl_[a-z0-9_]+)\s*\(", txt)))


def load_rccl():
    """dlopen libipcgpu_rccl.so (include/adapters/ipcgpu_rccl.cpp: RCCL bound to a context from C)."""
    global _rccl
    if _rccl is None:
        load_library()
        if not os.path.exists(_RCCL_PATH):
            raise IpcGpuError(f"{_RCCL_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        _rccl = C.CDLL(_RCCL_PATH)
        _rccl.ipcgpu_rccl_last_error.restype = C.c_char_p
    return _rccl


_lib = None


def load_library():
    """dlopen libipcgpu.so.  Raises when it has not been built: there is no fallback path."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise IpcGpuError(f"{_LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        _lib = C.CDLL(_LIB_PATH)
        _lib.ipcgpu_last_error.restype = C.c_char_p
        _lib.ipcgpu_tet_mesh_free.restype = None
        _lib.ipcgpu_tet_mesh_free.argtypes = [C.c_void_p]
        _lib.ipcgpu_tet_mesh_get.argtypes = [C.c_void_p, c_dp, c_ip, c_ip]
    return _lib


# one row of Context.contact_report (ipcgpu_contact_report: rowsI[8], rowsD[20])
CONTACT_REPORT_DTYPE = np.dtype([(k, np.int32) for k in ("a", "b", "nPP", "nPE", "nPT", "nEE", "nMollified", "argmin")] + [("minD2", np.float64)]
                                + [(k, np.float64, (3,)) for k in ("FA", "FB", "TA", "TB", "RA", "RB")] + [("W", np.float64)])


def _dp(a):
    return a.ctypes.data_as(c_dp) if a is not None else None


def _ip(a):
    return a.ctypes.data_as(c_ip) if a is not None else None


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def read_tet_mesh(path):
    """IglUtils::readTetMesh through the C ABI: (V, T, SF) of a .msh file (MSH 4.1 / 2.2 ASCII or the reference's msh-4.0 dialect)."""
    L = load_library()
    h = C.c_void_p()
    nV, nT, nSF = C.c_int(), C.c_int(), C.c_int()
    rc = L.ipcgpu_read_tet_mesh(str(path).encode(), C.byref(h), C.byref(nV), C.byref(nT), C.byref(nSF))
    if rc != 0:
        raise RuntimeError(f"ipcgpu_read_tet_mesh failed ({rc}): {L.ipcgpu_last_error().decode()}")
    try:
        V = np.zeros((nV.value, 3), order="F")
        T = np.zeros((nT.value, 4), dtype=np.int32, order="F")
        SF = np.zeros((nSF.value, 3), dtype=np.int32, order="F")
        rc = L.ipcgpu_tet_mesh_get(h, _dp(V), _ip(T), _ip(SF))
        if rc != 0:
            raise RuntimeError(f"ipcgpu_tet_mesh_get failed ({rc})")
    finally:
        L.ipcgpu_tet_mesh_free(h)
    return V, T, SF


def save_tet_mesh(path, V, T):
    """IglUtils::saveTetMesh through the C ABI (MSH 4.1 ASCII + $Surface)."""
    L = load_library()
    V = np.asfortranarray(V, dtype=np.float64)
    T = np.asfortranarray(T, dtype=np.int32)
    rc = L.ipcgpu_save_tet_mesh(str(path).encode(), C.c_int(V.shape[0]), C.c_int(T.shape[0]), _dp(V), _ip(T))
    if rc != 0:
        raise RuntimeError(f"ipcgpu_save_tet_mesh failed ({rc}): {L.ipcgpu_last_error().decode()}")


class Context:
    """One `ipcgpu_ctx` == one Optimizer with its Mesh, Energy and LinSysSolver on one GPU."""

    def __init__(self, device: int = 0, solver: int = SOLVER_MULTIFRONTAL):
        self._L = load_library()
        h = C.c_void_p()
        self._chk(self._L.ipcgpu_ctx_create(C.c_int(device), C.byref(h)))
        self.h = h
        self.nV = self.nT = 0
        self._cb = None
        if solver != SOLVER_MULTIFRONTAL:
            self.set_solver(solver)

    def _chk(self, rc, allow_not_pd=False):
        if rc == IPCGPU_OK:
            return rc
        if rc == IPCGPU_NOT_PD and allow_not_pd:
            return rc
        msg = self._L.ipcgpu_last_error().decode(errors="replace")
        if rc == IPCGPU_NOT_PD:
            raise NotPositiveDefinite(msg or "matrix not positive definite")
        raise IpcGpuError(f"ipcgpu error {rc}: {msg}")

    def close(self):
        if getattr(self, "h", None):
            self.rccl_detach()
            self._L.ipcgpu_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- context
    def set_solver(self, solver):
        self._chk(self._L.ipcgpu_ctx_set_solver(self.h, C.c_int(solver)))

    def set_shard(self, rank, world):
        self._chk(self._L.ipcgpu_ctx_set_shard(self.h, C.c_int(rank), C.c_int(world)))

    def set_solver_shard(self, rank, world):
        """subtree-sharded factorisation / solves (ipcgpu_linsys_set_shard); call after set_allreduce"""
        self._chk(self._L.ipcgpu_linsys_set_shard(self.h, C.c_int(rank), C.c_int(world)))

    def set_exchange(self, pyfunc):
        """the point-to-point hook of the sharded solver (ipcgpu_opt_set_exchange, host-ordered): pyfunc(ops) with ops = [(dev_ptr, count, peer, send), ...],
        ONE group -- no order between the operations may be assumed; returns 0."""
        def tramp(user, n, ops):
            try:
                return int(pyfunc([(int(ops[i].buf_dev), int(ops[i].count), int(ops[i].peer), int(ops[i].send)) for i in range(n)]))
            except Exception as e:  # noqa: BLE001
                print("exchange hook failed:", e, flush=True)
                return 1
        self._xcb = EXCHANGE_FN(tramp)
        self._chk(self._L.ipcgpu_opt_set_exchange(self.h, self._xcb, None))

    def solver_exchange_stats(self):
        """bytes this rank sent / received point to point through the solver so far (ipcgpu_linsys_exchange_stats)"""
        o = np.zeros(4)
        self._chk(self._L.ipcgpu_linsys_exchange_stats(self.h, _dp(o)))
        return dict(sent_bytes=int(o[0]), received_bytes=int(o[1]), calls=int(o[2]), wait_ms=float(o[3]))

    def solver_critical_path(self):
        """inputs of the strong-scaling model (ipcgpu_linsys_critical_path): dependent pivot steps of the assembly tree, those above the cut, the largest rank's share
        of the flops below the cut, levels, levels with a front above the cut"""
        o = np.zeros(5)
        self._chk(self._L.ipcgpu_linsys_critical_path(self.h, _dp(o)))
        return dict(steps=o[0], steps_above_cut=o[1], max_rank_share_below=o[2], levels=int(o[3]), levels_above_cut=int(o[4]))

    def entry_destinations(self):
        """per CSR entry its slot in the front buffer as the set-up's device kernel computed it (ipcgpu_linsys_entry_destinations)"""
        rows, nnz = self.get_dims()
        out = np.zeros(nnz, dtype=np.int64)
        self._chk(self._L.ipcgpu_linsys_entry_destinations(self.h, out.ctypes.data_as(C.POINTER(C.c_longlong))))
        return out

    def solver_shard_stats(self):
        o = np.zeros(2)
        self._chk(self._L.ipcgpu_linsys_shard_stats(self.h, _dp(o)))
        return dict(world=int(o[0]), shared_flop_fraction=float(o[1]))

    def comm_stats(self):
        """what crossed ranks so far (bytes, calls) through the time stepper's and through the solver's all-reduces; nodes whose rows this rank assembles"""
        o = np.zeros(6)
        self._chk(self._L.ipcgpu_opt_comm_stats(self.h, _dp(o)))
        return dict(stepper_bytes=int(o[0]), stepper_calls=int(o[1]), solver_bytes=int(o[2]), solver_calls=int(o[3]), rows_assembled_nodes=int(o[4]), nodes=int(o[5]))

    def complete_matrix(self):
        self._chk(self._L.ipcgpu_opt_complete_matrix(self.h))

    # ---- RCCL from C (include/ipcgpu_rccl.h): every exchange is then one ncclAllReduce on the context's own stream
    @staticmethod
    def rccl_unique_id():
        R = load_rccl()
        buf = C.create_string_buffer(128)
        if R.ipcgpu_rccl_unique_id(buf) != 0:
            raise IpcGpuError("ipcgpu_rccl_unique_id: " + R.ipcgpu_rccl_last_error().decode())
        return buf.raw

    def rccl_attach(self, rank, world, id128):
        R = load_rccl()
        if R.ipcgpu_rccl_attach(self.h, C.c_int(rank), C.c_int(world), C.c_char_p(bytes(id128))) != 0:
            raise IpcGpuError("ipcgpu_rccl_attach: " + R.ipcgpu_rccl_last_error().decode())
        self._rccl_attached = True

    def rccl_detach(self):
        if getattr(self, "_rccl_attached", False):
            load_rccl().ipcgpu_rccl_detach(self.h)
            self._rccl_attached = False

    def rccl_selftest_p2p(self, rank, world, count=1024):
        R = load_rccl()
        out = C.c_double()
        if R.ipcgpu_rccl_selftest_p2p(self.h, C.c_int(rank), C.c_int(world), C.c_longlong(count), C.byref(out)) != 0:
            raise IpcGpuError("ipcgpu_rccl_selftest_p2p: " + R.ipcgpu_rccl_last_error().decode())
        return out.value

    def rccl_selftest(self, rank, count=1024, op=0):
        R = load_rccl()
        out = C.c_double()
        if R.ipcgpu_rccl_selftest(self.h, C.c_int(rank), C.c_longlong(count), C.c_int(op), C.byref(out)) != 0:
            raise IpcGpuError("ipcgpu_rccl_selftest: " + R.ipcgpu_rccl_last_error().decode())
        return out.value

    def set_allreduce(self, pyfunc):
        """pyfunc(dev_ptr:int, count:int, op:int) -> int (0 ok)."""
        def tramp(user, buf, count, op):
            try:
                return int(pyfunc(int(buf), int(count), int(op)))
            except Exception as e:  # noqa: BLE001
                print("allreduce hook failed:", e, flush=True)
                return 1
        self._cb = ALLREDUCE_FN(tramp)
        self._chk(self._L.ipcgpu_opt_set_allreduce(self.h, self._cb, None))

    # ---- Mesh
    def set_mesh(self, V, F, YM=2e4, PR=0.4, density=1000.0):
        V = np.asfortranarray(V, dtype=np.float64)
        F = np.asfortranarray(F, dtype=np.int32)
        self.nV, self.nT = V.shape[0], F.shape[0]
        self._ncomp = 1  # a new mesh is one component until set_components
        self._chk(self._L.ipcgpu_set_mesh(self.h, C.c_int(self.nV), C.c_int(self.nT), _dp(V), _ip(F),
                                          C.c_double(YM), C.c_double(PR), C.c_double(density)))

    def set_dbc(self, ids, typ):
        ids = _i32(ids)
        self._chk(self._L.ipcgpu_set_dbc(self.h, C.c_int(len(ids)), _ip(ids), C.c_int(typ)))

    def set_component_material(self, node_range, tet_range, density, YM, PR):
        self._chk(self._L.ipcgpu_set_component_material(self.h, C.c_int(node_range[0]), C.c_int(node_range[1]), C.c_int(tet_range[0]),
                                                        C.c_int(tet_range[1]), C.c_double(density), C.c_double(YM), C.c_double(PR)))

    def set_components(self, node_end, tet_end):
        """The mesh components of the system report: accumulated node / element ends (the reference's compVAccSize / compFAccSize)."""
        node_end, tet_end = _i32(node_end).ravel(), _i32(tet_end).ravel()
        if len(node_end) != len(tet_end):
            raise ValueError("set_components: one node end and one element end per component")
        self._chk(self._L.ipcgpu_opt_set_components(self.h, C.c_int(len(node_end)), _ip(node_end), _ip(tet_end)))
        self._ncomp = len(node_end)

    def system_report(self):
        """Optimizer::computeSystemEnergy on the device: (E[nComp], M[nComp, 3], L[nComp, 3]) -- energy, linear momentum and angular momentum about
        the origin per component, for the state after precompute() or the last finished time step."""
        n = getattr(self, "_ncomp", 1)
        E, M, L = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3))
        self._chk(self._L.ipcgpu_opt_system_report(self.h, _dp(E), _dp(M), _dp(L)))
        return E, M, L

    def set_energy_type(self, name):
        """Scene-script `energy NH|FCR|SNH` (SNH: stable neo-Hookean, energy type 2 of the C ABI)."""
        self._chk(self._L.ipcgpu_set_energy_type(self.h, C.c_int({"NH": 0, "FCR": 1, "SNH": 2}[name])))

    def clear_dbc(self):
        self._chk(self._L.ipcgpu_clear_dbc(self.h))

    def set_positions(self, V):
        V = np.asfortranarray(V, dtype=np.float64)
        assert V.shape == (self.nV, 3)
        self._chk(self._L.ipcgpu_set_positions(self.h, _dp(V)))

    def get_positions(self):
        V = np.zeros((self.nV, 3), order="F")
        self._chk(self._L.ipcgpu_get_positions(self.h, _dp(V)))
        return V

    def set_xtilde(self, V):
        V = np.asfortranarray(V, dtype=np.float64)
        self._chk(self._L.ipcgpu_set_xtilde(self.h, _dp(V)))

    def features(self):
        A = np.zeros((self.nT, 9))
        vol = np.zeros(self.nT)
        mass = np.zeros(self.nV)
        mu = np.zeros(self.nT)
        lam = np.zeros(self.nT)
        self._chk(self._L.ipcgpu_get_features(self.h, _dp(A), _dp(vol), _dp(mass), _dp(mu), _dp(lam)))
        return dict(restTriInv=A, triArea=vol, mass=mass, mu=mu, lam=lam)

    def check_inversion(self):
        ok = C.c_int()
        self._chk(self._L.ipcgpu_check_inversion(self.h, C.byref(ok)))
        return bool(ok.value)

    # ---- Energy
    def elastic_energy(self, coef=1.0):
        E = C.c_double()
        self._chk(self._L.ipcgpu_elastic_energy(self.h, C.c_double(coef), C.byref(E)))
        return E.value

    def elastic_energy_per_elem(self):
        out = np.zeros(self.nT)
        self._chk(self._L.ipcgpu_elastic_energy_per_elem(self.h, _dp(out)))
        return out

    def elastic_stress(self, nodal=True):
        """Cauchy stress fields of the current positions (ipcgpu_elastic_stress): (elem[nT, 8], node[nV, 8] or None, n_invalid).  Columns: sxx, syy,
        szz, sxy, syz, sxz, von Mises, then J per element / the sum of the incident rest volumes per node.  An NH element with J <= 0 is NaN and
        counted in n_invalid; the stress entries of its four nodes are NaN too."""
        elem = np.zeros((self.nT, 8), order="F")
        node = np.zeros((self.nV, 8), order="F") if nodal else None
        n = C.c_int()
        self._chk(self._L.ipcgpu_elastic_stress(self.h, _dp(elem), _dp(node), C.byref(n)))
        return elem, node, n.value

    def elastic_gradient(self, coef=1.0, projectDBC=True):
        g = np.zeros(3 * self.nV)
        self._chk(self._L.ipcgpu_elastic_gradient(self.h, C.c_double(coef), C.c_int(int(projectDBC)), _dp(g)))
        return g

    def elastic_hessian_add(self, coef=1.0, projectDBC=True):
        self._chk(self._L.ipcgpu_elastic_hessian_add(self.h, C.c_double(coef), C.c_int(int(projectDBC))))

    def filter_step_size(self, p, step=1.0):
        p = _f64(p)
        s = C.c_double(step)
        self._chk(self._L.ipcgpu_filter_step_size(self.h, _dp(p), C.byref(s)))
        return s.value

    # ---- LinSysSolver
    def set_pattern(self, extra_pairs=None):
        if extra_pairs is None or len(extra_pairs) == 0:
            self._chk(self._L.ipcgpu_linsys_set_pattern(self.h, C.c_int(0), None))
        else:
            e = _i32(extra_pairs)
            self._chk(self._L.ipcgpu_linsys_set_pattern(self.h, C.c_int(e.shape[0]), _ip(e)))

    def set_pattern_csr(self, ia, ja):
        ia, ja = _i32(ia), _i32(ja)
        self._chk(self._L.ipcgpu_linsys_set_pattern_csr(self.h, C.c_int(len(ia) - 1), _ip(ia), _ip(ja)))

    def get_dims(self):
        n, nnz = C.c_int(), C.c_int()
        self._chk(self._L.ipcgpu_linsys_get_dims(self.h, C.byref(n), C.byref(nnz)))
        return n.value, nnz.value

    def get_pattern(self):
        n, nnz = self.get_dims()
        ia = np.zeros(n + 1, dtype=np.int32)
        ja = np.zeros(nnz, dtype=np.int32)
        self._chk(self._L.ipcgpu_linsys_get_pattern(self.h, _ip(ia), _ip(ja)))
        return ia, ja

    def set_zero(self):
        self._chk(self._L.ipcgpu_linsys_set_zero(self.h))

    def get_a(self):
        _, nnz = self.get_dims()
        a = np.zeros(nnz)
        self._chk(self._L.ipcgpu_linsys_get_values(self.h, _dp(a)))
        return a

    def set_a(self, a):
        a = _f64(a)
        self._chk(self._L.ipcgpu_linsys_set_values(self.h, _dp(a)))

    def add_coeff(self, r, c, v):
        self._chk(self._L.ipcgpu_linsys_add_coeff(self.h, C.c_int(r), C.c_int(c), C.c_double(v)))

    def set_coeff(self, r, c, v):
        self._chk(self._L.ipcgpu_linsys_set_coeff(self.h, C.c_int(r), C.c_int(c), C.c_double(v)))

    def multiply(self, x):
        x = _f64(x)
        y = np.zeros_like(x)
        self._chk(self._L.ipcgpu_linsys_multiply(self.h, _dp(x), _dp(y)))
        return y

    def multiply_sym(self, x):
        """the iterative solver's product: no atomics, the same bits on every run (ipcgpu_linsys_multiply_sym)"""
        x = _f64(x)
        y = np.zeros_like(x)
        self._chk(self._L.ipcgpu_linsys_multiply_sym(self.h, _dp(x), _dp(y)))
        return y

    def set_iterative(self, rel_tol=1e-5, max_iter=1000, precond=PRECOND_BLOCK_JACOBI, max_factor_age=1):
        """parameters of solver type 2 (ipcgpu_linsys_set_iterative); the defaults are the library's"""
        self._chk(self._L.ipcgpu_linsys_set_iterative(self.h, C.c_double(rel_tol), C.c_int(max_iter), C.c_int(precond), C.c_int(max_factor_age)))

    def iter_stats(self):
        """of the last solve of solver type 2 (ipcgpu_linsys_iter_stats)"""
        o = np.zeros(6)
        self._chk(self._L.ipcgpu_linsys_iter_stats(self.h, _dp(o)))
        return dict(iterations=int(o[0]), residual=float(o[1]), converged=int(o[2]), factorizations=int(o[3]), factor_age=int(o[4]), syncs=int(o[5]))

    def coarse_stats(self):
        """the coarse level of PRECOND_TWO_LEVEL (ipcgpu_linsys_coarse_stats)"""
        o = np.zeros(5)
        self._chk(self._L.ipcgpu_linsys_coarse_stats(self.h, _dp(o)))
        return dict(aggregates=int(o[0]), coarse_rows=int(o[1]), coarse_nnz=int(o[2]), coarse_factorizations=int(o[3]), jacobi_fallbacks=int(o[4]))

    def coarse_dims(self):
        """(aggregates, coarse rows, coarse nnz); zeros without a coarse level"""
        a, r, z = C.c_int(), C.c_int(), C.c_int()
        self._chk(self._L.ipcgpu_linsys_coarse_dims(self.h, C.byref(a), C.byref(r), C.byref(z)))
        return a.value, r.value, z.value

    def coarse_get(self, values=True):
        """(aggregate of every node, coarse ia, coarse ja, coarse values or None): the hierarchy of PRECOND_TWO_LEVEL as the last analyze_pattern /
        factorize left it (ipcgpu_linsys_coarse_get)"""
        _, rows, nnz = self.coarse_dims()
        n, _ = self.get_dims()
        agg = np.zeros(n // 3, dtype=np.int32)
        cia, cja = np.zeros(rows + 1, dtype=np.int32), np.zeros(nnz, dtype=np.int32)
        ca = np.zeros(nnz) if values else None
        self._chk(self._L.ipcgpu_linsys_coarse_get(self.h, _ip(agg), _ip(cia), _ip(cja), _dp(ca)))
        return agg, cia, cja, ca

    def analyze_pattern(self):
        self._chk(self._L.ipcgpu_linsys_analyze_pattern(self.h))

    def factorize(self):
        """Returns True when the matrix is positive definite (LinSysSolver::factorize)."""
        return self._chk(self._L.ipcgpu_linsys_factorize(self.h), allow_not_pd=True) == IPCGPU_OK

    def solve(self, rhs):
        rhs = _f64(rhs)
        x = np.zeros_like(rhs)
        self._chk(self._L.ipcgpu_linsys_solve(self.h, _dp(rhs), _dp(x)))
        return x

    def precondition_diag(self, v):
        v = _f64(v)
        out = np.zeros_like(v)
        self._chk(self._L.ipcgpu_linsys_precondition_diag(self.h, _dp(v), _dp(out)))
        return out

    def set_solver_tuning(self, bulk_min_mb=48.0, bulk_block=256):
        self._chk(self._L.ipcgpu_linsys_set_tuning(self.h, C.c_double(bulk_min_mb), C.c_int(bulk_block)))

    def linsys_stats(self):
        st = np.zeros(4)
        self._chk(self._L.ipcgpu_linsys_stats(self.h, _dp(st)))
        return dict(nnzL=st[0], flops=st[1], fronts=int(st[2]), levels=int(st[3]))

    # ---- SelfCollisionHandler
    def set_surface(self, SF, codim_edges=None):
        """codim_edges: n x 2 node pairs of `.seg` shapes (Mesh::CE); nodes without any neighbour count as `.pt` points"""
        SF = np.asfortranarray(np.asarray(SF, dtype=np.int32).reshape(-1, 3))
        if codim_edges is None or len(codim_edges) == 0:
            self._chk(self._L.ipcgpu_set_surface(self.h, C.c_int(SF.shape[0]), _ip(SF)))
            return
        CE = np.ascontiguousarray(codim_edges, dtype=np.int32).reshape(-1, 2)
        self._chk(self._L.ipcgpu_set_surface_codim(self.h, C.c_int(SF.shape[0]), _ip(SF), C.c_int(CE.shape[0]), _ip(CE)))

    def set_exact_predicates(self, on=True):
        """intersection checks as a USE_PREDICATES build of the reference makes them (exact orient3d)"""
        self._chk(self._L.ipcgpu_set_exact_predicates(self.h, C.c_int(int(on))))

    def set_codim_nodes(self, ids, mass):
        """Surface-only nodes that belong to the mesh (triangle meshes under `shapes`) with their lumped area masses; like a MeshCO they
        stay out of the bounding box behind dHat and of the mean nodal mass behind kappa (matSpaceBBoxSize2(dim) / avgNodeMass(dim))."""
        ids = _i32(ids)
        m = _f64(np.asarray(mass, dtype=np.float64))
        self._chk(self._L.ipcgpu_set_codim_nodes(self.h, C.c_int(len(ids)), _ip(ids), _dp(m)))

    # ---- what the methods of the codimensional energies (shell_*, shell_limit_*, rod_*) share: `term` is the middle of the entry point's name
    def _codim_energy(self, term, coef):
        e = C.c_double()
        self._chk(getattr(self._L, f"ipcgpu_{term}_energy")(self.h, C.c_double(coef), C.byref(e)))
        return e.value

    def _codim_gradient_add(self, term, coef, projectDBC, grad):
        g = np.zeros(3 * self.nV) if grad is None else _f64(grad).copy()
        self._chk(getattr(self._L, f"ipcgpu_{term}_gradient_add")(self.h, C.c_double(coef), C.c_int(int(projectDBC)), _dp(g)))
        return g

    def _codim_hessian_add(self, term, coef, projectDBC):
        self._chk(getattr(self._L, f"ipcgpu_{term}_hessian_add")(self.h, C.c_double(coef), C.c_int(int(projectDBC))))

    # ---- elastic shells (ipcgpu_set_shell: membrane + bending energy on triangle components)
    def set_shell(self, tri, thickness, YM, PR, rho, bend_scale=1.0):
        """tri: nTri x 3 node ids; thickness, YM, PR, rho: scalars or one value per triangle.  After set_mesh, before opt_init and set_pattern; sets the
        masses of the shell nodes and marks them as element nodes.  An empty `tri` removes the shell."""
        tri = np.asfortranarray(np.asarray(tri, dtype=np.int32).reshape(-1, 3))
        n = tri.shape[0]
        per = [_f64(np.broadcast_to(np.asarray(a, dtype=np.float64), (n,))) for a in (thickness, YM, PR, rho)]
        self._chk(self._L.ipcgpu_set_shell(self.h, C.c_int(n), _ip(tri), _dp(per[0]), _dp(per[1]), _dp(per[2]), _dp(per[3]), C.c_double(bend_scale)))

    def shell_get(self):
        """dict: nTri, nHinge, hinges (nHinge x 4: x0, x1 on the edge, x2, x3 opposite), restAngle, hingeWeight, area, mass (nV)"""
        cnt = np.zeros(2, dtype=np.int32)
        self._chk(self._L.ipcgpu_shell_get(self.h, _ip(cnt), None, None, None, None, None))
        nTri, nH = int(cnt[0]), int(cnt[1])
        hinges = np.zeros((nH, 4), dtype=np.int32)
        rest, w, area, mass = np.zeros(nH), np.zeros(nH), np.zeros(nTri), np.zeros(self.nV)
        self._chk(self._L.ipcgpu_shell_get(self.h, _ip(cnt), _ip(hinges), _dp(rest), _dp(w), _dp(area), _dp(mass)))
        return {"nTri": nTri, "nHinge": nH, "hinges": hinges, "restAngle": rest, "hingeWeight": w, "area": area, "mass": mass}

    def shell_energy(self, coef=1.0):
        return self._codim_energy("shell", coef)

    def shell_energy_per_elem(self):
        cnt = np.zeros(2, dtype=np.int32)
        self._chk(self._L.ipcgpu_shell_get(self.h, _ip(cnt), None, None, None, None, None))
        t, h = np.zeros(int(cnt[0])), np.zeros(int(cnt[1]))
        self._chk(self._L.ipcgpu_shell_energy_per_elem(self.h, _dp(t), _dp(h)))
        return t, h

    def shell_gradient_add(self, coef=1.0, projectDBC=True, grad=None):
        """grad (3 nV, xyz interleaved; zeros when None) += coef * shell gradient; returns it"""
        return self._codim_gradient_add("shell", coef, projectDBC, grad)

    def shell_hessian_add(self, coef=1.0, projectDBC=True):
        self._codim_hessian_add("shell", coef, projectDBC)

    # ---- strain limit of the shell (ipcgpu_shell_set_strain_limit: a log barrier on the principal stretches of the limited triangles)
    def _shell_ntri(self):
        cnt = np.zeros(2, dtype=np.int32)
        self._chk(self._L.ipcgpu_shell_get(self.h, _ip(cnt), None, None, None, None, None))
        return int(cnt[0])

    def set_shell_strain_limit(self, limit, onset=None, stiff=None):
        """limit, onset (None: 1), stiff (None: 1): scalars or one value per shell triangle; limit 0 leaves a triangle unlimited, None or all zeros removes the
        term.  After set_shell; set_shell and set_mesh drop it."""
        n = self._shell_ntri()
        per = [None if a is None else _f64(np.broadcast_to(np.asarray(a, dtype=np.float64), (n,))) for a in (limit, onset, stiff)]
        self._chk(self._L.ipcgpu_shell_set_strain_limit(self.h, _dp(per[0]), _dp(per[1]), _dp(per[2])))

    def shell_limit_energy(self, coef=1.0):
        return self._codim_energy("shell_limit", coef)

    def shell_limit_energy_per_elem(self):
        """the unscaled barrier energy per shell triangle (0 for an unlimited one, inf at or over the limit)"""
        t = np.zeros(self._shell_ntri())
        self._chk(self._L.ipcgpu_shell_limit_energy_per_elem(self.h, _dp(t)))
        return t

    def shell_limit_gradient_add(self, coef=1.0, projectDBC=True, grad=None):
        """grad (3 nV, xyz interleaved; zeros when None) += coef * gradient of the limit term; returns it"""
        return self._codim_gradient_add("shell_limit", coef, projectDBC, grad)

    def shell_limit_hessian_add(self, coef=1.0, projectDBC=True):
        self._codim_hessian_add("shell_limit", coef, projectDBC)

    def shell_stretch(self):
        """(sigma (nTri x 2: the principal stretches sigma1 >= sigma2 of every shell triangle), the maximum of sigma1 / limit over the limited triangles --
        0 without one)"""
        s = np.zeros((self._shell_ntri(), 2))
        r = C.c_double()
        self._chk(self._L.ipcgpu_shell_stretch(self.h, _dp(s), C.byref(r)))
        return s, r.value

    # ---- rubber membrane of the shell (ipcgpu_shell_set_membrane: incompressible Mooney-Rivlin on the chosen triangles, in place of their StVK membrane)
    def set_shell_membrane(self, model, alpha=None):
        """model: 0 (StVK) or 1 (rubber), alpha (None: 0; 0 <= alpha < 1, the Mooney-Rivlin fraction): scalars or one value per shell triangle; None or all
        zeros removes the term.  After set_shell; set_shell and set_mesh drop it."""
        n = self._shell_ntri()
        m = None if model is None else np.ascontiguousarray(np.broadcast_to(np.asarray(model, dtype=np.int32), (n,)))
        a = None if alpha is None else _f64(np.broadcast_to(np.asarray(alpha, dtype=np.float64), (n,)))
        self._chk(self._L.ipcgpu_shell_set_membrane(self.h, _ip(m), _dp(a)))

    def shell_membrane_get(self):
        """(model (nTri, int32), alpha (nTri)) as set; zeros without a rubber triangle"""
        n = self._shell_ntri()
        m, a = np.zeros(n, dtype=np.int32), np.zeros(n)
        self._chk(self._L.ipcgpu_shell_membrane_get(self.h, _ip(m), _dp(a)))
        return m, a

    def shell_rubber_energy(self, coef=1.0):
        return self._codim_energy("shell_rubber", coef)

    def shell_rubber_energy_per_elem(self):
        """the unscaled rubber energy per shell triangle (0 for a StVK one, inf for a degenerate rubber one)"""
        t = np.zeros(self._shell_ntri())
        self._chk(self._L.ipcgpu_shell_rubber_energy_per_elem(self.h, _dp(t)))
        return t

    def shell_rubber_gradient_add(self, coef=1.0, projectDBC=True, grad=None):
        """grad (3 nV, xyz interleaved; zeros when None) += coef * gradient of the rubber term; returns it"""
        return self._codim_gradient_add("shell_rubber", coef, projectDBC, grad)

    def shell_rubber_hessian_add(self, coef=1.0, projectDBC=True):
        self._codim_hessian_add("shell_rubber", coef, projectDBC)

    def shell_thickness(self):
        """the current thickness per shell triangle: h / (sigma1 sigma2) on a rubber triangle, the rest thickness on a StVK one"""
        h = np.zeros(self._shell_ntri())
        self._chk(self._L.ipcgpu_shell_thickness(self.h, _dp(h)))
        return h

    # ---- woven cloth of the shell (ipcgpu_shell_set_weave: an orthotropic StVK membrane and direction-dependent bending on the chosen triangles)
    def set_shell_weave(self, woven, direction=None, E1=None, E2=None, G12=None, nu12=None, bend_warp=None, bend_weft=None):
        """woven: 0 or 1; direction: one 3-vector of rest space or one per shell triangle (projected into each triangle's rest plane: the warp); E1 (warp), E2
        (weft), G12 (shear), nu12 (None: 0), bend_warp, bend_weft (None: 1): scalars or one value per shell triangle; woven None or all zeros removes the term.
        After set_shell, also between time steps; set_shell and set_mesh drop it."""
        n = self._shell_ntri()
        w = None if woven is None else np.ascontiguousarray(np.broadcast_to(np.asarray(woven, dtype=np.int32), (n,)))
        d = None if direction is None else _f64(np.broadcast_to(np.asarray(direction, dtype=np.float64), (n, 3)))
        per = [None if a is None else _f64(np.broadcast_to(np.asarray(a, dtype=np.float64), (n,))) for a in (E1, E2, G12, nu12, bend_warp, bend_weft)]
        self._chk(self._L.ipcgpu_shell_set_weave(self.h, _ip(w), _dp(d), *[_dp(a) for a in per]))

    def shell_weave_get(self):
        """dict: woven (nTri, int32), a (nTri x 2: the unit warp direction in each triangle's rest frame), const4 (nTri x 4: C11, C12, C22, G12), hingeFactor
        (nHinge); zeros (ones for hingeFactor) without a woven triangle"""
        n, nH = self._shell_counts()
        w, a, c4, hf = np.zeros(n, dtype=np.int32), np.zeros((n, 2)), np.zeros((n, 4)), np.ones(nH)
        self._chk(self._L.ipcgpu_shell_weave_get(self.h, _ip(w), _dp(a), _dp(c4), _dp(hf)))
        return {"woven": w, "a": a, "const4": c4, "hingeFactor": hf}

    def shell_weave_energy(self, coef=1.0):
        return self._codim_energy("shell_weave", coef)

    def shell_weave_energy_per_elem(self):
        """the unscaled woven energy per shell triangle (0 for one that is not woven)"""
        t = np.zeros(self._shell_ntri())
        self._chk(self._L.ipcgpu_shell_weave_energy_per_elem(self.h, _dp(t)))
        return t

    def shell_weave_gradient_add(self, coef=1.0, projectDBC=True, grad=None):
        """grad (3 nV, xyz interleaved; zeros when None) += coef * gradient of the woven term; returns it"""
        return self._codim_gradient_add("shell_weave", coef, projectDBC, grad)

    def shell_weave_hessian_add(self, coef=1.0, projectDBC=True):
        self._codim_hessian_add("shell_weave", coef, projectDBC)

    def shell_weave_state(self):
        """nTri x 6 per shell triangle: the warp strain Eww, the weft strain Eff, the shear angle between the yarns (radians) and the current unit warp direction
        (x, y, z); NaN where a yarn direction has length 0, zeros on a triangle that is not woven"""
        s = np.zeros((6, self._shell_ntri()))
        self._chk(self._L.ipcgpu_shell_weave_state(self.h, _dp(s)))
        return np.ascontiguousarray(s.T)

    # ---- plastic flow of the shell (ipcgpu_shell_set_plasticity: permanent stretch, creases and dents; ipc_amd/csrc/shell_plastic_kernels.h)
    def _shell_counts(self):
        cnt = np.zeros(2, dtype=np.int32)
        self._chk(self._L.ipcgpu_shell_get(self.h, _ip(cnt), None, None, None, None, None))
        return int(cnt[0]), int(cnt[1])

    def shell_set_plasticity(self, tri_range, yield_strain, bend_yield=None, creep=np.inf, harden=0.0):
        """shell triangles [tri_range[0], tri_range[1]): the membrane flows where the deviatoric Hencky strain norm n exceeds yield_strain + harden alpha, a hinge
        between two such triangles where its outer-fibre strain g |theta - thetaBar| exceeds bend_yield + harden alphaB (None: yield_strain); the excess decays like
        exp(-creep t) (inf: returned at once); inf switches a flow off.  After set_shell, also between time steps; later calls overwrite."""
        yb = yield_strain if bend_yield is None else bend_yield
        self._chk(self._L.ipcgpu_shell_set_plasticity(self.h, C.c_int(tri_range[0]), C.c_int(tri_range[1]), C.c_double(yield_strain), C.c_double(yb), C.c_double(creep), C.c_double(harden)))

    def shell_plastic_get(self):
        """dict: yield, bendYield, creep, harden, alpha (nTri each), triConst (nTri x 6, the current constants the kernels read: B = columns 0-3 as b00 b10 b01
        b11, then h A mu, h A lambda_ps), B0 (nTri x 4), hingeYield, hingeCreep, hingeHarden, g, alphaB, thetaBar (current), thetaBar0 (nHinge each)"""
        nT, nH = self._shell_counts()
        y, yb, cr, K, al = (np.zeros(nT) for _ in range(5))
        tc, B0, hp = np.zeros((nT, 6), order="F"), np.zeros((nT, 4), order="F"), np.zeros((nH, 4), order="F")
        alB, th, th0 = np.zeros(nH), np.zeros(nH), np.zeros(nH)
        self._chk(self._L.ipcgpu_shell_plastic_get(self.h, _dp(y), _dp(yb), _dp(cr), _dp(K), _dp(al), _dp(tc), _dp(B0), _dp(hp), _dp(alB), _dp(th), _dp(th0)))
        return {"yield": y, "bendYield": yb, "creep": cr, "harden": K, "alpha": al, "triConst": tc, "B": tc[:, :4].copy(), "B0": B0, "hingeYield": hp[:, 0].copy(),
                "hingeCreep": hp[:, 1].copy(), "hingeHarden": hp[:, 2].copy(), "g": hp[:, 3].copy(), "alphaB": alB, "thetaBar": th, "thetaBar0": th0}

    def shell_plastic_update(self, dt):
        """one flow of the membrane and of the hinges at the held positions, outside the stepper: (triangles that yielded, triangles skipped as collapsed,
        hinges that yielded, hinges skipped as degenerate)"""
        cnt = np.zeros(4, dtype=np.int32)
        self._chk(self._L.ipcgpu_shell_plastic_update(self.h, C.c_double(dt), _ip(cnt)))
        return tuple(int(v) for v in cnt)

    def shell_plastic_state(self):
        """(perTri nTri x 4: n, current yield strain y, alpha, det B0 / det B -- n is NaN where the flow would skip the triangle; perHinge nHinge x 4: eps, y,
        alphaB, thetaBar - thetaBar0; totals 7: the four counts of the last flow, max alpha, max alphaB, sum of h A alpha).  Read-only."""
        nT, nH = self._shell_counts()
        pt, ph, tot = np.zeros((nT, 4), order="F"), np.zeros((nH, 4), order="F"), np.zeros(7)
        self._chk(self._L.ipcgpu_shell_plastic_state(self.h, _dp(pt), _dp(ph), _dp(tot)))
        return pt, ph, tot

    def shell_plastic_set_state(self, B=None, alpha=None, thetaBar=None, alphaB=None):
        """the current B (nTri x 4: b00 b10 b01 b11 per row), alpha (nTri), thetaBar and alphaB (nHinge) from the caller; None leaves a part as it is"""
        nT, nH = self._shell_counts()
        Bf = None if B is None else np.asfortranarray(np.asarray(B, dtype=np.float64).reshape(nT, 4))
        al = None if alpha is None else _f64(np.asarray(alpha, dtype=np.float64).reshape(nT))
        th = None if thetaBar is None else _f64(np.asarray(thetaBar, dtype=np.float64).reshape(nH))
        ab = None if alphaB is None else _f64(np.asarray(alphaB, dtype=np.float64).reshape(nH))
        self._chk(self._L.ipcgpu_shell_plastic_set_state(self.h, _dp(Bf), _dp(al), _dp(th), _dp(ab)))

    def shell_plastic_reset(self):
        """forget the shell's plastic history: B and thetaBar of the first shell_set_plasticity call, alpha = alphaB = 0"""
        self._chk(self._L.ipcgpu_shell_plastic_reset(self.h))

    # ---- elastic rods (ipcgpu_set_rod: stretching + bending energy on segment components)
    def set_rod(self, seg, radius, YM, rho, bend_scale=1.0):
        """seg: nSeg x 2 node ids; radius, YM, rho: scalars or one value per segment.  After set_mesh, before opt_init and set_pattern; sets the masses of
        the rod nodes and marks them as element nodes.  Collision still needs the segments in set_surface.  An empty `seg` removes the rod."""
        seg = np.asfortranarray(np.asarray(seg, dtype=np.int32).reshape(-1, 2))
        n = seg.shape[0]
        per = [_f64(np.broadcast_to(np.asarray(a, dtype=np.float64), (n,))) for a in (radius, YM, rho)]
        self._chk(self._L.ipcgpu_set_rod(self.h, C.c_int(n), _ip(seg), _dp(per[0]), _dp(per[1]), _dp(per[2]), C.c_double(bend_scale)))

    def rod_get(self):
        """dict: nSeg, nBend, bend (nBend x 3: a, b, c with b the interior node), restLen, ks (per segment), kb, restKb (per triple), mass (nV)"""
        cnt = np.zeros(2, dtype=np.int32)
        self._chk(self._L.ipcgpu_rod_get(self.h, _ip(cnt), None, None, None, None, None, None))
        nSeg, nB = int(cnt[0]), int(cnt[1])
        bend = np.zeros((nB, 3), dtype=np.int32)
        L, ks, kb, rest, mass = np.zeros(nSeg), np.zeros(nSeg), np.zeros(nB), np.zeros(nB), np.zeros(self.nV)
        self._chk(self._L.ipcgpu_rod_get(self.h, _ip(cnt), _ip(bend), _dp(L), _dp(ks), _dp(kb), _dp(rest), _dp(mass)))
        return {"nSeg": nSeg, "nBend": nB, "bend": bend, "restLen": L, "ks": ks, "kb": kb, "restKb": rest, "mass": mass}

    def rod_energy(self, coef=1.0):
        return self._codim_energy("rod", coef)

    def rod_energy_per_elem(self):
        cnt = np.zeros(2, dtype=np.int32)
        self._chk(self._L.ipcgpu_rod_get(self.h, _ip(cnt), None, None, None, None, None, None))
        t, h = np.zeros(int(cnt[0])), np.zeros(int(cnt[1]))
        self._chk(self._L.ipcgpu_rod_energy_per_elem(self.h, _dp(t), _dp(h)))
        return t, h

    def rod_gradient_add(self, coef=1.0, projectDBC=True, grad=None):
        """grad (3 nV, xyz interleaved; zeros when None) += coef * rod gradient; returns it"""
        return self._codim_gradient_add("rod", coef, projectDBC, grad)

    def rod_hessian_add(self, coef=1.0, projectDBC=True):
        self._codim_hessian_add("rod", coef, projectDBC)

    # ---- attachments (ipcgpu_set_attachments: springs that tie a point of the mesh to another -- stitches and tethers)
    @staticmethod
    def _attach_points(nodes, weights, n):
        """nodes: n ids or n x (1 .. 3) ids (-1: unused slot); weights: None (one node per point, weight 1) or the same shape -> (n x 3 ids, n x 3 weights)"""
        ids = np.asarray(nodes, dtype=np.int32).reshape(n, -1)
        if ids.shape[1] > 3:
            raise ValueError("set_attachments: a point has at most three nodes")
        if weights is None:
            if ids.shape[1] != 1:
                raise ValueError("set_attachments: points of more than one node need weights")
            w = np.ones((n, 1))
        else:
            w = np.asarray(weights, dtype=np.float64).reshape(n, -1)
            if w.shape != ids.shape:
                raise ValueError("set_attachments: one weight per node slot")
        N, W = np.full((n, 3), -1, dtype=np.int32), np.zeros((n, 3))
        N[:, :ids.shape[1]], W[:, :ids.shape[1]] = ids, w
        return np.ascontiguousarray(N), np.ascontiguousarray(W)

    def set_attachments(self, nodesA, nodesB, k, L=0.0, weightsA=None, weightsB=None):
        """Ties point A to point B of every attachment with W = k (|d| - L)^2 / 2, d = A - B.  nodesA / nodesB: n node ids, or n x (1 .. 3) ids with
        weightsA / weightsB of the same shape (>= 0, sum 1; id -1 with weight 0: unused slot) for points on edges and in triangles; k, L: scalars or one
        value per attachment.  After set_mesh, before opt_init and set_pattern; changes no mass.  Contact between the attached bodies stays as it is (mask
        it with set_contact_groups, or give a rest length).  An empty list removes the attachments."""
        n = len(np.asarray(nodesA))
        if n == 0:
            self._chk(self._L.ipcgpu_set_attachments(self.h, C.c_int(0), None, None, None, None, None, None))
            return
        NA, WA = self._attach_points(nodesA, weightsA, n)
        NB, WB = self._attach_points(nodesB, weightsB, n)
        kk, LL = (_f64(np.broadcast_to(np.asarray(a, dtype=np.float64), (n,))) for a in (k, L))
        self._chk(self._L.ipcgpu_set_attachments(self.h, C.c_int(n), _ip(NA), _dp(WA), _ip(NB), _dp(WB), _dp(kk), _dp(LL)))

    def _attach_n(self):
        n = C.c_int()
        self._chk(self._L.ipcgpu_attach_get(self.h, C.byref(n), None, None, None, None, None, None))
        return n.value

    def attach_get(self):
        """dict: n, count (distinct nodes per attachment), nodes, coefs (n x 6: merged ids and signed coefficients, padding repeats slot 0 with 0), k, L,
        restDist (the distance of the two points at the rest positions)"""
        n = self._attach_n()
        cnt, nodes, coefs = np.zeros(n, dtype=np.int32), np.zeros((6, n), dtype=np.int32), np.zeros((6, n))
        k, L, rest = np.zeros(n), np.zeros(n), np.zeros(n)
        m = C.c_int()
        self._chk(self._L.ipcgpu_attach_get(self.h, C.byref(m), _ip(cnt), _ip(nodes), _dp(coefs), _dp(k), _dp(L), _dp(rest)))
        return {"n": n, "count": cnt, "nodes": nodes.T.copy(), "coefs": coefs.T.copy(), "k": k, "L": L, "restDist": rest}

    def attach_energy(self, coef=1.0):
        return self._codim_energy("attach", coef)

    def attach_energy_per_elem(self):
        e = np.zeros(self._attach_n())
        self._chk(self._L.ipcgpu_attach_energy_per_elem(self.h, _dp(e)))
        return e

    def attach_gradient_add(self, coef=1.0, projectDBC=True, grad=None):
        """grad (3 nV, xyz interleaved; zeros when None) += coef * attachment gradient; returns it"""
        return self._codim_gradient_add("attach", coef, projectDBC, grad)

    def attach_hessian_add(self, coef=1.0, projectDBC=True):
        self._codim_hessian_add("attach", coef, projectDBC)

    def attach_state(self):
        """(length l, signed force k (l - L)) per attachment at the current positions"""
        n = self._attach_n()
        l, f = np.zeros(n), np.zeros(n)
        self._chk(self._L.ipcgpu_attach_state(self.h, _dp(l), _dp(f)))
        return l, f

    # ---- pressure chambers (ipcgpu_set_chambers: a constant gas pressure inside closed surfaces)
    def set_chambers(self, tri_lists, pressures):
        """tri_lists: one m x 3 array of node ids per chamber -- a closed surface (or several), consistently oriented, outward by the right-hand rule --,
        pressures: one gauge pressure per chamber (positive pushes outward).  W = -p V per chamber, a follower load.  After set_mesh, before opt_init
        and set_pattern; changes no mass.  An empty list removes the chambers."""
        lists = [np.asarray(t, dtype=np.int32).reshape(-1, 3) for t in tri_lists]
        if len(lists) == 0:
            self._chk(self._L.ipcgpu_set_chambers(self.h, C.c_int(0), None, None, None))
            return
        p = _f64(np.broadcast_to(np.asarray(pressures, dtype=np.float64), (len(lists),)))
        end = _i32(np.cumsum([len(t) for t in lists]))
        tri = np.asfortranarray(np.vstack(lists), dtype=np.int32)
        self._chk(self._L.ipcgpu_set_chambers(self.h, C.c_int(len(lists)), _ip(end), _ip(tri), _dp(p)))

    def chamber_set_pressure(self, pressures):
        """new pressures (a scalar or one per chamber), at any time, also between time steps"""
        p = _f64(np.broadcast_to(np.asarray(pressures, dtype=np.float64), (self._chamber_counts()[0],)))
        self._chk(self._L.ipcgpu_chamber_set_pressure(self.h, _dp(p)))

    def _chamber_counts(self):
        cnt = np.zeros(2, dtype=np.int32)
        self._chk(self._L.ipcgpu_chamber_get(self.h, _ip(cnt), None, None, None, None))
        return int(cnt[0]), int(cnt[1])

    def chamber_get(self):
        """dict: n (chambers), nTri, triEnd, tri (nTri x 3, as given), restVolume, pressure"""
        n, nTri = self._chamber_counts()
        cnt, end, tri = np.zeros(2, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros((nTri, 3), dtype=np.int32, order="F")
        rest, p = np.zeros(n), np.zeros(n)
        self._chk(self._L.ipcgpu_chamber_get(self.h, _ip(cnt), _ip(end), _ip(tri), _dp(rest), _dp(p)))
        return {"n": n, "nTri": nTri, "triEnd": end, "tri": np.ascontiguousarray(tri), "restVolume": rest, "pressure": p}

    def chamber_state(self):
        """(volume, area, refPoint n x 3) per chamber at the current positions; refPoint is the r_c the evaluations use now"""
        n = self._chamber_counts()[0]
        v, a, r = np.zeros(n), np.zeros(n), np.zeros((n, 3))
        self._chk(self._L.ipcgpu_chamber_state(self.h, _dp(v), _dp(a), _dp(r)))
        return v, a, r

    def chamber_energy(self, coef=1.0):
        return self._codim_energy("chamber", coef)

    def chamber_energy_per_elem(self):
        e = np.zeros(self._chamber_counts()[1])
        self._chk(self._L.ipcgpu_chamber_energy_per_elem(self.h, _dp(e)))
        return e

    def chamber_gradient_add(self, coef=1.0, projectDBC=True, grad=None):
        """grad (3 nV, xyz interleaved; zeros when None) += coef * chamber gradient; returns it"""
        return self._codim_gradient_add("chamber", coef, projectDBC, grad)

    def chamber_hessian_add(self, coef=1.0, projectDBC=True):
        """the sparse part only: a gas chamber's rank-one term beta gradV gradV^T lives in chamber_gas_solve and the stepper"""
        self._codim_hessian_add("chamber", coef, projectDBC)

    # ---- wind and air drag (ipcgpu_set_aero: a drag load on triangle surfaces that depends on their normal and their velocity against the air)
    def set_aero(self, tri_lists, cn=1.28, ct=0.0, one_sided=False):
        """tri_lists: one m x 3 array of node ids per surface (shell triangles or boundary faces, open or closed); cn, ct, one_sided: a scalar or one value
        per surface.  D = dt (rho_a A / 6) (cn |s_n|^3 + ct |u_t|^3) per triangle, normal, area and start centroid lagged per time step.  After set_mesh,
        before opt_init and set_pattern; changes no mass.  An empty list removes the surfaces."""
        lists = [np.asarray(t, dtype=np.int32).reshape(-1, 3) for t in tri_lists]
        if len(lists) == 0:
            self._chk(self._L.ipcgpu_set_aero(self.h, C.c_int(0), None, None, None, None, None))
            return
        n = len(lists)
        a = _f64(np.broadcast_to(np.asarray(cn, dtype=np.float64), (n,)))
        b = _f64(np.broadcast_to(np.asarray(ct, dtype=np.float64), (n,)))
        o = _i32(np.broadcast_to(np.asarray(one_sided), (n,)).astype(bool))
        end = _i32(np.cumsum([len(t) for t in lists]))
        tri = np.asfortranarray(np.vstack(lists), dtype=np.int32)
        self._chk(self._L.ipcgpu_set_aero(self.h, C.c_int(n), _ip(end), _ip(tri), _dp(a), _dp(b), _ip(o)))

    def aero_set_wind(self, wind=(0.0, 0.0, 0.0), density=1.225):
        """the wind velocity (uniform in space) and the air density, at any time, also between time steps"""
        w = _f64(np.asarray(wind, dtype=np.float64).reshape(3))
        self._chk(self._L.ipcgpu_aero_set_wind(self.h, _dp(w), C.c_double(density)))

    def _aero_counts(self):
        cnt = np.zeros(2, dtype=np.int32)
        self._chk(self._L.ipcgpu_aero_get(self.h, _ip(cnt), None, None, None, None, None, None, None))
        return int(cnt[0]), int(cnt[1])

    def aero_get(self):
        """dict: n (surfaces), nTri, triEnd, tri (nTri x 3, as given), cn, ct, oneSided, wind, density"""
        n, nTri = self._aero_counts()
        cnt, end, tri = np.zeros(2, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros((nTri, 3), dtype=np.int32, order="F")
        cn, ct, one, w, rho = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros(3), C.c_double()
        self._chk(self._L.ipcgpu_aero_get(self.h, _ip(cnt), _ip(end), _ip(tri), _dp(cn), _dp(ct), _ip(one), _dp(w), C.byref(rho)))
        return {"n": n, "nTri": nTri, "triEnd": end, "tri": np.ascontiguousarray(tri), "cn": cn, "ct": ct, "oneSided": one.astype(bool), "wind": w, "density": rho.value}

    def aero_state(self, with_force=True):
        """(force nTri x 3, lagged nTri x 8, total5): the force on every triangle at the current positions, the lagged records (n, A, c^n, 0) the evaluations
        use now, and the total force (3), the dissipated power and the loaded area.  with_force=False: the lagged records alone (allowed before opt_init)."""
        nTri = self._aero_counts()[1]
        f, lag, tot = np.zeros((nTri, 3)), np.zeros((nTri, 8)), np.zeros(5)
        self._chk(self._L.ipcgpu_aero_state(self.h, _dp(f) if with_force else None, _dp(lag), _dp(tot) if with_force else None))
        return f, lag, tot

    def aero_energy(self, coef=1.0):
        return self._codim_energy("aero", coef)

    def aero_energy_per_elem(self):
        e = np.zeros(self._aero_counts()[1])
        self._chk(self._L.ipcgpu_aero_energy_per_elem(self.h, _dp(e)))
        return e

    def aero_gradient_add(self, coef=1.0, projectDBC=True, grad=None):
        """grad (3 nV, xyz interleaved; zeros when None) += coef * air-drag gradient; returns it"""
        return self._codim_gradient_add("aero", coef, projectDBC, grad)

    def aero_hessian_add(self, coef=1.0, projectDBC=True):
        self._codim_hessian_add("aero", coef, projectDBC)

    # ---- fibre reinforcement and active contraction of tetrahedral elements (ipcgpu_set_fibers; ipc_amd/csrc/fiber_kernels.h)
    FIBER_LAWS = {"spring": 0, "exp": 1}
    FIBER_MAX_GROUPS = 64

    def set_fibers(self, tet_range, direction, k, law="spring", k2=0.0, tension_only=False, group=0):
        """elements [tet_range[0], tet_range[1]) get one fibre family along `direction` (3 numbers, or one row per element of the range; rest frame, normalised
        by the call) with stiffness k (a stress; 0 removes the fibres).  law "spring": k (l - l0)^2 / 2 with l0 = 1 - activation of `group`, tension_only
        switches it off for l <= l0; law "exp": k / (2 k2) (exp(k2 (l^2 - 1)^2) - 1) for l > 1.  Any time after set_mesh; later calls overwrite."""
        d = _f64(np.asarray(direction, dtype=np.float64))
        per = d.ndim == 2
        if per and d.shape != (tet_range[1] - tet_range[0], 3) or not per and d.shape != (3,):
            raise ValueError("direction: 3 numbers, or one row of 3 per element of the range")
        self._chk(self._L.ipcgpu_set_fibers(self.h, C.c_int(tet_range[0]), C.c_int(tet_range[1]), _dp(d), C.c_int(int(per)), C.c_double(k),
                                            C.c_int(self.FIBER_LAWS.get(law, law)), C.c_double(k2), C.c_int(int(tension_only)), C.c_int(group)))

    def fiber_set_activation(self, group, act):
        """the activation of one group: the spring fibres of it want the stretch 1 - act (act < 1; 0 is passive)"""
        self._chk(self._L.ipcgpu_fiber_set_activation(self.h, C.c_int(group), C.c_double(act)))

    def fiber_get(self):
        """dict: n (fibred elements), k, k2, law, tensionOnly, group (nT each), dir (nT x 3, unit; zeros without a fibre), act (64)"""
        nT = self.nT
        n = C.c_int()
        k, k2, d, act = np.zeros(nT), np.zeros(nT), np.zeros((nT, 3)), np.zeros(self.FIBER_MAX_GROUPS)
        law, to, grp = np.zeros(nT, dtype=np.int32), np.zeros(nT, dtype=np.int32), np.zeros(nT, dtype=np.int32)
        self._chk(self._L.ipcgpu_fiber_get(self.h, C.byref(n), _dp(k), _dp(k2), _ip(law), _ip(to), _ip(grp), _dp(d), _dp(act)))
        return {"n": n.value, "k": k, "k2": k2, "law": law, "tensionOnly": to, "group": grp, "dir": d, "act": act}

    def fiber_energy(self, coef=1.0):
        return self._codim_energy("fiber", coef)

    def fiber_energy_per_elem(self):
        """W per element (nT; 0 without a fibre)"""
        e = np.zeros(self.nT)
        self._chk(self._L.ipcgpu_fiber_energy_per_elem(self.h, _dp(e)))
        return e

    def fiber_gradient_add(self, coef=1.0, projectDBC=True, grad=None):
        """grad (3 nV, xyz interleaved; zeros when None) += coef * fibre gradient; returns it"""
        return self._codim_gradient_add("fiber", coef, projectDBC, grad)

    def fiber_hessian_add(self, coef=1.0, projectDBC=True):
        self._codim_hessian_add("fiber", coef, projectDBC)

    def fiber_state(self, per_elem=True):
        """(perElem nT x 5: stretch l, tension psi'(l), current direction t -- 1, 0 and 0 0 0 without a fibre; totals: min l, max l, sum of W).  Read-only."""
        pe, tot = np.zeros((self.nT, 5), order="F"), np.zeros(3)
        self._chk(self._L.ipcgpu_fiber_state(self.h, _dp(pe) if per_elem else None, _dp(tot)))
        return (pe if per_elem else None), tot

    # ---- plastic flow of tetrahedral elements (ipcgpu_set_plasticity: yield, creep, isotropic hardening; ipc_amd/csrc/plastic_kernels.h)
    def set_plasticity(self, tet_range, yield_strain, creep=np.inf, harden=0.0):
        """elements [tet_range[0], tet_range[1]) yield where the deviatoric Hencky strain norm n exceeds yield_strain + harden alpha (for small strains the von
        Mises stress is sqrt(6) mu n); the excess decays like exp(-creep t) (inf: returned at once); yield_strain = inf switches the range off.  Any time
        after set_mesh, also between time steps; later calls overwrite."""
        self._chk(self._L.ipcgpu_set_plasticity(self.h, C.c_int(tet_range[0]), C.c_int(tet_range[1]), C.c_double(yield_strain), C.c_double(creep), C.c_double(harden)))

    def plastic_get(self):
        """dict: yield, creep, harden, alpha (nT each), restTriInv0 (nT x 9: the rest shapes plastic_reset restores)"""
        y, cr, K, al, A0 = np.zeros(self.nT), np.zeros(self.nT), np.zeros(self.nT), np.zeros(self.nT), np.zeros((self.nT, 9))
        self._chk(self._L.ipcgpu_plastic_get(self.h, _dp(y), _dp(cr), _dp(K), _dp(al), _dp(A0)))
        return {"yield": y, "creep": cr, "harden": K, "alpha": al, "restTriInv0": A0}

    def plastic_update(self, dt):
        """one flow at the held positions, outside the stepper: (elements that yielded, elements skipped as flat or inverted)"""
        ny, ns = C.c_int(), C.c_int()
        self._chk(self._L.ipcgpu_plastic_update(self.h, C.c_double(dt), C.byref(ny), C.byref(ns)))
        return ny.value, ns.value

    def plastic_state(self, per_elem=True):
        """(perElem nT x 3: n, current yield strain y, alpha -- n is NaN where the flow would skip the element; totals: yielded and skipped in the last flow,
        max alpha, sum of rest volume x alpha).  Read-only."""
        pe, tot = np.zeros((self.nT, 3), order="F"), np.zeros(4)
        self._chk(self._L.ipcgpu_plastic_state(self.h, _dp(pe) if per_elem else None, _dp(tot)))
        return (pe if per_elem else None), tot

    def plastic_set_state(self, restTriInv=None, alpha=None):
        """the current rest shapes (nT x 9, as features()['restTriInv']) and / or the accumulated plastic strain (nT) from the caller"""
        A = None if restTriInv is None else _f64(np.asarray(restTriInv, dtype=np.float64).reshape(self.nT, 9))
        al = None if alpha is None else _f64(np.asarray(alpha, dtype=np.float64).reshape(self.nT))
        self._chk(self._L.ipcgpu_plastic_set_state(self.h, _dp(A), _dp(al)))

    def plastic_reset(self):
        """forget the plastic history: the rest shapes of the first set_plasticity call, alpha = 0"""
        self._chk(self._L.ipcgpu_plastic_reset(self.h))

    # ---- the gas law of the chambers (ipcgpu_chamber_set_gas)
    def chamber_set_gas(self, is_gas, ambient=0.0, gamma=1.0, fill_volume=None):
        """per chamber (scalars broadcast): is_gas (False: constant pressure), the ambient absolute pressure, the exponent gamma (1 isothermal, 1.4 adiabatic
        air) and the fill volume (None or <= 0: the rest volume).  The chamber's pressure becomes the gauge pressure at the fill volume.  After set_chambers,
        at any time; all False restores the constant chambers exactly."""
        n = self._chamber_counts()[0]
        g = _i32(np.broadcast_to(np.asarray(is_gas).astype(np.int32), (n,)))
        a = _f64(np.broadcast_to(np.asarray(ambient, dtype=np.float64), (n,)))
        k = _f64(np.broadcast_to(np.asarray(gamma, dtype=np.float64), (n,)))
        f = None if fill_volume is None else _f64(np.broadcast_to(np.asarray(fill_volume, dtype=np.float64), (n,)))
        self._chk(self._L.ipcgpu_chamber_set_gas(self.h, _ip(g), _dp(a), _dp(k), _dp(f)))

    def chamber_gas_get(self):
        """dict: isGas, ambient, gamma, fillVolume per chamber"""
        n = self._chamber_counts()[0]
        g, a, k, f = np.zeros(n, dtype=np.int32), np.zeros(n), np.zeros(n), np.zeros(n)
        self._chk(self._L.ipcgpu_chamber_gas_get(self.h, _ip(g), _dp(a), _dp(k), _dp(f)))
        return {"isGas": g, "ambient": a, "gamma": k, "fillVolume": f}

    def chamber_gas_state(self):
        """(volume, gauge, beta) per chamber at the current positions; a constant chamber: (volume, p, 0)"""
        n = self._chamber_counts()[0]
        v, g, b = np.zeros(n), np.zeros(n), np.zeros(n)
        self._chk(self._L.ipcgpu_chamber_gas_state(self.h, _dp(v), _dp(g), _dp(b)))
        return v, g, b

    def chamber_volume_gradient(self, chamber, projectDBC=True):
        """gradV of one chamber at the current positions (3 nV, xyz interleaved)"""
        u = np.zeros(3 * self.nV)
        self._chk(self._L.ipcgpu_chamber_volume_gradient(self.h, C.c_int(int(chamber)), C.c_int(int(projectDBC)), _dp(u)))
        return u

    def chamber_gas_solve(self, coef, rhs):
        """(A + coef sum_c beta_c u_c u_c^T)^-1 rhs on the matrix as last assembled and factorised: the stepper's own routine"""
        rhs = _f64(rhs)
        x = np.zeros_like(rhs)
        self._chk(self._L.ipcgpu_chamber_gas_solve(self.h, C.c_double(coef), _dp(rhs), _dp(x)))
        return x

    def set_obstacle(self, ids, obstacle_only=False):
        ids = _i32(ids)
        self._chk(self._L.ipcgpu_set_obstacle_nodes(self.h, C.c_int(len(ids)), _ip(ids), C.c_int(int(obstacle_only))))

    def set_contact_groups(self, groups, collide, fric_scale=None):
        """Contact groups (ipcgpu_set_contact_groups): `groups[c]` the group of component c of set_components, `collide` a symmetric 0 / 1 matrix over the
        groups (0: the pair of groups forms no contact pair at all), `fric_scale` a symmetric matrix of factors >= 0 on the lagged normal forces (None:
        all 1; effective coefficient = selfFric x scale).  `groups=None` or empty goes back to the default."""
        g = _i32([] if groups is None else groups).ravel()
        if len(g) == 0:
            self._chk(self._L.ipcgpu_set_contact_groups(self.h, C.c_int(0), None, C.c_int(0), None, None))
            return
        col = np.ascontiguousarray(collide, dtype=np.uint8)
        if col.ndim != 2 or col.shape[0] != col.shape[1]:
            raise ValueError("set_contact_groups: collide must be a square matrix")
        fs = None
        if fric_scale is not None:
            fs = _f64(fric_scale)
            if fs.shape != col.shape:
                raise ValueError("set_contact_groups: fric_scale must have the shape of collide")
        self._chk(self._L.ipcgpu_set_contact_groups(self.h, C.c_int(len(g)), _ip(g), C.c_int(col.shape[0]), col.ctypes.data_as(C.POINTER(C.c_ubyte)), _dp(fs)))

    def get_contact_groups(self):
        """(nGroups, words[nV]): per node the word the contact kernels read -- bits 4-7 its group, bits 16-31 the group's row of `collide`."""
        n = C.c_int()
        w = np.zeros(self.nV, dtype=np.int32)
        self._chk(self._L.ipcgpu_get_contact_groups(self.h, C.byref(n), _ip(w)))
        return n.value, w.view(np.uint32)

    def get_surface(self):
        n = np.zeros(3, dtype=np.int32)
        self._chk(self._L.ipcgpu_get_surface(self.h, _ip(n), None, None))
        svi = np.zeros(n[0], dtype=np.int32)
        sfe = np.zeros((n[2], 2), dtype=np.int32)
        self._chk(self._L.ipcgpu_get_surface(self.h, _ip(n), _ip(svi), _ip(sfe)))
        return svi, sfe

    def contact_build(self, dHat):
        n = np.zeros(3, dtype=np.int32)
        self._chk(self._L.ipcgpu_contact_build(self.h, C.c_double(dHat), _ip(n)))
        a = np.zeros((n[0], 4), dtype=np.int32)
        p = np.zeros((n[1], 4), dtype=np.int32)
        q = np.zeros((n[1], 2), dtype=np.int32)
        cs = np.zeros((n[2], 2), dtype=np.int32)
        self._chk(self._L.ipcgpu_contact_get(self.h, _ip(a), _ip(p), _ip(q), _ip(cs)))
        return dict(active=a, para=p, para_eiej=q, cs_ptee=cs)

    def contact_set(self, active, para=None, para_eiej=None):
        a = np.ascontiguousarray(active, dtype=np.int32).reshape(-1, 4)
        p = np.ascontiguousarray(para if para is not None else np.zeros((0, 4)), dtype=np.int32).reshape(-1, 4)
        q = np.ascontiguousarray(para_eiej if para_eiej is not None else np.zeros((0, 2)), dtype=np.int32).reshape(-1, 2)
        self._chk(self._L.ipcgpu_contact_set(self.h, C.c_int(a.shape[0]), _ip(a), C.c_int(p.shape[0]), _ip(p), _ip(q)))

    def contact_energy(self, dHat, kappa):
        E = C.c_double()
        self._chk(self._L.ipcgpu_contact_energy(self.h, C.c_double(dHat), C.c_double(kappa), C.byref(E)))
        return E.value

    def contact_gradient_add(self, dHat, kappa, projectDBC=True, grad=None):
        g = np.zeros(3 * self.nV) if grad is None else _f64(grad).copy()
        self._chk(self._L.ipcgpu_contact_gradient_add(self.h, C.c_double(dHat), C.c_double(kappa), C.c_int(int(projectDBC)), _dp(g)))
        return g

    def contact_held(self):
        """The constraint sets the context holds (of the last contact_build / contact_set or of the stepper's last build), without rebuilding them."""
        n = np.zeros(3, dtype=np.int32)
        self._chk(self._L.ipcgpu_contact_counts(self.h, _ip(n)))
        a, p, q = np.zeros((n[0], 4), dtype=np.int32), np.zeros((n[1], 4), dtype=np.int32), np.zeros((n[1], 2), dtype=np.int32)
        self._chk(self._L.ipcgpu_contact_get(self.h, _ip(a), _ip(p), _ip(q), None))
        return dict(active=a, para=p, para_eiej=q)

    def contact_evaluate(self, tuples):
        """Squared distances of MMCVID tuples at the positions the context holds (ipcgpu_contact_evaluate)."""
        t = np.ascontiguousarray(tuples, dtype=np.int32).reshape(-1, 4)
        val = np.zeros(t.shape[0])
        self._chk(self._L.ipcgpu_contact_evaluate(self.h, C.c_int(t.shape[0]), _ip(t), _dp(val)))
        return val

    def contact_report(self, dHat=None, kappa=None, x_prev=None, eps2=None, coef=None):
        """Contact report of the sets the context holds at the positions it holds (ipcgpu_contact_report; changes no state): a structured array with
        one entry per pair of components `(a, b)`, a <= b, or component and half-space `(a, -1 - h)`, that has a contributing tuple -- fields `a`, `b`,
        `nPP`, `nPE`, `nPT`, `nEE`, `nMollified`, `argmin`, `minD2`, `FA`, `FB`, `TA`, `TB` (barrier force and torque on either side), `RA`, `RB`, `W`
        (lagged friction forces and their work over the step from `x_prev`).  Missing dHat / kappa come from state().  The friction fields need `x_prev`
        AND `coef`, the friction coefficient the lagged terms are scaled with (the scene's selfFric: the library keeps no copy the caller could ask for);
        a missing eps2 comes from friction_state().  Without them the friction fields are zero."""
        if dHat is None or kappa is None:
            st = self.state()
            dHat = st["dHat"] if dHat is None else dHat
            kappa = st["kappa"] if kappa is None else kappa
        Vt = None
        if x_prev is not None:
            coef = 0.0 if coef is None else coef
            if coef > 0 and eps2 is None:
                eps2 = self.friction_state()["fricDHat"]
            if coef > 0 and eps2 > 0:
                Vt = np.asfortranarray(x_prev, dtype=np.float64)
                assert Vt.shape == (self.nV, 3)
        call = lambda cap, ri, rd, n: self._L.ipcgpu_contact_report(self.h, C.c_double(dHat), C.c_double(kappa), _dp(Vt), C.c_double(eps2 or 0.0),
                                                                    C.c_double(coef or 0.0), C.c_int(cap), C.byref(n), _ip(ri), _dp(rd))
        n = C.c_int(0)
        rc = call(0, None, None, n)
        if rc != IPCGPU_OK and n.value == 0:
            self._chk(rc)
        rows_i, rows_d = np.zeros((n.value, 8), dtype=np.int32), np.zeros((n.value, 20))
        if n.value:
            self._chk(call(n.value, rows_i, rows_d, n))
        out = np.zeros(n.value, dtype=CONTACT_REPORT_DTYPE)
        for k, name in enumerate(("a", "b", "nPP", "nPE", "nPT", "nEE", "nMollified", "argmin")):
            out[name] = rows_i[:, k]
        out["minD2"] = rows_d[:, 0]
        for k, name in enumerate(("FA", "FB", "TA", "TB", "RA", "RB")):
            out[name] = rows_d[:, 1 + 3 * k:4 + 3 * k]
        out["W"] = rows_d[:, 19]
        return out

    def contact_hessian_add(self, dHat, kappa, projectDBC=True):
        self._chk(self._L.ipcgpu_contact_hessian_add(self.h, C.c_double(dHat), C.c_double(kappa), C.c_int(int(projectDBC))))

    def contact_connectivity(self):
        n = C.c_int()
        self._chk(self._L.ipcgpu_contact_connectivity(self.h, C.c_int(0), None, C.byref(n)))
        buf = np.zeros((max(n.value, 1), 2), dtype=np.int32)
        self._chk(self._L.ipcgpu_contact_connectivity(self.h, C.c_int(n.value), _ip(buf), C.byref(n)))
        return buf[:n.value].copy()

    def ccd_partial(self, p, slackness=0.8, step=1.0):
        p = _f64(p)
        s = C.c_double(step)
        pair = np.zeros(2, dtype=np.int32)
        self._chk(self._L.ipcgpu_ccd_partial(self.h, _dp(p), C.c_double(slackness), C.byref(s), _ip(pair)))
        return s.value, (int(pair[0]), int(pair[1]))

    def ccd_full(self, p, slackness=0.8, step=1.0):
        p = _f64(p)
        s = C.c_double(step)
        pair = np.zeros(2, dtype=np.int32)
        n = C.c_int()
        self._chk(self._L.ipcgpu_ccd_full(self.h, _dp(p), C.c_double(slackness), C.byref(s), _ip(pair), C.byref(n)))
        return s.value, (int(pair[0]), int(pair[1])), n.value

    def ccd_full_reference(self, p, slackness=0.8, step=1.0):
        """The reference's full sweep: returns the bound, the step after the hash's cap, the limiting pair (kind, i, j), #pairs queried."""
        p = _f64(p)
        s, cap = C.c_double(step), C.c_double()
        arg = np.zeros(3, dtype=np.int32)
        n = C.c_int()
        self._chk(self._L.ipcgpu_ccd_full_reference(self.h, _dp(p), C.c_double(slackness), C.byref(s), C.byref(cap), _ip(arg), C.byref(n)))
        return s.value, cap.value, tuple(int(x) for x in arg), n.value

    def set_ccd_mode(self, mode):
        self._chk(self._L.ipcgpu_set_ccd_mode(self.h, C.c_int(mode)))

    def is_intersected(self):
        f = C.c_int()
        self._chk(self._L.ipcgpu_is_intersected(self.h, C.byref(f)))
        return bool(f.value)

    # ---- Optimizer building blocks
    def assemble_newton(self, dtSq, projectDBC=True, with_gradient=True):
        g = np.zeros(3 * self.nV) if with_gradient else None
        self._chk(self._L.ipcgpu_assemble_newton(self.h, C.c_double(dtSq), C.c_int(int(projectDBC)), _dp(g)))
        return g

    def incremental_potential(self, dtSq):
        E = C.c_double()
        self._chk(self._L.ipcgpu_incremental_potential(self.h, C.c_double(dtSq), C.byref(E)))
        return E.value

    def gradient(self, dtSq, projectDBC=True):
        g = np.zeros(3 * self.nV)
        self._chk(self._L.ipcgpu_gradient(self.h, C.c_double(dtSq), C.c_int(int(projectDBC)), _dp(g)))
        return g

    # ---- Optimizer
    def opt_init(self, dt=0.04, gravity=False):
        self._chk(self._L.ipcgpu_opt_init(self.h, C.c_double(dt), C.c_int(int(gravity))))

    def set_rel_tol(self, tol):
        self._chk(self._L.ipcgpu_opt_set_rel_tol(self.h, C.c_double(tol)))

    def set_twist(self, left, right, ang_vel=0.4 * np.pi):
        left, right = _i32(left), _i32(right)
        self._chk(self._L.ipcgpu_opt_set_twist(self.h, C.c_int(len(left)), _ip(left), C.c_int(len(right)),
                                               _ip(right), C.c_double(ang_vel)))

    def precompute(self):
        self._chk(self._L.ipcgpu_opt_precompute(self.h))

    def begin_timestep(self):
        self._chk(self._L.ipcgpu_opt_begin_timestep(self.h))

    def newton_iter(self):
        cv = C.c_int()
        self._chk(self._L.ipcgpu_opt_newton_iter(self.h, C.byref(cv)))
        return bool(cv.value)

    def end_timestep(self):
        self._chk(self._L.ipcgpu_opt_end_timestep(self.h))

    def solve_timestep(self, max_iter=100):
        n = C.c_int()
        self._chk(self._L.ipcgpu_opt_solve_timestep(self.h, C.c_int(max_iter), C.byref(n)))
        return n.value

    def state(self):
        V = np.zeros((self.nV, 3), order="F")
        p = np.zeros(3 * self.nV)
        g = np.zeros(3 * self.nV)
        sc = np.zeros(8)
        self._chk(self._L.ipcgpu_opt_get_state(self.h, _dp(V), _dp(p), _dp(g), _dp(sc)))
        return dict(V=V, searchDir=p, gradient=g, E=sc[0], stepSize=sc[1], targetGRes=sc[2],
                    innerIterAmt=int(sc[3]), timestep=int(sc[4]), alphaFeasible=sc[5], kappa=sc[6], dHat=sc[7])

    def enable_self_collision(self, dHatEps=1e-3):
        self._chk(self._L.ipcgpu_opt_enable_self_collision(self.h, C.c_double(dHatEps)))

    def set_pattern_lookahead(self, pad=4.0):
        self._chk(self._L.ipcgpu_opt_set_pattern_lookahead(self.h, C.c_double(pad)))

    def add_half_space(self, origin, normal, dHatEps=1e-3):
        o, n = _f64(np.asarray(origin)), _f64(np.asarray(normal))
        idx = C.c_int()
        self._chk(self._L.ipcgpu_opt_add_half_space(self.h, _dp(o), _dp(n), C.c_double(dHatEps), C.byref(idx)))
        return idx.value

    def halfspace_build(self, idx, dHat):
        verts = np.zeros(self.nV, dtype=np.int32)
        n = C.c_int()
        self._chk(self._L.ipcgpu_halfspace_build(self.h, C.c_int(idx), C.c_double(dHat), C.c_int(self.nV), _ip(verts), C.byref(n)))
        return verts[:n.value].copy()

    def halfspace_set(self, idx, verts):
        verts = _i32(verts)
        self._chk(self._L.ipcgpu_halfspace_set(self.h, C.c_int(idx), C.c_int(len(verts)), _ip(verts)))

    def halfspace_energy(self, idx, dHat, kappa):
        E = C.c_double()
        self._chk(self._L.ipcgpu_halfspace_energy(self.h, C.c_int(idx), C.c_double(dHat), C.c_double(kappa), C.byref(E)))
        return E.value

    def halfspace_gradient_add(self, idx, dHat, kappa, grad=None):
        g = np.zeros(3 * self.nV) if grad is None else _f64(grad).copy()
        self._chk(self._L.ipcgpu_halfspace_gradient_add(self.h, C.c_int(idx), C.c_double(dHat), C.c_double(kappa), _dp(g)))
        return g

    def halfspace_hessian_add(self, idx, dHat, kappa, projectDBC=True):
        self._chk(self._L.ipcgpu_halfspace_hessian_add(self.h, C.c_int(idx), C.c_double(dHat), C.c_double(kappa),
                                                       C.c_int(int(projectDBC))))

    def half_space_move(self, idx, delta, slackness=0.5):
        """HalfSpace::move: displace plane `idx` by (the feasible fraction of) delta; returns the fraction left"""
        d = _f64(np.asarray(delta, dtype=np.float64))
        left = C.c_double()
        self._chk(self._L.ipcgpu_halfspace_move(self.h, C.c_int(idx), _dp(d), C.c_double(slackness), C.byref(left)))
        return left.value

    def halfspace_step_bound(self, idx, p, slackness=0.9, step=1.0):
        p = _f64(np.asarray(p).reshape(-1))
        s = C.c_double(step)
        self._chk(self._L.ipcgpu_halfspace_step_bound(self.h, C.c_int(idx), _dp(p), C.c_double(slackness), C.byref(s)))
        return s.value

    # ---- round colliders (spheres, capsules; ipc_amd/csrc/round_collider_kernels.h) ----
    def add_round_collider(self, p0, p1, R, hollow=False, dHatEps=1e-3):
        """segment [p0, p1] with radius R: a sphere where p0 == p1, a capsule otherwise; hollow: the bodies live inside (spheres only)"""
        a, b = _f64(np.asarray(p0, dtype=np.float64).reshape(3)), _f64(np.asarray(p1, dtype=np.float64).reshape(3))
        idx = C.c_int()
        self._chk(self._L.ipcgpu_opt_add_round_collider(self.h, _dp(a), _dp(b), C.c_double(R), C.c_int(int(hollow)), C.c_double(dHatEps), C.byref(idx)))
        return idx.value

    def add_sphere_collider(self, centre, R, hollow=False, dHatEps=1e-3):
        return self.add_round_collider(centre, centre, R, hollow, dHatEps)

    def round_build(self, idx, dHat):
        verts = np.zeros(self.nV, dtype=np.int32)
        n = C.c_int()
        self._chk(self._L.ipcgpu_round_build(self.h, C.c_int(idx), C.c_double(dHat), C.c_int(self.nV), _ip(verts), C.byref(n)))
        return verts[:n.value].copy()

    def round_set(self, idx, verts):
        verts = _i32(verts)
        self._chk(self._L.ipcgpu_round_set(self.h, C.c_int(idx), C.c_int(len(verts)), _ip(verts)))

    def round_energy(self, idx, dHat, kappa):
        E = C.c_double()
        self._chk(self._L.ipcgpu_round_energy(self.h, C.c_int(idx), C.c_double(dHat), C.c_double(kappa), C.byref(E)))
        return E.value

    def round_gradient_add(self, idx, dHat, kappa, grad=None):
        g = np.zeros(3 * self.nV) if grad is None else _f64(grad).copy()
        self._chk(self._L.ipcgpu_round_gradient_add(self.h, C.c_int(idx), C.c_double(dHat), C.c_double(kappa), _dp(g)))
        return g

    def round_hessian_add(self, idx, dHat, kappa, projectDBC=True):
        self._chk(self._L.ipcgpu_round_hessian_add(self.h, C.c_int(idx), C.c_double(dHat), C.c_double(kappa), C.c_int(int(projectDBC))))

    def round_step_bound(self, idx, p, slackness=0.9, step=1.0):
        p = _f64(np.asarray(p).reshape(-1))
        s = C.c_double(step)
        self._chk(self._L.ipcgpu_round_step_bound(self.h, C.c_int(idx), _dp(p), C.c_double(slackness), C.byref(s)))
        return s.value

    def round_move(self, idx, delta, slackness=0.5):
        """translate round collider `idx` by (the feasible fraction of) delta; returns the fraction left"""
        d = _f64(np.asarray(delta, dtype=np.float64).reshape(3))
        left = C.c_double()
        self._chk(self._L.ipcgpu_round_move(self.h, C.c_int(idx), _dp(d), C.c_double(slackness), C.byref(left)))
        return left.value

    def round_get(self, idx):
        p0, p1, R, hollow = np.zeros(3), np.zeros(3), C.c_double(), C.c_int()
        self._chk(self._L.ipcgpu_round_get(self.h, C.c_int(idx), _dp(p0), _dp(p1), C.byref(R), C.byref(hollow)))
        return dict(p0=p0, p1=p1, R=R.value, hollow=bool(hollow.value))

    def set_round_collider_friction(self, idx, mu):
        self._chk(self._L.ipcgpu_opt_set_round_collider_friction(self.h, C.c_int(idx), C.c_double(mu)))

    def round_lag_update(self, idx, dHat, kappa):
        n = C.c_int()
        self._chk(self._L.ipcgpu_round_lag_update(self.h, C.c_int(idx), C.c_double(dHat), C.c_double(kappa), C.byref(n)))
        return n.value

    def round_friction_energy(self, idx, Vt, eps2):
        Vt = _f64(np.asarray(Vt).reshape(-1))
        E = C.c_double()
        self._chk(self._L.ipcgpu_round_friction_energy(self.h, C.c_int(idx), _dp(Vt), C.c_double(eps2), C.byref(E)))
        return E.value

    def round_friction_gradient_add(self, idx, Vt, eps2, grad=None):
        Vt = _f64(np.asarray(Vt).reshape(-1))
        g = np.zeros(3 * self.nV) if grad is None else _f64(grad).copy()
        self._chk(self._L.ipcgpu_round_friction_gradient_add(self.h, C.c_int(idx), _dp(Vt), C.c_double(eps2), _dp(g)))
        return g

    def round_friction_hessian_add(self, idx, Vt, eps2, projectDBC=True):
        Vt = _f64(np.asarray(Vt).reshape(-1))
        self._chk(self._L.ipcgpu_round_friction_hessian_add(self.h, C.c_int(idx), _dp(Vt), C.c_double(eps2), C.c_int(int(projectDBC))))

    def round_state(self, idx, dHat=0.0, kappa=0.0):
        """set size, smallest signed distance over the surface nodes, total barrier force on the bodies, its torque about p0, total lagged friction force"""
        n, out = C.c_int(), np.zeros(10)
        self._chk(self._L.ipcgpu_round_state(self.h, C.c_int(idx), C.c_double(dHat), C.c_double(kappa), C.byref(n), _dp(out)))
        return dict(n=n.value, min_s=float(out[0]), force=out[1:4].copy(), torque=out[4:7].copy(), friction=out[7:10].copy())

    def set_friction_target(self, eps_v_target):
        """eps_v homotopy target (`tuning`'s sixth entry); <= 0: the same as eps_v"""
        self._chk(self._L.ipcgpu_opt_set_friction_target(self.h, C.c_double(eps_v_target)))

    def set_constructor_dt(self, h):
        """the step size inside eps_v^2 h^2 and CN_MBC (0.025 in the reference whatever the scene's dt: Optimizer.cpp:116, 268, 290-303)"""
        self._chk(self._L.ipcgpu_opt_set_constructor_dt(self.h, C.c_double(h)))

    def set_parameter_scaling(self, use_abs_parameters=False, dtol_rel=1e-9, kappa_min_multiplier=1e11):
        """`useAbsParameters`, tuning[3] and `kappaMinMultiplier` of the scene file (Config.cpp:553-558)"""
        self._chk(self._L.ipcgpu_opt_set_parameter_scaling(self.h, C.c_int(int(use_abs_parameters)), C.c_double(dtol_rel),
                                                           C.c_double(kappa_min_multiplier)))

    def set_friction(self, self_fric=0.0, fric_iter_amt=1, eps_v=1e-3):
        self._chk(self._L.ipcgpu_opt_set_friction(self.h, C.c_double(self_fric), C.c_int(fric_iter_amt), C.c_double(eps_v)))

    def set_kappa(self, kappa):
        self._chk(self._L.ipcgpu_opt_set_kappa(self.h, C.c_double(kappa)))

    def set_dhat_target(self, eps):
        self._chk(self._L.ipcgpu_opt_set_dhat_target(self.h, C.c_double(eps)))

    def set_damping(self, damping_stiff):
        self._chk(self._L.ipcgpu_opt_set_damping(self.h, C.c_double(damping_stiff)))

    def set_friction_scales(self, scale_self=1.0, scale_obstacle=1.0):
        self._chk(self._L.ipcgpu_opt_set_friction_scales(self.h, C.c_double(scale_self), C.c_double(scale_obstacle)))

    def force_friction_loop(self, on=True):
        self._chk(self._L.ipcgpu_opt_force_friction_loop(self.h, C.c_int(int(on))))

    def set_half_space_friction(self, idx, mu):
        self._chk(self._L.ipcgpu_opt_set_half_space_friction(self.h, C.c_int(idx), C.c_double(mu)))

    def next_subproblem(self):
        more = C.c_int()
        self._chk(self._L.ipcgpu_opt_next_subproblem(self.h, C.byref(more)))
        return bool(more.value)

    def friction_state(self):
        sc = np.zeros(4)
        self._chk(self._L.ipcgpu_opt_get_friction_state(self.h, _dp(sc), None))
        lam = np.zeros(int(sc[1]))
        if lam.size:
            self._chk(self._L.ipcgpu_opt_get_friction_state(self.h, _dp(sc), _dp(lam)))
        return dict(fricDHat=sc[0], n_lagged=int(sc[1]), fric_iter=int(sc[2]), n_half_space_lagged=int(sc[3]), lam=lam)

    def friction_update(self, dHat, kappa):
        n = C.c_int()
        self._chk(self._L.ipcgpu_friction_update(self.h, C.c_double(dHat), C.c_double(kappa), C.byref(n)))
        lam, co, ba = np.zeros(n.value), np.zeros((n.value, 2)), np.zeros((n.value, 6))
        if n.value:
            self._chk(self._L.ipcgpu_friction_get(self.h, _dp(lam), _dp(co), _dp(ba)))
        return dict(lam=lam, coord=co, basis=ba)

    def friction_energy(self, Vt, eps2, coef):
        Vt = np.asfortranarray(Vt, dtype=np.float64)
        E = C.c_double()
        self._chk(self._L.ipcgpu_friction_energy(self.h, _dp(Vt), C.c_double(eps2), C.c_double(coef), C.byref(E)))
        return E.value

    def friction_gradient_add(self, Vt, eps2, coef, grad=None):
        Vt = np.asfortranarray(Vt, dtype=np.float64)
        g = np.zeros(3 * self.nV) if grad is None else _f64(grad).copy()
        self._chk(self._L.ipcgpu_friction_gradient_add(self.h, _dp(Vt), C.c_double(eps2), C.c_double(coef), _dp(g)))
        return g

    def friction_hessian_add(self, Vt, eps2, coef, projectDBC=True):
        Vt = np.asfortranarray(Vt, dtype=np.float64)
        self._chk(self._L.ipcgpu_friction_hessian_add(self.h, _dp(Vt), C.c_double(eps2), C.c_double(coef), C.c_int(int(projectDBC))))

    def set_time_integration(self, name, beta=0.25, gamma=0.5):
        """Scene-script `timeIntegration BE | NM beta gamma`."""
        self._chk(self._L.ipcgpu_opt_set_time_integration(self.h, C.c_int({"BE": 0, "NM": 1}[name]), C.c_double(beta), C.c_double(gamma)))

    def set_warm_start(self, option):
        self._chk(self._L.ipcgpu_opt_set_warm_start(self.h, C.c_int(int(option))))

    def warm_step(self):
        v = C.c_double()
        self._chk(self._L.ipcgpu_opt_get_warm_step(self.h, C.byref(v)))
        return v.value

    def add_dirichlet(self, ids, lin_vel=(0, 0, 0), ang_vel_deg=(0, 0, 0), t0=0.0, t1=float("inf")):
        """One `DBC bboxMin bboxMax linVel angVel [t0 t1]` entry of a shape line (degrees per second, as in the script)."""
        ids = _i32(ids)
        lin = _f64(np.asarray(lin_vel, dtype=np.float64))
        ang = _f64(np.asarray(ang_vel_deg, dtype=np.float64) * np.pi / 180)
        self._chk(self._L.ipcgpu_opt_add_dirichlet(self.h, C.c_int(len(ids)), _ip(ids), _dp(lin), _dp(ang), C.c_double(t0), C.c_double(t1)))

    def set_dirichlet_targets(self, group, targets):
        """mesh-sequence motion: the positions the group's nodes are to reach in the next time step (None ends the sequence)"""
        if targets is None:
            self._chk(self._L.ipcgpu_opt_set_dirichlet_targets(self.h, C.c_int(group), C.c_int(0), None))
            return
        t = _f64(np.ascontiguousarray(np.asarray(targets, dtype=np.float64).reshape(-1, 3)))
        self._chk(self._L.ipcgpu_opt_set_dirichlet_targets(self.h, C.c_int(group), C.c_int(t.shape[0]), _dp(t)))

    def set_dirichlet_motion(self, group, lin_vel=(0, 0, 0), ang_vel_deg=(0, 0, 0), center=None, force_nonzero=True):
        """Motion of Dirichlet group `group` for the coming time steps (the rule-driven scripts of AnimScripter.cpp:1961-2135)."""
        lin = _f64(np.asarray(lin_vel, dtype=np.float64))
        ang = _f64(np.asarray(ang_vel_deg, dtype=np.float64) * np.pi / 180)
        ctr = None if center is None else _f64(np.asarray(center, dtype=np.float64))
        self._chk(self._L.ipcgpu_opt_set_dirichlet_motion(self.h, C.c_int(group), _dp(lin), _dp(ang), None if ctr is None else _dp(ctr),
                                                          C.c_int(int(force_nonzero))))

    def end_dirichlet(self, group, t_end):
        """Free the vertices of Dirichlet group `group` from the time step starting at t_end on (scripts that let go of a handle)."""
        self._chk(self._L.ipcgpu_opt_end_dirichlet(self.h, C.c_int(group), C.c_double(t_end)))

    def add_neumann(self, ids, accel, t0=0.0, t1=float("inf")):
        """One `NBC bboxMin bboxMax force [t0 t1]` entry of a shape line."""
        ids = _i32(ids)
        a = _f64(np.asarray(accel, dtype=np.float64))
        self._chk(self._L.ipcgpu_opt_add_neumann(self.h, C.c_int(len(ids)), _ip(ids), _dp(a), C.c_double(t0), C.c_double(t1)))

    def dbc_state(self):
        out = np.zeros(4)
        self._chk(self._L.ipcgpu_opt_get_dbc_state(self.h, _dp(out)))
        return dict(completed=out[0], rho=out[1], projectDBC=bool(out[2]), n_targets=int(out[3]))

    def kinematics(self):
        vel, acc, dx = np.zeros(3 * self.nV), np.zeros(3 * self.nV), np.zeros(3 * self.nV)
        self._chk(self._L.ipcgpu_opt_get_kinematics(self.h, _dp(vel), _dp(acc), _dp(dx)))
        return dict(velocity=vel, acceleration=acc, dx_Elastic=dx)

    def save_status(self, path):
        self._chk(self._L.ipcgpu_opt_save_status(self.h, str(path).encode()))

    def load_status(self, path):
        self._chk(self._L.ipcgpu_opt_load_status(self.h, str(path).encode()))

    def set_velocity(self, vel):
        vel = _f64(np.asarray(vel).reshape(-1))
        assert vel.size == 3 * self.nV
        self._chk(self._L.ipcgpu_opt_set_velocity(self.h, _dp(vel)))

    def contact_state(self):
        cnt = np.zeros(6, dtype=np.int32)
        pr = np.zeros(2, dtype=np.int32)
        self._chk(self._L.ipcgpu_opt_get_contact_state(self.h, _ip(cnt), _ip(pr)))
        return dict(nActive=int(cnt[0]), nPara=int(cnt[1]), nCand=int(cnt[2]), nHalfSpace=int(cnt[3]), nFullCCD=int(cnt[4]),
                    nPatternChanges=int(cnt[5]), ccdPair=(int(pr[0]), int(pr[1])))

    def timers(self):
        t = np.zeros(16)
        self._chk(self._L.ipcgpu_opt_get_timers(self.h, _dp(t)))
        return t

    # ---- measurement
    def bench_assembly(self, dtSq, reps=20):
        ms, by = C.c_double(), C.c_double()
        self._chk(self._L.ipcgpu_bench_assembly(self.h, C.c_double(dtSq), C.c_int(reps), C.byref(ms), C.byref(by)))
        return ms.value, by.value

    def bench_factor_solve(self, reps=3):
        f, s = C.c_double(), C.c_double()
        self._chk(self._L.ipcgpu_bench_factor_solve(self.h, C.c_int(reps), C.byref(f), C.byref(s)))
        return f.value, s.value

    def bench_multiply_sym(self, reps=50):
        ms, by = C.c_double(), C.c_double()
        self._chk(self._L.ipcgpu_bench_multiply_sym(self.h, C.c_int(reps), C.byref(ms), C.byref(by)))
        return ms.value, by.value

    def bench_stream(self, nbytes=1 << 30, reps=10):
        g = C.c_double()
        self._chk(self._L.ipcgpu_bench_stream(self.h, C.c_longlong(nbytes), C.c_int(reps), C.byref(g)))
        return g.value
