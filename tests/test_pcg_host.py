"""Host side of the iterative solver (solver type 2): the scene keyword, the header, the numpy CG the GPU tests count against, the adapter."""
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

import pcg_numpy
from ipc_amd import scene_script as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = "energy NH\ntime 1 0.01\n%s\n"


@pytest.mark.parametrize("line,solver", [("linearSolver AMGCL", 2), ("linearSolver amgcl", 2), ("linSysSolver AMGCL", 2), ("linearSolver CHOLMOD", 0),
                                         ("linearSolver cholmod", 0), ("linearSolver Eigen", 0), ("linearSolver EIGEN", 0), ("", 0)])
def test_scene_keyword(line, solver):
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # a known name does not warn
        cfg = ss.SceneConfig.parse(SCENE % line)
    assert cfg.linear_solver == solver


def test_unknown_solver_name_falls_back_to_the_exact_solver():
    with pytest.warns(UserWarning, match="unknown linear system solver"):  # Config.cpp:704-705
        cfg = ss.SceneConfig.parse(SCENE % "linearSolver pardiso")
    assert cfg.linear_solver == 0


def test_header_declares_the_iterative_solver():
    txt = open(os.path.join(ROOT, "include", "ipcgpu.h")).read()
    for name, val in (("IPCGPU_SOLVER_PCG", 2), ("IPCGPU_PRECOND_BLOCK_JACOBI", 0), ("IPCGPU_PRECOND_LAGGED_CHOLESKY", 1)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, val), txt), name
    from ipc_amd import lib
    decl = lib.declared_symbols()
    for fn in ("ipcgpu_linsys_set_iterative", "ipcgpu_linsys_iter_stats", "ipcgpu_linsys_multiply_sym"):
        assert fn in decl
    assert (lib.SOLVER_PCG, lib.PRECOND_BLOCK_JACOBI, lib.PRECOND_LAGGED_CHOLESKY) == (2, 0, 1)


def random_spd_upper_csr(nodes, seed):
    rng = np.random.default_rng(seed)
    n = 3 * nodes
    B = rng.normal(size=(n, n)) * (rng.random((n, n)) < 0.3)
    A = B @ B.T + np.diag(rng.uniform(0.5, 50.0, size=n))
    ia, ja, a = [0], [], []
    for r in range(n):
        for c in range(r, n):
            if c == r or A[r, c] != 0.0:
                ja.append(c)
                a.append(A[r, c])
        ia.append(len(ja))
    return A, np.array(ia, dtype=np.int32), np.array(ja, dtype=np.int32), np.array(a)


@pytest.mark.parametrize("block_jacobi", [False, True])
def test_numpy_cg_solves_a_small_spd_system(block_jacobi):
    A, ia, ja, a = random_spd_upper_csr(8, 5)
    b = np.random.default_rng(6).normal(size=A.shape[0])
    assert np.allclose(pcg_numpy.symv(ia, ja, a, b), A @ b, rtol=1e-13, atol=1e-13)
    x, n = pcg_numpy.cg(ia, ja, a, b, 1e-12, 10 * A.shape[0], block_jacobi=block_jacobi)
    assert n < 10 * A.shape[0]
    assert np.linalg.norm(A @ x - b) <= 1e-11 * np.linalg.norm(b)
    assert np.allclose(x, np.linalg.solve(A, b), rtol=1e-9, atol=1e-12)
    if block_jacobi:
        Dinv = pcg_numpy.block_jacobi_inverse(ia, ja, a)
        for v in range(8):
            assert np.allclose(Dinv[v] @ A[3 * v:3 * v + 3, 3 * v:3 * v + 3], np.eye(3), atol=1e-12)


def _compile_iterative_adapter(exe, flags, links):
    import test_adapters as ta
    from ipc_amd import build as b
    b.build()
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    src = os.path.join(ROOT, "tests", "adapters", "test_adapter_iterative.cpp")
    cmd = ["g++", "-std=c++17", "-O1"] + flags + ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "include", "adapters"), src, "-o", exe,
           "-L" + os.path.join(ROOT, "ipc_amd"), "-lipcgpu"] + links + ["-Wl,-rpath," + os.path.join(ROOT, "ipc_amd"), "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "compiled and linked (1)" in r.stdout, r.stdout + r.stderr
    return ta


def test_adapter_with_the_iterative_selection_compiles_against_the_stand_ins():
    import test_adapters as ta
    _compile_iterative_adapter(os.path.join(ta.BUILD, "test_adapter_iterative"), ["-Wall", "-Werror", "-I" + os.path.join(ROOT, "tests", "mock_ipc")], [])
    txt = open(os.path.join(ROOT, "include", "adapters", "HipLinSysSolver.hpp")).read()
    assert "LinSysSolverType::AMGCL" in txt and "ipcgpu_linsys_set_iterative" in txt and "IPCGPU_SOLVER_PCG" in txt


def test_adapter_with_the_iterative_selection_compiles_against_the_reference_headers():
    import test_adapters as ta
    if not (os.path.isdir(ta.REF_SRC) and os.path.exists(ta.LIB_REF)):
        pytest.skip("the reference's headers exist in the build container only")
    _compile_iterative_adapter(os.path.join(ta.REF_BUILD, "test_adapter_iterative_ref"),
                               ["-w", "-DDIM=3", "-DNDEBUG", "-DIPCGPU_LINSYSSOLVER_TYPE=LinSysSolverType::CHOLMOD"] + ta._ref_includes(),
                               ["-L" + os.path.dirname(ta.LIB_REF), "-lipcref", "-Wl,-rpath," + os.path.dirname(ta.LIB_REF), "-Wl,-rpath," + os.path.join(ROOT, "oracle", "_build")])
