"""The header-only C++20 facade of the Kronecker-sum handle's factored data term: tests/cpp/kron_obs_facade_test.cpp, compiled here with the g++ flags of
tests/cpp/Makefile (as tests/test_cpp_block_obs.py compiles its driver).
  * CPU: it compiles -- PDE::KroneckerSolver::compute(A, Phi, Psi, weights, scale), set_observations and the explicit instantiation of
    SMW<PDE::KroneckerSolver> -- and, without a device, loads the fixture and refuses to go on;
  * GPU: on quasi_circle with the golden incidence matrix, two time nodes and three observation instants with missing observations,
    eval_basis(1, incidence) -> compute(A, Phi, Psi, weights) -> solve equals the C ABI route bit for bit and agrees with the densified system's PartialPivLU to
    1e-8, set_observations replaces the term (checked through the dense inverse of the merged matrix), and an SMW solve with a rank-2 update on top agrees
    with LU to 1e-8."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "kron_obs_facade_test.cpp")
EXE = os.path.join(ROOT, "build", "kron_obs_facade_test")
MESHES = os.path.join(ROOT, "tests", "golden", "mesh")


def _build():
    from fdapde_loader import load_package

    load_package()   # (the C ABI library the driver links against)
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    lib = os.path.join(ROOT, "fdapde-core_amd", "lib")
    subprocess.check_call(["g++", "-std=c++20", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), SRC, "-L" + lib, "-lfdapde_hip",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined", "-o", EXE])


def test_kron_obs_facade_compiles_and_refuses_to_run_without_a_device():
    _build()
    assert os.path.exists(EXE)
    import ctypes

    lib = ctypes.CDLL(os.path.join(ROOT, "fdapde-core_amd", "lib", "libfdapde_hip.so"))
    if lib.fdapde_device_count() == 0:
        r = subprocess.run([EXE, MESHES], capture_output=True, text=True, timeout=120)
        assert r.returncode == 3 and "no CPU fallback" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_spacetime_areal_system_through_the_cpp_facade():
    _build()
    r = subprocess.run([EXE, MESHES], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout
