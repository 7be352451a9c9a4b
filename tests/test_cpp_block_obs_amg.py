"""The header-only C++20 facade of FDAPDE_SOLVER_BLOCK_AMG with the factored data term carried: tests/cpp/block_obs_amg_facade_test.cpp, compiled here with
the g++ flags of tests/cpp/Makefile (as tests/test_cpp_block_obs.py compiles its driver).
  * CPU: it compiles -- PDE::BlockSolver::carry_observations and the explicit instantiation of SMW<PDE::BlockSolver> -- and, without a device, loads the
    fixture and refuses to go on;
  * GPU: on quasi_circle with the golden incidence matrix, compute(A, Psi) -> carry_observations() -> solve with method FDAPDE_SOLVER_BLOCK_AMG agrees with
    the densified system's PartialPivLU to 1e-8, an SMW solve with a rank-3 update on top does too, and without carry_observations() the solve throws with
    "term" in the message."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "block_obs_amg_facade_test.cpp")
EXE = os.path.join(ROOT, "build", "block_obs_amg_facade_test")
MESHES = os.path.join(ROOT, "tests", "golden", "mesh")


def _build():
    from fdapde_loader import load_package

    load_package()   # (the C ABI library the driver links against)
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    lib = os.path.join(ROOT, "fdapde-core_amd", "lib")
    subprocess.check_call(["g++", "-std=c++20", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), SRC, "-L" + lib, "-lfdapde_hip",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined", "-o", EXE])


def test_block_obs_amg_facade_compiles_and_refuses_to_run_without_a_device():
    _build()
    assert os.path.exists(EXE)
    import ctypes

    lib = ctypes.CDLL(os.path.join(ROOT, "fdapde-core_amd", "lib", "libfdapde_hip.so"))
    if lib.fdapde_device_count() == 0:
        r = subprocess.run([EXE, MESHES], capture_output=True, text=True, timeout=120)
        assert r.returncode == 3 and "no CPU fallback" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_areal_block_system_with_the_term_carried_through_the_cpp_facade():
    _build()
    r = subprocess.run([EXE, MESHES], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout
