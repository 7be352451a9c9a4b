"""The header-only C++20 facade on 1-D meshes (Triangulation<1,1>, Triangulation<1,2>): tests/cpp/network_facade_test.cpp, compiled here with the g++ flags of
tests/cpp/Makefile (invoked directly; the Makefile builds the planar driver only).
  * CPU: it compiles -- Triangulation<1,1>(a, b, n) and (nodes), MeshLoader<1,2>, PDE<Triangulation<1,N>, ..., FEM_HIP, fem_order<R>> with
    ScalarField<N> forcing, SMatrix<2> diffusion, SVector<2> advection, Integrator<FEM_HIP, 1, R> -- and, without a device, loads the network
    fixture, builds the interval and refuses to go on;
  * GPU: problems with zero Dirichlet data on the reference's network and on Triangulation<1,1>(0, 1, 64) at P1 and P2 through the facade match
    the C ABI path to 1e-12 (stiffness bit for bit), and the network's total length through Integrator matches the sum of the segment lengths."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "network_facade_test.cpp")
EXE = os.path.join(ROOT, "build", "network_facade_test")
MESHES = os.path.join(ROOT, "tests", "golden", "mesh")


def _build():
    from fdapde_loader import load_package

    load_package()   # (the C ABI library the driver links against)
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    lib = os.path.join(ROOT, "fdapde-core_amd", "lib")
    subprocess.check_call(["g++", "-std=c++20", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), SRC, "-L" + lib, "-lfdapde_hip",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined", "-o", EXE])


def test_network_facade_compiles_and_refuses_to_run_without_a_device():
    _build()
    assert os.path.exists(EXE)
    import ctypes

    lib = ctypes.CDLL(os.path.join(ROOT, "fdapde-core_amd", "lib", "libfdapde_hip.so"))
    if lib.fdapde_device_count() == 0:
        r = subprocess.run([EXE, MESHES], capture_output=True, text=True, timeout=120)
        assert r.returncode == 3 and "no CPU fallback" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_network_problems_through_the_cpp_facade():
    _build()
    r = subprocess.run([EXE, MESHES], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout
