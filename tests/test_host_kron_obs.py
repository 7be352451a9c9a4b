"""The host set-up of the Kronecker-sum handle's factored data term (csrc/host_kron_obs.cpp with host_obs.cpp: plain loops, no device) on the CPU:
tests/cpp/host_kron_obs_test.cpp, compiled here as tests/test_host_obs.py compiles its driver.  The program checks that the validation refuses each malformed
input fdapde_kron_set_obs names (p out of range, Phi == NULL with p > q, a non-finite entry of Phi, weight or scale, and what obs_validate refuses of Psi),
the weights' transposition into the per-observation order, Phi = NULL as [I_p 0], the team width and the form rule, and the dense stage's merged q n-row CSR
matrix against a dense A + scale B^T W B on a 5 x 5 grid with q = 3 and p = 2 -- Psi with an empty row, a one-entry row, a row over every DOF, and a DOF in
no row.  All values are multiples of 1/8: the comparisons are exact.  The same stand-alone program, compiled with -fsanitize=address,undefined, comes out
clean (host code only: nothing is preloaded, no device is touched)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fdapde-core_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "cpp", "host_kron_obs_test.cpp"), os.path.join(CSRC, "host_kron_obs.cpp"), os.path.join(CSRC, "host_obs.cpp")]


def _build(tmp_path_factory, name, extra):
    path = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call(["g++", "-std=c++20", "-O2", "-Wall", "-Wextra", *extra, *SRC, "-o", path])
    return path


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory, "host_kron_obs_test", [])


@pytest.fixture(scope="module")
def exe_sanitized(tmp_path_factory):
    return _build(tmp_path_factory, "host_kron_obs_test_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


def _run(path):
    res = subprocess.run([path], capture_output=True, text=True, timeout=120)
    print(res.stdout)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "0 failures" in res.stdout
    assert res.stdout.count("off the pattern)") == 4, "all four cases of the merged matrix ran"
    return res


def test_host_kron_obs_validation_weights_and_merged_matrix(exe):
    _run(exe)


def test_host_kron_obs_under_address_and_undefined_behaviour_sanitizers(exe_sanitized):
    res = _run(exe_sanitized)
    assert "ERROR" not in res.stderr and "runtime error" not in res.stderr, res.stderr
