"""The host set-up of the 2 x 2 block handle's factored data term (csrc/host_obs.cpp: plain loops, no device) on the CPU: tests/cpp/host_obs_test.cpp,
compiled here as tests/test_host_amg.py compiles its driver.  The program checks that the validation refuses each malformed input fdapde_block_set_obs names
(a column out of range, a row that is not strictly ascending, a non-monotone rowptr, a value, weight or scale that is not finite), Psi in the internal order
and Psi^T against a dense transpose, and the dense stage's merged 2 n-row CSR matrix against a dense A + scale Psi^T W Psi on a 5 x 5 grid -- Psi with an
empty row, a one-entry row, a row covering every DOF, and a DOF in no row.  All values are multiples of 1/8: the comparisons are exact."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(ROOT, "tests", "cpp", "host_obs_test.cpp"), os.path.join(ROOT, "fdapde-core_amd", "csrc", "host_obs.cpp")]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("host_obs") / "host_obs_test")
    subprocess.check_call(["g++", "-std=c++20", "-O2", "-Wall", "-Wextra", *SRC, "-o", path])
    return path


def test_host_obs_validation_transpose_and_merged_matrix(exe):
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(res.stdout)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "0 failures" in res.stdout
    assert res.stdout.count("off the pattern)") == 3, "all three cases of the merged matrix ran"
