"""obs_coarsen (csrc/host_obs.cpp: plain loops, no device) on the CPU: tests/cpp/host_obs_coarsen_test.cpp, compiled here as tests/test_host_obs.py compiles
its driver.  The observation matrix of the next level of an aggregation hierarchy, Psi_c = Psi P with P piecewise constant, on a 5 x 5 grid with aggregates of
1 - 4 members -- Psi with an empty row, a one-entry row, a row covering every DOF but one, a row whose entries all fall into one aggregate, and a DOF in no
row: Psi_c and Psi_c^T against the dense Psi P, (Psi P)^T W (Psi P) == P^T (Psi^T W Psi) P, the merged coarsest matrix through obs_merge_dense, and a second
level.  All values are multiples of 1/8: the comparisons are exact."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(ROOT, "tests", "cpp", "host_obs_coarsen_test.cpp"), os.path.join(ROOT, "fdapde-core_amd", "csrc", "host_obs.cpp")]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("host_obs_coarsen") / "host_obs_coarsen_test")
    subprocess.check_call(["g++", "-std=c++20", "-O2", "-Wall", "-Wextra", *SRC, "-o", path])
    return path


def test_host_obs_coarsen_against_dense(exe):
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(res.stdout)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "0 failures" in res.stdout
    assert res.stdout.count("merged coarsest matrix") == 2 and res.stdout.count("the second level") == 2, "both passes ran"
