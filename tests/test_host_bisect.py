"""The coordinate bisection that cuts the single-launch CG's interior rows into blocks (csrc/host_bisect.cpp), on the CPU: structured squares
and cubes, odd workgroup counts included.  tests/cpp/host_bisect_test.cpp checks that the partition is a permutation, that the blocks' row
counts add up, that two runs agree, that every split leaves its left half within one maximal row cost of its share, and that on the 59^3 / 64
and 80^3 / 256 cases fewer entries cross a block boundary than with equal-cost chunks of the internal order; then it replays the operator application of layouts
built on bisection blocks (plain and symmetric storage, with and without Dirichlet rows) against the CSR product of the real pattern."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fdapde-core_amd", "csrc")
SRC = [os.path.join(ROOT, "tests", "cpp", "host_bisect_test.cpp")] + [os.path.join(CSRC, f) for f in ("host_bisect.cpp", "host_persist.cpp", "host_setup.cpp", "tables.cpp")]


def test_host_bisection_partitions_grids(tmp_path):
    exe = str(tmp_path / "host_bisect_test")
    subprocess.check_call(["g++", "-std=c++20", "-O2", "-Wall", *SRC, "-pthread", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("ok ")]
    assert len(lines) == 12, out.stdout
    print(out.stdout)
