"""The launch dispatch (csrc/kernels/dispatch.h) on the CPU.

Which instantiation a launch runs changes no pixel (every instantiation is
exact), so no parity test can see a wrong selection; the frame time alone
moves. tests/cpp/test_dispatch.cpp, built here with the host C++ compiler
(host code only: it links nothing, no GPU), holds the selection and the
launchers' argument checks to the rules written out row by row, over the
whole product of what they read, and prints the table of instantiated kinds.
The table is then held to what was compiled: the kernel symbols of the built
libraries.
"""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "schwarzschild-raytracer_amd"
COUNTS = {"sr_integrate_kernel": 27, "sr_resume_kernel": 5, "sr_shade_kernel": 3, "sr_trace_kernel": 3}


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """The program's table: the demangled names of the instantiated kernels, in the lists' order."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("dispatch") / "test_dispatch"
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", f"-I{ROOT / 'include'}", f"-I{PKG / 'csrc'}",
           str(ROOT / "tests/cpp/test_dispatch.cpp"), "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr
    assert "ALL OK" in res.stdout
    return [line for line in res.stdout.splitlines() if re.match(r"sr_\w+_kernel<", line)]


def test_dispatch_rules_and_table(table):
    """The rules, the soundness of every selection, no dead and no missing kind (asserted by the
    program); the table holds the counted kinds, each once."""
    assert len(set(table)) == len(table)
    for family, n in COUNTS.items():
        assert sum(name.startswith(family + "<") for name in table) == n, family
    assert len(table) == sum(COUNTS.values())


@pytest.mark.parametrize("lib", ["libsr.so", "libsr_alt.so"])
def test_table_is_what_was_compiled(table, lib):
    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("no nm")
    path = PKG / "lib" / lib
    assert path.exists(), path
    out = subprocess.run([nm, "-C", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
    built = re.findall(r"^\S+ V void (sr_(?:integrate|resume|shade|trace)_kernel<[^>]*>)\(", out, re.M)
    assert len(set(built)) == len(built)
    for family, n in COUNTS.items():
        assert sum(name.startswith(family + "<") for name in built) == n, family
    assert set(built) == set(table), sorted(set(built) ^ set(table))
