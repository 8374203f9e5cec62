"""The context's device caches (csrc/host/device_cache.h) on the CPU.

An allocation or a copy cannot be made to fail on the GPU, so no GPU test
reaches the caches' failure paths, and the ones that walk the caches past
their capacity see only that the frames stay right. tests/cpp/
test_device_cache.cpp, built here with the host C++ compiler (no ROCm include
path, no GPU) under AddressSanitizer and UBSan, drives the generic cache and
the context's four through a counting device: hits, the LRU eviction, the key
equality of the exclusion tables, a failure injected at every allocation and
every copy of every kind, the cascade of an evicted block list, the lifetime
of the uploads' host sources, and "release everything".
"""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "schwarzschild-raytracer_amd"


def test_device_caches_against_a_counting_device(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "test_device_cache"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", f"-I{ROOT / 'include'}", f"-I{PKG / 'csrc'}",
           str(ROOT / "tests/cpp/test_device_cache.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr
    assert re.search(r"^ALL OK: \d+ checks$", res.stdout, re.M), res.stdout[-2000:]
    # every failure site of every kind ran: 2 + 2 + 4 + 2
    assert len(re.findall(r"^(?:table|xtab|order|block list): failure at ", res.stdout, re.M)) == 10


def test_the_header_has_no_hip():
    """What lets the program above build: the header, and what it includes, names no HIP header."""
    for path in (PKG / "csrc/host/device_cache.h", PKG / "csrc/host/precompute.h"):
        assert not re.search(r'#include\s*[<"]hip/', path.read_text()), path
