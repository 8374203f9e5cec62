"""sr_ray_maps through the test-only libraries: the second register
allocation (lib/libsr_alt.so, tests/test_gpu_allocation.py) and the build that
checks the asserted wave-uniformity at run time (lib/libsr_chk.so,
tests/test_gpu_uniformity.py). The ray-map kernels assert no wave-uniformity
of their own (they load object data per lane), and the pixels their resume
kernel walks on come from a worklist in any order: the maps through either
library equal libsr.so's bytes (held to the oracle by
tests/test_gpu_ray_maps.py), and the checked build counts no wave whose lanes
disagree at any site its launches reached.
"""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import test_gpu_ray_maps as M

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
LIBDIR = ROOT / "schwarzschild-raytracer_amd" / "lib"
# (scene, camera, culling, params): the stacked layers (every pixel through the resume kernel), translucent
# objects among 21, the textured and normal-mapped primitives, flat and split rays, the reference's loop
CELLS = [("stacked-through", "view", True, {}), ("large", "view", True, {}), ("features", "box", True, {}),
         ("default-rig", "view", True, {"raytrace_type": 2, "curved_percentage": 0.5}),
         ("default-rig", "view", True, {"raytrace_type": 1}), ("stacked-through", "view", False, {}),
         ("small", "fly1", False, {})]


@pytest.fixture(scope="module")
def cells(pkg, oracle, textures):
    return M.Cells(pkg, oracle, textures)


@pytest.fixture(scope="module")
def ship(pkg, cells):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    r = pkg.Renderer(0)
    r.set_background(cells.sky)
    yield r
    r.close()


def other(pkg, cells, name):
    path = LIBDIR / name
    assert path.exists(), f"lib/{name} not built (make -C schwarzschild-raytracer_amd)"
    lib = pkg.abi.load(path)
    r = pkg.Renderer(0, lib=lib)
    r.set_background(cells.sky)
    return lib, r


def run(r, cells, key, cam, cull, prm):
    r.set_culling(cull)
    m = M.launch(r, cells, key, cam, **prm)
    r.set_culling(True)
    return m


def same_maps(a, b, cell):
    for k in M.MAPS + ("pick",):
        assert a[k].tobytes() == b[k].tobytes(), (cell, k)


def test_second_register_allocation(pkg, cells, ship):
    _, alt = other(pkg, cells, "libsr_alt.so")
    try:
        for cell in CELLS:
            same_maps(run(ship, cells, *cell), run(alt, cells, *cell), cell)
    finally:
        alt.close()


def test_checked_uniformity(pkg, cells, ship):
    """Read as tests/test_gpu_uniformity.py reads them: reset, launch, seen / bad per site."""
    lib, chk = other(pkg, cells, "libsr_chk.so")
    lib.sr_debug_uniform_sites.restype = C.c_int
    lib.sr_debug_uniform_site_name.restype = C.c_char_p
    lib.sr_debug_uniform_site_name.argtypes = [C.c_int]
    n = int(lib.sr_debug_uniform_sites())
    names = [lib.sr_debug_uniform_site_name(i).decode() for i in range(n)]
    try:
        assert lib.sr_debug_uniform_reset() == 0
        for cell in CELLS:
            same_maps(run(ship, cells, *cell), run(chk, cells, *cell), cell)
        seen, bad = (C.c_uint * n)(), (C.c_uint * n)()
        assert lib.sr_debug_uniform_read(seen, bad, n) == 0
        seen, bad = np.array(seen, dtype=np.int64), np.array(bad, dtype=np.int64)
        lines = (C.c_int * n)()
        assert lib.sr_debug_uniform_lines(lines, n) == 0
        assert not bad.any(), "lanes of one wave disagree at " + "; ".join(
            f"{names[i]} (line {lines[i]}): {bad[i]} of {seen[i]} waves" for i in np.flatnonzero(bad))
        reached = {names[i] for i in np.flatnonzero(seen)}
        # the resume path's rounds run the budget slots' records, the events' spent mask and the opacity waterfall
        assert {"SLOT_TYPE", "EVENT_SPENT", "OPQ_SLOT"} <= reached, sorted(reached)
    finally:
        chk.close()
