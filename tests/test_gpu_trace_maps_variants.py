"""sr_trace_ray_maps through the test-only libraries, as
tests/test_gpu_trace_variants.py runs sr_trace_rays through them: the second
register allocation (lib/libsr_alt.so) and the build that checks the asserted
wave-uniformity at run time (lib/libsr_chk.so). The lanes of a trace-maps
launch's waves are unrelated rays and the kernel pins nothing of a ray to an
SGPR, so the scattered sets under the rig through either library equal
libsr.so's bytes (held to the oracle by tests/test_gpu_trace_maps.py), and the
checked build counts no wave whose lanes disagree at any site it reached.
"""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import trace_cases as T
import trace_map_cases as M

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
LIBDIR = ROOT / "schwarzschild-raytracer_amd" / "lib"


@pytest.fixture(scope="module")
def tm(pkg, oracle, textures):
    return M.TraceMaps(pkg, oracle, textures)


@pytest.fixture(scope="module")
def ship(pkg, textures):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    r = pkg.Renderer(0)
    r.set_texture_array(textures[1])
    yield r
    r.close()


def other(pkg, textures, name):
    path = LIBDIR / name
    assert path.exists(), f"lib/{name} not built (make -C schwarzschild-raytracer_amd)"
    lib = pkg.abi.load(path)
    r = pkg.Renderer(0, lib=lib)
    r.set_texture_array(textures[1])
    return lib, r


def run(r, tm, key, overlay, mode, cull):
    import torch

    r.set_culling(cull)
    r.set_scene(tm.scene(key))
    r.set_test_ray(tm.tr.wd.test_rays[overlay])
    O, V, _ = tm.rays(key)
    o = torch.from_numpy(np.array(O, order="C")).cuda()  # (copies: the sets are read-only)
    v = torch.from_numpy(np.array(V, order="C")).cuda()
    got = r.trace_ray_maps(o, v, tm.params(raytrace_type=mode))
    torch.cuda.synchronize()
    r.set_culling(True)
    return {k: t.cpu().numpy() for k, t in got.items()}


CELLS = [(key, overlay, mode, cull) for key, overlay in T.SCATTERED for mode in (T.CURVED, T.FLAT)
         for cull in (True, False) if cull or mode == T.CURVED]


def test_second_register_allocation(pkg, textures, tm, ship):
    _, alt = other(pkg, textures, "libsr_alt.so")
    try:
        for cell in CELLS:
            a, b = run(ship, tm, *cell), run(alt, tm, *cell)
            for k in a:
                assert a[k].tobytes() == b[k].tobytes(), (cell, k)
    finally:
        alt.close()


def test_checked_uniformity(pkg, textures, tm, ship):
    """Read as tests/test_gpu_uniformity.py reads them: reset, launch, seen / bad per site."""
    lib, chk = other(pkg, textures, "libsr_chk.so")
    lib.sr_debug_uniform_sites.restype = C.c_int
    lib.sr_debug_uniform_site_name.restype = C.c_char_p
    lib.sr_debug_uniform_site_name.argtypes = [C.c_int]
    n = int(lib.sr_debug_uniform_sites())
    names = [lib.sr_debug_uniform_site_name(i).decode() for i in range(n)]
    try:
        assert lib.sr_debug_uniform_reset() == 0
        for cell in CELLS:
            a, b = run(ship, tm, *cell), run(chk, tm, *cell)
            for k in a:
                assert a[k].tobytes() == b[k].tobytes(), (cell, k)
        seen, bad = (C.c_uint * n)(), (C.c_uint * n)()
        assert lib.sr_debug_uniform_read(seen, bad, n) == 0
        seen, bad = np.array(seen, dtype=np.int64), np.array(bad, dtype=np.int64)
        lines = (C.c_int * n)()
        assert lib.sr_debug_uniform_lines(lines, n) == 0
        assert not bad.any(), "lanes of one wave disagree at " + "; ".join(
            f"{names[i]} (line {lines[i]}): {bad[i]} of {seen[i]} waves" for i in np.flatnonzero(bad))
        reached = {names[i] for i in np.flatnonzero(seen)}
        # what a trace-maps launch runs: the budget slots' records, the events' spent mask and the opacity test's
        # waterfall; never the lighting's waterfall (no shade), the recording kernels' start records or step index
        assert {"SLOT_TYPE", "EVENT_SPENT", "OPQ_SLOT"} <= reached, sorted(reached)
        assert not any(s.startswith(("START_", "HEAD_", "SHADE_")) or s in ("STEP_I", "FAST_KEEP", "COAST_KEEP")
                       for s in reached)
    finally:
        chk.close()
