"""Shutter frames through the test-only libraries: the second register
allocation (lib/libsr_alt.so, tests/test_gpu_allocation.py) and the build that
checks the asserted wave-uniformity at run time (lib/libsr_chk.so,
tests/test_gpu_uniformity.py). A shutter launch is the first whose frames
differ in scene, camera AND sub-pixel phase at once, so a site that took one
frame's value for the launch's would show here: a subset of
tests/test_gpu_shutter.py's cells through either library equals libsr.so's
bytes (held to the oracle there), and the checked build counts no wave whose
lanes disagree at any site it reached.
"""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from shutter_cases import Case, Shutter
from test_gpu_launch_matrix import H, W, host

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
LIBDIR = ROOT / "schwarzschild-raytracer_amd" / "lib"
TURNS = ("view", "fly1", "fly5")


@pytest.fixture(scope="module")
def sh(pkg, oracle, textures):
    return Shutter(pkg, oracle, textures)


@pytest.fixture(scope="module")
def ship(pkg, textures):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    r = pkg.Renderer(0)
    r.set_background(textures[0])
    r.set_texture_array(textures[1])
    yield r
    r.close()


def other(pkg, textures, name):
    path = LIBDIR / name
    assert path.exists(), f"lib/{name} not built (make -C schwarzschild-raytracer_amd)"
    lib = pkg.abi.load(path)
    r = pkg.Renderer(0, lib=lib)
    r.set_background(textures[0])
    r.set_texture_array(textures[1])
    return lib, r


def cells(sh):
    """(case, overlay, culling, w, h): the sequence and the own scene, slot counts that change per sub-frame,
    cameras in turn and moving, the overlay and the reference's loop"""
    return [
        (sh.case("view_k4_ss2"), False, True, W, H),
        (sh.case("flyby_k4_ss2"), True, True, W, H),
        (sh.case("own_k4_ss2"), False, True, W, H),
        (Case("mix_2x3_ss2", 2, 3, 2, [TURNS[j % 3] for j in range(6)], seq="MIX"), True, True, 33, 17),
        (Case("mix_2x3_ss3", 2, 3, 3, [TURNS[j % 3] for j in range(6)], seq="MIX"), False, False, 33, 17),
        (Case("own_1x9_ss3", 1, 9, 3, [TURNS[j % 3] for j in range(9)], own="large"), False, True, 33, 17),
    ]


def run(r, sh, case, overlay, cull, w, h):
    r.set_culling(cull)
    r.set_test_ray(sh.wd.test_rays[overlay])
    if case.seq is not None:
        r.set_scene_sequence(sh.sq.scenes(case.seq))
    else:
        r.set_scene(sh.wd.scene(case.own))
    cams = [sh.cam(c) for c in case.cams[:case.n]]
    for _ in range(2):  # the second launch runs the learned order
        t = r.render_shutter(case.first_scene, cams, case.K, sh.sq.params(), w, h, case.ss)
    band = r.render_shutter(case.first_scene, cams, case.K, sh.sq.params(), w, h, case.ss, row_begin=3, row_end=h - 2)
    acc = r.accumulate_shutter(case.first_scene, cams[:case.K], sh.sq.params(), w, h, case.ss)
    out = host(t, band, acc)
    r.set_culling(True)
    r.set_test_ray(sh.wd.test_rays[False])
    return out


def test_second_register_allocation(pkg, textures, sh, ship):
    _, alt = other(pkg, textures, "libsr_alt.so")
    try:
        for cell in cells(sh):
            a, b = run(ship, sh, *cell), run(alt, sh, *cell)
            for x, y in zip(a, b):
                assert x.tobytes() == y.tobytes(), cell[0].name
        assert alt.diag_counters() == {"hit_not_opaque": 0, "free_errors": 0}
    finally:
        alt.close()


def test_checked_uniformity(pkg, textures, sh, ship):
    """Read as tests/test_gpu_uniformity.py reads them: reset, launch, seen / bad per site."""
    lib, chk = other(pkg, textures, "libsr_chk.so")
    lib.sr_debug_uniform_sites.restype = C.c_int
    lib.sr_debug_uniform_site_name.restype = C.c_char_p
    lib.sr_debug_uniform_site_name.argtypes = [C.c_int]
    n = int(lib.sr_debug_uniform_sites())
    names = [lib.sr_debug_uniform_site_name(i).decode() for i in range(n)]
    try:
        assert lib.sr_debug_uniform_reset() == 0
        for cell in cells(sh):
            a, b = run(ship, sh, *cell), run(chk, sh, *cell)
            for x, y in zip(a, b):
                assert x.tobytes() == y.tobytes(), cell[0].name
        seen, bad = (C.c_uint * n)(), (C.c_uint * n)()
        assert lib.sr_debug_uniform_read(seen, bad, n) == 0
        seen, bad = np.array(seen, dtype=np.int64), np.array(bad, dtype=np.int64)
        lines = (C.c_int * n)()
        assert lib.sr_debug_uniform_lines(lines, n) == 0
        assert not bad.any(), "lanes of one wave disagree at " + "; ".join(
            f"{names[i]} (line {lines[i]}): {bad[i]} of {seen[i]} waves" for i in np.flatnonzero(bad))
        assert seen.any(), "the shutter launches reached no checked site"
    finally:
        chk.close()
