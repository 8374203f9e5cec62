"""Retired lanes finished once per loop exit: every pixel as before.

The coasting loop of sr_integrate_kernel parks a lane whose reseed is certain
to end its ray (geodesic.hip certain_end) without running the reseed, and
computes the chords and statuses of all such lanes together where the wave
next leaves the loop; a lane that fails the predicate runs the reseed in the
handler as before. Nothing here has a tolerance: RGBA8 bytes, float FragColor
bits and step counts against the CPU oracle's frame of the same cell
(computed once, Cells.cell), with culling on and with culling off (the loop
that tests every chord); the per-wave step and budget-event counts against a
recording of the parent commit's build
(tests/golden/lane_finish_wave_costs.npz, by
tests/golden/make_lane_finish_costs.py). Every case runs on libsr.so and on
libsr_alt.so (the same source at the other register allocation).

tests/test_lane_finish_predicate.py holds the predicate to a float32
emulation of the reseed on the CPU.
"""
from pathlib import Path

import numpy as np
import pytest

from test_gpu_lane_retire import Cells
from test_gpu_launch_matrix import FILL, block_rows_of, host, reset, same, split_checker
from test_gpu_parity import compare

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
COSTS = ROOT / "tests" / "golden" / "lane_finish_wave_costs.npz"
LIBALT = ROOT / "schwarzschild-raytracer_amd" / "lib" / "libsr_alt.so"
SIZES = [(65, 41), (128, 72)]
# 100: a step angle of 0.126, lanes also leave by u < 0; 8000: u falls by
# little more than 2^-10 of itself per step for the shallowest rays, which
# fail the predicate and run the reseed in the handler
STEPS = [100, 2000, 8000]
END_STEPS = [501, 502, 503, 504]  # every place of the four-step iteration
W, H = SIZES[0]
# (scene, camera, max_steps, u_f, max_revolutions) of the sr_wave_costs recording
COST_CELLS = [("small", "default", n, 0.01, 2) for n in STEPS] + \
             [("small", "outside", 300, 0.05, 2), ("general", "default", 2000, 0.01, 2)] + \
             [("small", "edge1", n, 0.01, 1) for n in END_STEPS[:2]]
COST_SIZE = (128, 72)


@pytest.fixture(scope="module")
def wd(pkg, oracle, textures):
    return Cells(pkg, oracle, textures)


@pytest.fixture(scope="module", params=["libsr", "libsr_alt"])
def gpu(request, pkg, textures):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    lib = None
    if request.param == "libsr_alt":
        assert LIBALT.exists(), "lib/libsr_alt.so not built (make -C schwarzschild-raytracer_amd)"
        lib = pkg.abi.load(LIBALT)
    bg, arr = textures
    r = pkg.Renderer(0, lib=lib)
    r.set_background(bg)
    r.set_texture_array(arr)
    yield r
    r.close()


def debug(gpu, wd, key, cam, w, h, steps, u_f=0.01, rev=2, label="", launches=1, after_first=None):
    prm = wd.prm(steps, u_f, max_revolutions=rev)
    for k in range(launches):
        out = gpu.render_debug(wd.cams[cam], prm, w, h)
        if k == 0 and after_first:
            after_first(((w + 15) // 16) * ((h + 15) // 16))
    f, b, s = host(*out)
    return compare((b, f, s), wd.cell(key, False, cam, w, h, steps, u_f, rev),
                   f"{label}{key}, {cam}, {w}x{h}, {steps} steps, u_f {u_f}")


def both_loops(gpu, wd, key, cam, w, h, steps, u_f=0.01, rev=2):
    """Culling off, then on: both equal the oracle, so each other."""
    gpu.set_scene(wd.scene(key))
    gpu.set_culling(False)
    debug(gpu, wd, key, cam, w, h, steps, u_f, rev, label="culling off, ")
    gpu.set_culling(True)
    debug(gpu, wd, key, cam, w, h, steps, u_f, rev)


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_default_scene(gpu, wd, w, h, steps):
    """65x41 (partial waves and partial tiles) and 128x72 of the default
    scene and camera. Most pixels escape: their lanes are parked."""
    s = wd.cell("small", False, "default", w, h, steps)[2]
    assert ((s > 1) & (s < steps)).mean() > 0.5
    try:
        both_loops(gpu, wd, "small", "default", w, h, steps)
    finally:
        reset(gpu, wd)


def test_reseeds_that_go_on(gpu, wd):
    """u_f = 0.05, a sphere of radius 20, and the camera at r = 26.2: every
    ray is below u_f at step 0, and those whose line enters the sphere are
    reseeded there and go on (asserted on the oracle: they take more than one
    step), cross it and end on its far side."""
    cam = wd.cams["outside"]
    assert sum(x * x for x in cam.transform.pos) > (1.0 / 0.05) ** 2
    s = wd.cell("small", False, "outside", W, H, 300, 0.05)[2]
    assert (s > 1).any()
    try:
        both_loops(gpu, wd, "small", "outside", W, H, 300, 0.05)
    finally:
        reset(gpu, wd)


@pytest.mark.parametrize("n", END_STEPS)
def test_loop_ends_with_lanes_parked(gpu, wd, n):
    """A camera at the shadow's edge with one revolution: lanes cross u_f one
    to four steps before the last while their wave-mates run to max_steps, so
    the loop ends with lanes parked (asserted on the oracle)."""
    s = wd.cell("small", False, "edge1", W, H, n, 0.01, 1)[2]
    assert (s == n).any() and ((s < n) & (s >= n - 4)).any()
    tiles = [s[y:y + 8, x:x + 8] for y in range(0, H, 8) for x in range(0, W, 8)]
    assert any((t == n).any() and ((t < n) & (t > n // 4)).any() for t in tiles)
    try:
        both_loops(gpu, wd, "small", "edge1", W, H, n, rev=1)
    finally:
        reset(gpu, wd)


def test_batch_of_two_cameras(gpu, wd):
    """Two frames with different cameras in one launch, twice (the second
    launch runs the learned order)."""
    import torch

    names = ("default", "fly5")
    prm, cams = wd.prm(2000), wd.cam_array(names)
    refs = [wd.cell("small", False, c, W, H, 2000)[0] for c in names]
    assert refs[0].tobytes() != refs[1].tobytes()
    nb8 = (H + 7) // 8
    try:
        gpu.set_scene(wd.scene("small"))
        out = torch.full((2, nb8 * 8, W, 4), FILL, dtype=torch.uint8, device="cuda")
        for _ in range(2):
            _, rows = gpu.render_blocks_batch(cams, prm, W, H, 8, 0, 1, out=out)
        assert rows == H
        (got,) = host(out)
        for f, name in enumerate(names):
            same(got[f, :H], block_rows_of(refs[f], 0, 1, H), f"batch frame {name}")
            assert (got[f, H:] == FILL).all(), f"batch frame {name}: wrote past its rows"
    finally:
        reset(gpu, wd)


@pytest.mark.parametrize("lanes", [4, 16])
def test_split_tiles(gpu, wd, lanes):
    """The costliest tiles run as sparse waves, `lanes` live lanes each and
    the rest idle from the start."""
    try:
        gpu.set_scene(wd.scene("small"))
        gpu.set_split(64, lanes, 1)
        debug(gpu, wd, "small", "default", W, H, 2000, launches=2,
              after_first=split_checker(gpu, 64, lanes, exact=False), label=f"split {lanes}, ")
    finally:
        reset(gpu, wd)


@pytest.mark.parametrize("steps", [500, 2000])
def test_eight_slot_scene(gpu, wd, steps):
    """Eight objects: the general instantiation."""
    try:
        both_loops(gpu, wd, "general", "default", W, H, steps)
    finally:
        reset(gpu, wd)


# ---- sr_wave_costs
def cost_key(cell):
    key, cam, steps, u_f, rev = cell
    return f"{key}/{cam}/{steps}/{u_f}/{rev}"


def wave_cost_maps(gpu, wd):
    out = {}
    w, h = COST_SIZE
    try:
        for cell in COST_CELLS:
            key, cam, steps, u_f, rev = cell
            gpu.set_scene(wd.scene(key))
            (a,) = host(gpu.wave_costs(wd.cams[cam], wd.prm(steps, u_f, max_revolutions=rev), w, h))
            out[cost_key(cell)] = a.astype(np.int32)
    finally:
        reset(gpu, wd)
    return out


def test_wave_costs_as_before(gpu, wd):
    """Per 8x8 wave of the 128x72 cells, the longest ray's steps and the
    wave's budget events equal the parent commit's: finishing parked lanes
    later adds, drops or moves no event."""
    want = np.load(COSTS)
    got = wave_cost_maps(gpu, wd)
    assert sorted(got) == sorted(want.files) and len(got) == len(COST_CELLS)
    assert sum(int(want[k][..., 1].sum()) for k in want.files) > 0
    w, h = COST_SIZE
    bad = []
    for k in sorted(got):
        assert got[k].shape == want[k].shape == ((h + 7) // 8, (w + 7) // 8, 2), k
        d = got[k] != want[k]
        if d.any():
            bad.append(f"{k}: steps differ in {int(d[..., 0].sum())} waves, events in {int(d[..., 1].sum())} "
                       f"(events {int(got[k][..., 1].sum())} against {int(want[k][..., 1].sum())})")
    assert not bad, "; ".join(bad)


def test_zz_diag_counters_zero(gpu):
    assert gpu.diag_counters() == {"hit_not_opaque": 0, "free_errors": 0}
