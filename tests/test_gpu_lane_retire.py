"""Lanes retired inside the coasting loop: every pixel as before.

sr_integrate_kernel's coasting loop applies the step at which some lanes
cross u_f, reseeds them with the step loop's own reseed code and, when their
rays end there, parks them in the loop instead of taking the wave through the
slow path (geodesic.hip, SR_RETIRE_COAST). Nothing here has a tolerance: RGBA8
bytes always, float FragColor bits and step counts wherever the path returns
them, against the CPU oracle's frame of the same cell (computed once, Cells.ref);
the per-wave step and budget-event counts against a recording of the parent
commit's build (tests/golden/lane_retire_wave_costs.npz, by
tests/golden/make_lane_retire_costs.py).

tests/test_lane_retire_cases.py shows on the oracle that the base frames hold
waves whose escaping lanes end at up to 49 different steps next to captured
and object-hit lanes.

End of the loop. With the default camera no lane crosses u_f near the last
step at any max_steps: the step angle is 2 pi max_revolutions / max_steps, so
a ray's end step scales with max_steps, and the frame's last escaping lane
ends at 0.38 max_steps. The sweep over max_steps therefore also runs two
cameras aimed at the shadow's edge with max_revolutions = 1, whose rays swing
once round the hole: at every max_steps of the sweep lanes end one to four
steps before the last (asserted on the oracle).
"""
import ctypes as C
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from test_gpu_launch_matrix import FILL, NB8, World, block_rows_of, host, reset, same, split_checker
from test_gpu_parity import compare

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
COSTS = ROOT / "tests" / "golden" / "lane_retire_wave_costs.npz"
W, H = 68, 44
SIZES = [(8, 8), (16, 16), (W, H)]
STEPS = [100, 500, 2000]
UFS = [0.01, 0.05]
PATH_STEPS = 500
# (scene, camera, max_steps, u_f, overlay) of the sr_wave_costs recording
COST_CELLS = [("small", "default", n, uf, False) for n in STEPS for uf in UFS] + \
             [(k, "default", PATH_STEPS, 0.01, ov) for k in ("general", "large", "stacked") for ov in (False, True)] + \
             [("small", "default", PATH_STEPS, 0.01, True), ("small", "r3", 300, 0.01, False),
              ("small", "outside", 300, 0.05, False)]


def edge_camera(sc, degrees, fov):
    """From the default camera's place, the direction to the hole turned by
    `degrees` about y: the shadow's edge (b = 2.6 at r = 15.1) is 9.9 degrees
    off the centre."""
    pos = (0.0, 2.0, 15.0)
    d = math.sqrt(sum(x * x for x in pos))
    to = tuple(-x / d for x in pos)
    a = math.radians(degrees)
    fwd = (to[0] * math.cos(a) + to[2] * math.sin(a), to[1], -to[0] * math.sin(a) + to[2] * math.cos(a))
    return sc.camera_look(pos, fwd, fov=fov)


class Cells(World):
    """The launch matrix's world, the cameras of this module and the oracle's
    frames by (scene, overlay, camera, size, params)."""

    def __init__(self, pkg, oracle, textures):
        super().__init__(pkg, oracle, textures)
        sc, abi = pkg.scenes, pkg.abi
        self.cams.update({
            "default": abi.default_camera(),
            # outside the u_f = 0.05 sphere (r = 20): every ray reseeds at step 0 and goes on
            "outside": sc.camera_look((0.0, 3.0, 26.0), (0.0, -3.0, -26.0)),
            # at r = 3 looking at the hole: lanes fall in at different steps
            "r3": sc.camera_look((0.0, 0.4, 3.0), (0.0, -0.4, -3.0)),
            "edge1": edge_camera(sc, 10.0, 1.0),
            "edge03": edge_camera(sc, 10.1, 0.3),
        })
        self.batch = ("default", "fly1", "fly5")
        self._cells = {}

    def prm(self, steps, u_f=0.01, **kw):
        return self.params(steps, u_f=u_f, **kw)

    def cell(self, key, overlay, cam, w, h, steps, u_f=0.01, rev=2):
        k = (key, overlay, cam, w, h, steps, u_f, rev)
        if k not in self._cells:
            out = self.oracle.render(self.scene(key), self.cams[cam], self.prm(steps, u_f, max_revolutions=rev), w, h,
                                     self.tex, self.test_rays[overlay])
            for a in out:
                a.setflags(write=False)
            self._cells[k] = out
        return self._cells[k]


@pytest.fixture(scope="module")
def wd(pkg, oracle, textures):
    return Cells(pkg, oracle, textures)


@pytest.fixture(scope="module")
def gpu(pkg, textures):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    bg, arr = textures
    r = pkg.Renderer(0)
    r.set_background(bg)
    r.set_texture_array(arr)
    yield r
    r.close()


def setup(gpu, wd, key, overlay):
    gpu.set_scene(wd.scene(key))
    gpu.set_test_ray(wd.test_rays[overlay])


def debug(gpu, wd, key, overlay, cam, w, h, steps, u_f=0.01, rev=2, label="", launches=1, after_first=None):
    prm = wd.prm(steps, u_f, max_revolutions=rev)
    for k in range(launches):
        out = gpu.render_debug(wd.cams[cam], prm, w, h)
        if k == 0 and after_first:
            after_first(((w + 15) // 16) * ((h + 15) // 16))
    f, b, s = host(*out)
    return compare((b, f, s), wd.cell(key, overlay, cam, w, h, steps, u_f, rev),
                   f"{label or key}, {cam}, {w}x{h}, {steps} steps, u_f {u_f}, render_debug")


def padded(gpu, wd, key, overlay, cam, w, h, steps, u_f):
    """sr_render into the middle of a sentinel-filled buffer with a padded
    pitch: the payload equals the oracle's rows, every other byte is kept."""
    import torch

    abi, lib = wd.pkg.abi, gpu.lib
    prm, c = wd.prm(steps, u_f), wd.cams[cam]
    pitch, guard, sentinel = 4 * w + 32, 4096, 0xA5
    size = 2 * guard + pitch * h
    buf = torch.full((size,), sentinel, dtype=torch.uint8, device="cuda")
    want = np.full(size, sentinel, dtype=np.uint8)
    rb = wd.cell(key, overlay, cam, w, h, steps, u_f)[0]
    for y in range(h):
        o = guard + y * pitch
        want[o:o + 4 * w] = rb[y].reshape(-1)
    rc = lib.sr_render(gpu.ctx, C.byref(c), C.byref(prm), w, h, 0, h, C.c_void_p(buf.data_ptr() + guard), pitch,
                       gpu._stream(None))
    assert rc == abi.SR_OK, rc
    (got,) = host(buf)
    bad = got != want
    payload = want != sentinel
    assert not bad.any(), (f"{key}, {cam}, {w}x{h}, {steps} steps, u_f {u_f}, sr_render: {int((bad & payload).sum())} "
                           f"payload bytes differ, {int((bad & ~payload).sum())} bytes outside the payload changed")


# ---- base cells
@pytest.mark.parametrize("u_f", UFS)
@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_base_cells(gpu, wd, w, h, steps, u_f):
    """The default scene and camera: render_debug (RGBA8, float RGBA, step
    map) and a plain render into a padded sentinel buffer. At 100 steps lanes
    also leave by u < 0, so both kinds of exit meet in one wave."""
    try:
        setup(gpu, wd, "small", False)
        debug(gpu, wd, "small", False, "default", w, h, steps, u_f)
        padded(gpu, wd, "small", False, "default", w, h, steps, u_f)
    finally:
        reset(gpu, wd)


# ---- the end of the loop
@pytest.mark.parametrize("n0", [120, 500])
def test_end_of_loop(gpu, wd, n0):
    """16x16 at every max_steps from n0 to n0 + 8 (every place of the
    four-step iteration, and of latency mode's two): the default camera, and
    the two cameras at the shadow's edge whose lanes cross u_f one to four
    steps before the last."""
    try:
        setup(gpu, wd, "small", False)
        for n in range(n0, n0 + 9):
            before_end = set()
            for cam in ("edge1", "edge03"):
                s = wd.cell("small", False, cam, 16, 16, n, 0.01, 1)[2]
                before_end |= set((n - s[(s < n) & (s >= n - 4)]).tolist())
            assert before_end, f"{n} steps: no lane ends within the last four steps"
            if n0 == 500:
                assert before_end == {1, 2, 3, 4}, (n, before_end)
            for latency in (False, True):
                gpu.set_latency_mode(latency)
                debug(gpu, wd, "small", False, "default", 16, 16, n, label=f"latency {latency}")
                for cam in ("edge1", "edge03"):
                    debug(gpu, wd, "small", False, cam, 16, 16, n, rev=1, label=f"latency {latency}")
    finally:
        reset(gpu, wd)


# ---- other scenes and launch paths
def batch(gpu, wd, key, overlay, label, after_first=None):
    import torch

    prm, cams = wd.prm(PATH_STEPS), wd.cam_array(wd.batch)
    refs = [wd.cell(key, overlay, c, W, H, PATH_STEPS)[0] for c in wd.batch]
    assert len({r.tobytes() for r in refs}) == 3
    out = torch.full((3, NB8 * 8, W, 4), FILL, dtype=torch.uint8, device="cuda")
    for k in range(2):  # the second launch runs the learned order
        _, rows = gpu.render_blocks_batch(cams, prm, W, H, 8, 0, 1, out=out)
        if k == 0 and after_first:
            after_first(((W + 15) // 16) * ((NB8 * 8 + 15) // 16))
    assert rows == H
    (got,) = host(out)
    for f, name in enumerate(wd.batch):
        same(got[f, :H], block_rows_of(refs[f], 0, 1), f"{label}, batch frame {name}")
        assert (got[f, H:] == FILL).all(), f"{label}, batch frame {name}: wrote past its rows"


PATHS = ["debug", "batch", "split16", "split4", "split1", "latency"]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("overlay", [False, True], ids=["plain", "overlay"])
@pytest.mark.parametrize("key", ["small", "general", "large", "stacked"])
def test_scenes_and_paths(gpu, wd, key, overlay, path):
    """The small, general and large instantiations and the stacked
    translucent layers (every ray resumed), the press-R overlay off and on
    (with it flat_misses is false: a parked lane ends ST_FLAT and its ray
    origin must survive), 68x44 at 500 steps. Each cell first renders with
    culling off (the loop that tests every chord), the same frame."""
    label = f"{key}, overlay {'on' if overlay else 'off'}, {path}"
    try:
        setup(gpu, wd, key, overlay)
        gpu.set_culling(False)
        debug(gpu, wd, key, overlay, "default", W, H, PATH_STEPS, label=label + ", culling off")
        gpu.set_culling(True)
        if path == "debug":
            debug(gpu, wd, key, overlay, "default", W, H, PATH_STEPS, label=label)
            for cam in ("fly1", "fly5"):
                debug(gpu, wd, key, overlay, cam, W, H, PATH_STEPS, label=label)
        elif path == "batch":
            batch(gpu, wd, key, overlay, label)
        elif path.startswith("split"):
            lanes = int(path[5:])
            gpu.set_split(64, lanes, 1)
            chk = split_checker(gpu, 64, lanes, exact=False)
            debug(gpu, wd, key, overlay, "default", W, H, PATH_STEPS, label=label, launches=2, after_first=chk)
            batch(gpu, wd, key, overlay, label, after_first=chk)
        else:
            gpu.set_latency_mode(True)
            debug(gpu, wd, key, overlay, "default", W, H, PATH_STEPS, label=label)
            batch(gpu, wd, key, overlay, label)
    finally:
        reset(gpu, wd)


# ---- cameras
@pytest.mark.parametrize("key", ["small", "large"])
def test_camera_outside_the_u_f_sphere(gpu, wd, key):
    """From r = 26 with u_f = 0.05 (a sphere of radius 20) every ray reseeds
    at step 0 and goes on: the shared reseed code's continuing branch."""
    try:
        setup(gpu, wd, key, False)
        for steps in (300, 2000):
            debug(gpu, wd, key, False, "outside", W, H, steps, 0.05)
    finally:
        reset(gpu, wd)


@pytest.mark.parametrize("key", ["small", "large"])
def test_camera_near_the_hole(gpu, wd, key):
    """From r = 3 looking at the hole lanes fall in at different steps."""
    s = wd.cell(key, False, "r3", W, H, 300)[2]
    b = wd.cell(key, False, "r3", W, H, 300)[0]
    black = (b[..., :3] == 0).all(-1)
    assert len(np.unique(s[black])) >= 8 and not black.all()  # captured at many steps, next to other lanes
    try:
        setup(gpu, wd, key, False)
        for steps in (300, 2000):
            debug(gpu, wd, key, False, "r3", W, H, steps)
    finally:
        reset(gpu, wd)


@pytest.mark.parametrize("key,cam", [("small", "default"), ("large", "default"), ("large", "r3")],
                         ids=["scene-outside", "scene-across", "camera-inside"])
def test_u_f_02(gpu, wd, key, cam):
    """u_f = 0.2, a sphere of radius 5: the default scene lies outside it
    (from the default camera every ray starts with a reseed), the stress
    scene reaches across it, and the camera at r = 3 is inside it."""
    try:
        setup(gpu, wd, key, False)
        for steps in (300, 2000):
            debug(gpu, wd, key, False, cam, W, H, steps, 0.2)
    finally:
        reset(gpu, wd)


# ---- sr_wave_costs
def cost_key(cell):
    key, cam, steps, u_f, overlay = cell
    return f"{key}/{cam}/{steps}/{u_f}/{'overlay' if overlay else 'plain'}"


def wave_cost_maps(gpu, wd):
    out = {}
    try:
        for cell in COST_CELLS:
            key, cam, steps, u_f, overlay = cell
            setup(gpu, wd, key, overlay)
            (a,) = host(gpu.wave_costs(wd.cams[cam], wd.prm(steps, u_f), W, H))
            out[cost_key(cell)] = a.astype(np.int32)
    finally:
        reset(gpu, wd)
    return out


def test_wave_costs_as_before(gpu, wd):
    """Per 8x8 wave of the 68x44 cells, the longest ray's steps and the
    wave's budget events equal the parent commit's: no event is added,
    dropped or moved by retiring lanes in the loop."""
    want = np.load(COSTS)
    got = wave_cost_maps(gpu, wd)
    assert sorted(got) == sorted(want.files) and len(got) == len(COST_CELLS)
    assert sum(int(want[k][..., 1].sum()) for k in want.files) > 0
    bad = []
    for k in sorted(got):
        assert got[k].shape == want[k].shape == (NB8, (W + 7) // 8, 2), k
        d = got[k] != want[k]
        if d.any():
            bad.append(f"{k}: steps differ in {int(d[..., 0].sum())} waves, events in {int(d[..., 1].sum())} "
                       f"(events {int(got[k][..., 1].sum())} against {int(want[k][..., 1].sum())})")
    assert not bad, "; ".join(bad)


# ---- counters
# slow-path entries of the headline frame that were no budget event before
# lanes retired in the loop (profiles/r07/s1/prof_waves_new_0.json: 350,816
# entries, 207,642 events)
PARENT_NON_EVENT = 350816 - 207642


def test_counters_show_retirements():
    """With an SR_STATS_RETIRE build (tools/build_variant.sh retire -DSR_STATS
    -DSR_STATS_RETIRE, or SR_RETIRE_STATS_LIB): the headline frame retires
    exit steps in the loop and enters the slow path without an event less
    often than the parent did."""
    lib = Path(os.environ.get("SR_RETIRE_STATS_LIB",
                              ROOT / "schwarzschild-raytracer_amd" / "lib" / "variants" / "libsr_retire.so"))
    if not lib.exists():
        pytest.skip(f"no SR_STATS_RETIRE build at {lib} (tools/build_variant.sh retire -DSR_STATS -DSR_STATS_RETIRE)")
    p = subprocess.run([sys.executable, str(ROOT / "tools" / "stats_frame.py"), str(lib), "--retire"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])["retire"]
    print(out)
    assert out["retired_exit_steps"] > 0 and out["lanes_parked"] > 0
    assert out["non_event_slow_entries"] < PARENT_NON_EVENT


def test_zz_diag_counters_zero(gpu):
    assert gpu.diag_counters() == {"hit_not_opaque": 0, "free_errors": 0}
