"""The start table: the camera-only start budgets, once per launch and frame.

sr_launch_geodesic fills one sr_dev_start record per frame of the batch
(sr_start_table_kernel) before the integrate kernel, whose rays read their
start budgets from it (budget_start) instead of each wave computing them
from the camera (budget_init). Nothing here has a tolerance: frames equal
the CPU oracle's (RGBA8 always; float FragColor bits and step counts from
render_debug), outputs of launches in flight equal the same launch alone,
and the per-wave step and budget-event counts equal those recorded from a
build of the parent commit (tests/golden/start_table_wave_costs.npz, by
tests/golden/make_start_table_costs.py): equal event counts are the evidence
that the budgets are the same bits, not merely conservative ones.

Shapes are the launch matrix's: 68x44 (partial waves and tiles), 400 steps.
"""
from pathlib import Path

import numpy as np
import pytest

from test_gpu_launch_matrix import FILL, H, NB8, STEPS, W, World, host, reset, same, setup
from test_gpu_parity import compare

pytestmark = pytest.mark.gpu

COSTS = Path(__file__).resolve().parent / "golden" / "start_table_wave_costs.npz"
COST_SCENES = ("small", "general", "large", "large_translucent", "stacked")
COST_CAMS = ("view", "fly1", "r1.05")
# one batch, cameras of different regimes of the start code
MIXED = ("view", "fly1", "fly5", "r1.05", "r0.9", "far", "tube", "rect")


def start_world(pkg, oracle, textures):
    """The launch matrix's world plus the cameras of MIXED. The default
    scene's cylinder is the tube x^2 + z^2 = 4, 10 <= y <= 15, its rectangle
    lies in the plane y = 0 (0 <= x <= 3, 10 <= z <= 12)."""
    wd = World(pkg, oracle, textures)
    sc = pkg.scenes
    s = wd.scene("small")
    cyl, rect = s.cylinders[0], s.rectangles[0]
    assert list(cyl.transform.pos) == [0.0, 10.0, 0.0] and (cyl.height, cyl.radius) == (5.0, 2.0)
    assert list(cyl.transform.axes[3:6]) == [0.0, 1.0, 0.0]
    assert list(rect.plane.transform.pos) == [0.0, 0.0, 10.0] and list(rect.plane.transform.axes[3:6]) == [0.0, 1.0, 0.0]
    wd.cams.update({
        # beyond r = 100: the launch's win_ok is 0 (no u window for the hole)
        "far": sc.camera_look((0.0, 20.0, 150.0), (0.0, -20.0, -150.0)),
        # inside the cylinder's tube, off its axis, looking down it at the hole
        "tube": sc.camera_look((0.5, 12.0, 0.3), (-0.1, -1.0, -0.05)),
        # 0.07 above the rectangle's plane, over the rectangle, looking along it
        "rect": sc.camera_look((1.2, 0.07, 11.5), (0.1, -0.05, -1.0)),
    })
    return wd


@pytest.fixture(scope="module")
def wd(pkg, oracle, textures):
    return start_world(pkg, oracle, textures)


def new_renderer(pkg, textures):
    bg, arr = textures
    r = pkg.Renderer(0)
    r.set_background(bg)
    r.set_texture_array(arr)
    return r


@pytest.fixture(scope="module")
def gpu(pkg, textures):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    r = new_renderer(pkg, textures)
    yield r
    r.close()


@pytest.mark.parametrize("overlay", [False, True], ids=["plain", "overlay"])
@pytest.mark.parametrize("key", ["small", "general", "large"])
def test_mixed_batch(gpu, wd, key, overlay):
    """One sr_render_blocks_batch launch of eight cameras of different
    regimes: every frame equals the oracle's; then each camera alone through
    render_debug, with float bits and step counts."""
    import torch

    label = f"{key}, overlay {'on' if overlay else 'off'}"
    prm = wd.params()
    refs = {c: wd.ref(key, overlay, c) for c in MIXED}
    assert len({refs[c][0].tobytes() for c in MIXED}) == len(MIXED)  # eight different pictures
    try:
        setup(gpu, wd, key, overlay)
        out = torch.full((len(MIXED), NB8 * 8, W, 4), FILL, dtype=torch.uint8, device="cuda")
        for _ in range(2):  # the second launch runs the learned order
            _, rows = gpu.render_blocks_batch(wd.cam_array(MIXED), prm, W, H, 8, 0, 1, out=out)
        assert rows == H
        (got,) = host(out)
        for f, c in enumerate(MIXED):
            same(got[f, :H], refs[c][0], f"{label}, mixed batch frame {f} ({c})")
            assert (got[f, H:] == FILL).all(), f"{label}, mixed batch frame {f} ({c}): wrote past its rows"
        for c in MIXED:
            f_, b_, s_ = host(*gpu.render_debug(wd.cams[c], prm, W, H))
            compare((b_, f_, s_), refs[c], f"{label}, camera {c} alone, render_debug")
    finally:
        reset(gpu, wd)


@pytest.mark.parametrize("key", ["small", "large"])
def test_full_capacity(gpu, wd, key):
    """32 frames (SR_MAX_BATCH) of 32 distinct flyby cameras at 20x12: frame
    f of the batch equals a single-frame render of cams[f]."""
    abi = wd.pkg.abi
    w, h, prm = 20, 12, wd.params()
    try:
        setup(gpu, wd, key, False)
        cams = [abi.camera_flyby((f + 0.25) / 32.0, 30.0, 10.0) for f in range(32)]
        single = [host(gpu.render(c, prm, w, h))[0] for c in cams]
        assert len({s.tobytes() for s in single}) == 32
        for _ in range(2):
            out, rows = gpu.render_blocks_batch(cams, prm, w, h, 8, 0, 1)
        assert rows == h
        (got,) = host(out)
        for f in range(32):
            same(got[f, :h], single[f], f"{key}, batch of 32, frame {f}")
    finally:
        reset(gpu, wd)


def test_table_rebuilt_per_launch_in_stream_order(gpu, wd):
    """Launches back to back on one context and stream with no host
    synchronisation between them, changing in turn the camera, max_steps,
    max_revolutions and the scene (small -> large -> small): each output
    equals that launch rendered alone (and the oracle's frame where the
    launch matrix holds one)."""
    import torch

    abi = wd.pkg.abi
    p400 = wd.params()
    p300 = wd.params(300)
    prev = wd.params(STEPS, max_revolutions=abi.default_params().max_revolutions + 1)
    seq = [("small", "view", p400), ("small", "fly1", p400), ("small", "fly1", p300), ("small", "fly1", prev),
           ("large", "fly1", prev), ("large", "view", p400), ("small", "view", p400), ("small", "r1.05", p300)]
    try:
        gpu.set_test_ray(wd.test_rays[False])
        alone = []
        for key, cam, prm in seq:
            gpu.set_scene(wd.scene(key))
            (a,) = host(gpu.render(wd.cams[cam], prm, W, H))
            alone.append(a)
        same(alone[0], wd.ref("small", False, "view")[0], "alone: small, view")
        same(alone[4 + 1], wd.ref("large", False, "view")[0], "alone: large, view")
        assert len({alone[k].tobytes() for k in (0, 1, 4, 5)}) == 4  # the cameras and scenes give different pictures
        torch.cuda.synchronize()
        outs = []
        cur = None
        for key, cam, prm in seq:  # no synchronisation of the test's own from here ...
            if key != cur:
                gpu.set_scene(wd.scene(key))
                cur = key
            outs.append(gpu.render(wd.cams[cam], prm, W, H))
        got = host(*outs)  # ... to here
        for k, (key, cam, prm) in enumerate(seq):
            same(got[k], alone[k], f"launch {k} ({key}, {cam}, {prm.max_steps} steps, {prm.max_revolutions} rev)")
    finally:
        reset(gpu, wd)


def test_one_table_per_context(gpu, wd, pkg, textures):
    """Two contexts on two streams, launches interleaved, different cameras
    and scenes: each output equals its own launch alone."""
    import torch

    prm = wd.params()
    other = new_renderer(pkg, textures)
    try:
        gpu.set_test_ray(wd.test_rays[False])
        other.set_test_ray(wd.test_rays[False])
        gpu.set_scene(wd.scene("small"))
        other.set_scene(wd.scene("large"))
        plan = [(gpu, "small", "view"), (other, "large", "fly1"), (gpu, "small", "fly5"), (other, "large", "view"),
                (gpu, "small", "rect"), (other, "large", "tube"), (gpu, "small", "fly1"), (other, "large", "fly5")]
        alone = [host(r.render(wd.cams[cam], prm, W, H))[0] for r, key, cam in plan]
        for k, (r, key, cam) in enumerate(plan):
            same(alone[k], wd.ref(key, False, cam)[0], f"alone: {key}, {cam}")
        torch.cuda.synchronize()
        streams = {id(gpu): torch.cuda.Stream(), id(other): torch.cuda.Stream()}
        # two rounds, both kept alive: no buffer is reused while a launch may still write it
        rounds = [[r.render(wd.cams[cam], prm, W, H, stream=streams[id(r)]) for r, key, cam in plan] for _ in range(2)]
        got = host(*rounds[1])
        for k, (r, key, cam) in enumerate(plan):
            same(got[k], alone[k], f"interleaved launch {k} ({key}, {cam})")
    finally:
        other.close()
        reset(gpu, wd)


def wave_cost_maps(gpu, wd):
    """sr_wave_costs (per 8x8 wave: the longest ray's steps, budget events)
    of COST_SCENES x COST_CAMS x overlay off / on at 68x44, 400 steps. The
    overlay's map is priced by the instantiation without the test ray's
    budget: recorded as it is."""
    out = {}
    prm = wd.params()
    try:
        for key in COST_SCENES:
            for overlay in (False, True):
                setup(gpu, wd, key, overlay)
                for cam in COST_CAMS:
                    (a,) = host(gpu.wave_costs(wd.cams[cam], prm, W, H))
                    out[f"{key}/{cam}/{'overlay' if overlay else 'plain'}"] = a.astype(np.int32)
    finally:
        reset(gpu, wd)
    return out


def test_same_budgets_as_before(gpu, wd):
    """The per-wave steps and budget events equal the parent commit's."""
    want = np.load(COSTS)
    got = wave_cost_maps(gpu, wd)
    assert sorted(got) == sorted(want.files) and len(got) == 30
    assert sum(int(want[k][..., 1].sum()) for k in want.files) > 0  # events were recorded
    bad = []
    for k in sorted(got):
        assert got[k].shape == want[k].shape == (NB8, (W + 7) // 8, 2), k
        d = got[k] != want[k]
        if d.any():
            bad.append(f"{k}: steps differ in {int(d[..., 0].sum())} waves, events in {int(d[..., 1].sum())} "
                       f"(events {int(got[k][..., 1].sum())} against {int(want[k][..., 1].sum())})")
    assert not bad, "; ".join(bad)


def test_zz_diag_counters_zero(gpu):
    assert gpu.diag_counters() == {"hit_not_opaque": 0, "free_errors": 0}
