"""Every launch path on every kernel instantiation, at partial waves.

sr_launch_geodesic dispatches ten sr_integrate_kernel and three
sr_resume_kernel instantiations of the pinhole projection:
csrc/kernels/dispatch.h lists them and says which launch runs which, and
tests/test_dispatch.py holds that rule on the CPU (no pixel depends on it,
so nothing here can see it). tests/test_gpu_parity.py runs the launch paths on
the default scene (the small instantiation) and the other instantiations
through whole render_debug frames; this module runs the cross product on a
frame whose every wave shape is partial somewhere, plus the frame shapes,
buffer layouts, step counts and cameras the other modules never reach.

The reference of every comparison is the CPU oracle's frame of the same
scene, camera, params and size (computed once per cell, World.ref), and
nothing has a tolerance: RGBA8 bytes always, float FragColor bits and step
counts wherever the path returns them (NaN == NaN as in compare).

A. The matrix: 68x44 (5x3 workgroup tiles, a last wave column 4 pixels
   wide, a last tile row 12 rows high, six 8-row blocks, the last of 4
   rows), 400 steps, five scenes x overlay off / on x the launch paths.
B. Frame shapes from 1x1 up, padded pitch and frame stride, batch capacity.
C. Step counts 0 .. 7 and cameras at and inside the horizon.
D. Argument rejection on a live context.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import compare, stacked_layers_scene

pytestmark = pytest.mark.gpu

W, H, STEPS = 68, 44, 400
NB8 = (H + 7) // 8  # 8-row blocks of the frame
TILES = ((W + 15) // 16) * ((H + 15) // 16)
SCENES = ("small", "general", "large", "large_translucent", "stacked")
SHARES = ((0, 1), (1, 2))  # (block_first, block_step) of the batch path
LIST = [5, 0, -1, 3, -1, 2]  # block 5 holds the frame's last 4 rows
FILL = 77


class World:
    """Scenes, test rays, cameras and the oracle's frames, built once."""

    def __init__(self, pkg, oracle, textures):
        self.pkg, self.oracle = pkg, oracle
        sc, abi = pkg.scenes, pkg.abi
        bg, arr = textures
        self.tex = oracle.TextureSet(bg, arr)
        self.cams = {
            "view": sc.camera_look((0.0, 2.0, 15.0), (0.0, -2.0, -15.0)),
            "fly1": abi.camera_flyby(1.0 / 6.0, 30.0, 10.0),
            "fly5": abi.camera_flyby(5.0 / 6.0, 30.0, 10.0),
            # at and inside the horizon (section C)
            "r1.4": sc.camera_look((0.0, 0.0, 1.4), (0.3, 0.1, -1.0), fov=120.0),
            "r1.05": sc.camera_look((0.0, 0.3, 1.05), (0.3, 0.1, -1.0), fov=120.0),
            "r0.9": sc.camera_look((0.0, 0.0, 0.9), (0.3, 0.1, -1.0), fov=120.0),
        }
        self.batch = ("view", "fly1", "fly5")
        self._scenes, self._ref = {}, {}
        # the press-R polyline of test_test_ray_budget_instantiations
        cam0 = sc.camera_look((1.0, 3.0, 16.0), (0.18, -0.1, -1.0))
        fwd = list(cam0.transform.axes[6:9])
        pts = abi.test_ray_points(list(cam0.transform.pos), fwd, 600, 2)[:abi.MAX_POINTS]
        assert len(pts) == 177
        tr = abi.default_test_ray()
        tr.visible = 1
        tr.num_curved_points = len(pts)
        for i, p in enumerate(pts):
            tr.curved_points[i][0], tr.curved_points[i][1], tr.curved_points[i][2] = p
        for k in range(3):
            tr.flat_origin[k] = cam0.transform.pos[k] + fwd[k]
            tr.flat_dir[k] = fwd[k]
        self.test_rays = {False: abi.default_test_ray(), True: tr}

    def scene(self, key):
        if key not in self._scenes:
            sc, abi = self.pkg.scenes, self.pkg.abi
            self._scenes[key] = {
                "small": lambda: sc.scene_default(True),
                "general": lambda: sc.scene_random(7, n_objects=8, translucent=False, planes=False),
                "large": lambda: sc.scene_stress(),
                "large_translucent": lambda: sc.scene_random(11, n_objects=21, translucent=True, planes=True),
                "stacked": lambda: stacked_layers_scene(sc, abi),
            }[key]()
        return self._scenes[key]

    def params(self, steps=STEPS, **kw):
        return self.pkg.abi.default_params(max_steps=steps, percent_black=-1.0, crosshair=0, **kw)

    def ref(self, key, overlay, cam="view", w=W, h=H, steps=STEPS):
        """The oracle's (rgba8, float rgba, steps) of a cell, read-only."""
        k = (key, overlay, cam, w, h, steps)
        if k not in self._ref:
            out = self.oracle.render(self.scene(key), self.cams[cam], self.params(steps), w, h, self.tex,
                                     self.test_rays[overlay])
            for a in out:
                a.setflags(write=False)
            self._ref[k] = out
        return self._ref[k]

    def cam_array(self, names):
        return [self.cams[n] for n in names]


@pytest.fixture(scope="module")
def wd(pkg, oracle, textures):
    return World(pkg, oracle, textures)


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


def reset(gpu, wd):
    """The context state every test leaves behind."""
    gpu.set_split(0)
    gpu.set_latency_mode(False)
    gpu.set_culling(True)
    gpu.set_test_ray(wd.test_rays[False])


def setup(gpu, wd, key, overlay):
    gpu.set_scene(wd.scene(key))
    gpu.set_test_ray(wd.test_rays[overlay])


def host(*tensors):
    import torch

    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in tensors)


def same(got, want, label):
    """Byte equality of RGBA8 rows, with the count in the message."""
    assert got.shape == want.shape, (label, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), f"{label}: {int(bad.any(-1).sum())} of {bad[..., 0].size} pixels differ"


def overlay_pixels(b):
    rgb = b[..., :3]
    return int(((rgb == (255, 0, 0)).all(-1) | (rgb == (0, 255, 0)).all(-1)).sum())


def split_count(gpu):
    codes = gpu.last_order()
    return int(((codes >= 0) & ((codes & 0x80) != 0)).sum())


def block_rows_of(frame, first, step, h=H):
    """The rows sr_render_blocks packs for blocks first, first + step, ..."""
    parts = [frame[b * 8:min(h, b * 8 + 8)] for b in range(first, (h + 7) // 8, step)]
    return np.concatenate(parts) if parts else frame[:0]


# ---- the launch paths; `launches` > 1 repeats the launch (the last one is
# compared: it runs the order, and the split tiles, the one before learned),
# after_first runs between the first launch and the next
def path_debug(gpu, wd, key, ov, label, launches=1, after_first=None, cam="view", w=W, h=H, steps=STEPS):
    prm = wd.params(steps)
    for i in range(launches):
        f, b, s = gpu.render_debug(wd.cams[cam], prm, w, h)
        if i == 0 and after_first:
            after_first(((w + 15) // 16) * ((h + 15) // 16))
    f, b, s = host(f, b, s)
    return compare((b, f, s), wd.ref(key, ov, cam, w, h, steps), f"{label}, render_debug")


def path_rows(gpu, wd, key, ov, label):
    prm, cam = wd.params(), wd.cams["view"]
    rb, rf, rs = wd.ref(key, ov)
    for y0, y1 in ((0, H), (5, 6), (7, 25), (40, H)):
        (got,) = host(gpu.render(cam, prm, W, H, y0, y1))
        same(got, rb[y0:y1], f"{label}, render rows [{y0}, {y1})")
    f, b, s = host(*gpu.render_debug(cam, prm, W, H, 7, 25))  # the band's floats and steps too
    compare((b, f, s), (rb[7:25], rf[7:25], rs[7:25]), f"{label}, render_debug rows [7, 25)")


def path_blocks(gpu, wd, key, ov, label):
    import torch

    prm, cam = wd.params(), wd.cams["view"]
    rb = wd.ref(key, ov)[0]
    frame = np.zeros_like(rb)
    for first, step in ((0, 1), (1, 2), (2, 3), (5, 6)):
        blocks = list(range(first, NB8, step))
        out = torch.full((len(blocks) * 8, W, 4), FILL, dtype=torch.uint8, device="cuda")
        _, rows = gpu.render_blocks(cam, prm, W, H, 8, first, step, out=out)
        want = block_rows_of(rb, first, step)
        assert rows == len(want) == gpu.lib.sr_blocks_row_count(H, 8, first, step), (label, first, step, rows)
        (got,) = host(out)
        same(got[:rows], want, f"{label}, render_blocks ({first}, {step})")
        assert (got[rows:] == FILL).all(), f"{label}, render_blocks ({first}, {step}): wrote past its rows"
        k = 0
        for b in blocks:
            n = min(8, H - b * 8)
            frame[b * 8:b * 8 + n] = got[k:k + n]
            k += n
        assert k == rows
    same(frame, rb, f"{label}, render_blocks reassembled")


def path_batch(gpu, wd, key, ov, label, after_first=None, shares=SHARES):
    import torch

    prm, cams = wd.params(), wd.cam_array(wd.batch)
    refs = [wd.ref(key, ov, c)[0] for c in wd.batch]
    for first, step in shares:
        nb = len(range(first, NB8, step))
        out = torch.full((len(cams), nb * 8, W, 4), FILL, dtype=torch.uint8, device="cuda")
        for i in range(2):  # the second launch runs the learned order
            _, rows = gpu.render_blocks_batch(cams, prm, W, H, 8, first, step, out=out)
            if i == 0 and after_first:
                after_first(((W + 15) // 16) * ((nb * 8 + 15) // 16))
        (got,) = host(out)
        for f, name in enumerate(wd.batch):
            want = block_rows_of(refs[f], first, step)
            assert rows == len(want)
            same(got[f, :rows], want, f"{label}, render_blocks_batch ({first}, {step}) frame {name}")
            assert (got[f, rows:] == FILL).all(), f"{label}, batch ({first}, {step}) frame {name}: wrote past its rows"


def path_list(gpu, wd, key, ov, label, after_first=None):
    import torch

    prm, cams = wd.params(), wd.cam_array(wd.batch)
    out = torch.full((len(cams), len(LIST) * 8, W, 4), FILL, dtype=torch.uint8, device="cuda")
    for i in range(2):  # the second launch runs the learned order
        gpu.render_block_list(cams, prm, W, H, 8, LIST, out=out)
        if i == 0 and after_first:
            after_first(((W + 15) // 16) * ((len(LIST) * 8 + 15) // 16))
    (got,) = host(out)
    for f, name in enumerate(wd.batch):
        want = np.full((len(LIST) * 8, W, 4), FILL, dtype=np.uint8)  # padding and rows past the frame keep 77
        rb = wd.ref(key, ov, name)[0]
        for s, b in enumerate(LIST):
            if b >= 0:
                n = min(8, H - b * 8)
                want[s * 8:s * 8 + n] = rb[b * 8:b * 8 + n]
        same(got[f], want, f"{label}, render_block_list frame {name}")


def split_checker(gpu, max_tiles, lanes, exact):
    """The split count order_tiles left after a learning launch: max_tiles
    tiles (a frame with at least that many tiles of cost >= min_steps), or
    every such tile when max_tiles exceeds the grid, each as 64 / lanes
    workgroups."""
    S = 64 // lanes

    def check(tiles):
        n = split_count(gpu)
        if exact:
            assert n == max_tiles * S, (n, max_tiles, S)
        else:
            assert n > 0 and n % S == 0 and n <= min(max_tiles, tiles, TILES) * S, (n, tiles, S)

    return check


PATHS = ["debug", "rows", "blocks", "batch", "list",
         "split16x4", "split16x64", "split4x4", "split4x64", "split1x4", "split1x64", "split4x64min100",
         "latency", "cull_off", "wave_costs"]


def run_wave_costs(gpu, wd, key, ov, label):
    D = wd.pkg.dist
    prm, cam = wd.params(), wd.cams["view"]
    rb, rf, rs = wd.ref(key, ov)
    gpu.set_split(4, 4, 1)
    path_debug(gpu, wd, key, ov, label + ", before wave_costs")  # learns the costs
    a, = host(gpu.wave_costs(cam, prm, W, H))
    b, = host(gpu.wave_costs(cam, prm, W, H))
    assert a.shape == (NB8, (W + 7) // 8, 2) == (6, 9, 2)
    assert np.array_equal(a, b), f"{label}: two sr_wave_costs maps differ"
    pad = np.zeros((a.shape[0] * 8, a.shape[1] * 8), dtype=np.int64)
    pad[:H, :W] = rs
    mx = pad.reshape(a.shape[0], 8, a.shape[1], 8).max(axis=(1, 3))
    # the integrate kernel's count: at least the oracle's (it runs on past a
    # hit it logged as possibly translucent where the shader stops). A ray
    # whose hit log filled is continued by sr_resume_kernel, which adds its
    # steps to the map: before it did, the stacked layers (every ray resumed)
    # reported 46 of 54 waves below the oracle's count.
    assert (a[..., 0] >= mx).all(), f"{label}: wave steps below the oracle's in {int((a[..., 0] < mx).sum())} waves"
    assert (a[..., 0] <= STEPS).all()
    assert (a[..., 1] >= 0).all() and (a[..., 1][a[..., 0] == 0] == 0).all()
    lists = D.balanced_blocks(D.block_costs(a), 3)
    assert sorted(x for l in lists for x in l if x >= 0) == list(range(NB8))
    # the split setting survived and no pixel moved: a learning launch leaves
    # four split tiles again, the next one runs them
    path_debug(gpu, wd, key, ov, label + ", after wave_costs", launches=2,
               after_first=split_checker(gpu, 4, 4, True))


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("overlay", [False, True], ids=["plain", "overlay"])
@pytest.mark.parametrize("key", SCENES)
def test_matrix(gpu, wd, key, overlay, path):
    label = f"{key}, overlay {'on' if overlay else 'off'}, {path}"
    if overlay:  # the overlay is on screen (flat: green, curved: red)
        assert overlay_pixels(wd.ref(key, True)[0]) > 0
    try:
        setup(gpu, wd, key, overlay)
        if path == "debug":
            path_debug(gpu, wd, key, overlay, label)
        elif path == "rows":
            path_rows(gpu, wd, key, overlay, label)
        elif path == "blocks":
            path_blocks(gpu, wd, key, overlay, label)
        elif path == "batch":
            path_batch(gpu, wd, key, overlay, label)
        elif path == "list":
            path_list(gpu, wd, key, overlay, label)
        elif path.startswith("split"):
            lanes, _, rest = path[5:].partition("x")
            tiles, _, min_steps = rest.partition("min")
            lanes, tiles, min_steps = int(lanes), int(tiles), int(min_steps or 1)
            gpu.set_split(tiles, lanes, min_steps)
            chk = split_checker(gpu, tiles, lanes, exact=tiles == 4)
            path_debug(gpu, wd, key, overlay, label, launches=2, after_first=chk)
            path_batch(gpu, wd, key, overlay, label, after_first=chk)
            path_list(gpu, wd, key, overlay, label, after_first=chk)
        elif path == "latency":
            gpu.set_latency_mode(True)
            path_debug(gpu, wd, key, overlay, label)
            path_batch(gpu, wd, key, overlay, label)
        elif path == "cull_off":
            gpu.set_culling(False)
            path_debug(gpu, wd, key, overlay, label)
            path_batch(gpu, wd, key, overlay, label)
        else:
            run_wave_costs(gpu, wd, key, overlay, label)
    finally:
        reset(gpu, wd)


def test_batch_cameras_differ(wd):
    """The three batch frames are three pictures, in every scene."""
    for key in SCENES:
        assert len({wd.ref(key, False, c)[0].tobytes() for c in wd.batch}) == 3, key


# ---- B. frame shapes and buffers
SIZES = [(1, 1), (3, 2), (7, 5), (8, 8), (9, 9), (16, 16), (17, 9), (65, 1), (1, 65)]


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("key,overlay", [("small", False), ("large", False), ("small", True)],
                         ids=["small", "large", "small-overlay"])
def test_small_frames(gpu, wd, key, overlay, w, h):
    """Frames smaller than a workgroup tile or a wave, one pixel wide or
    high: render_debug, a two-camera batch and a launch with every tile
    split into one-ray waves."""
    import torch

    label = f"{key}, overlay {'on' if overlay else 'off'}, {w}x{h}"
    steps = 300
    prm = wd.params(steps)
    try:
        setup(gpu, wd, key, overlay)
        path_debug(gpu, wd, key, overlay, label, w=w, h=h, steps=steps)
        names = ("view", "fly1")
        nb = (h + 7) // 8
        out = torch.full((2, nb * 8, w, 4), FILL, dtype=torch.uint8, device="cuda")
        for _ in range(2):
            _, rows = gpu.render_blocks_batch(wd.cam_array(names), prm, w, h, 8, 0, 1, out=out)
        assert rows == h
        (got,) = host(out)
        for f, name in enumerate(names):
            same(got[f, :h], wd.ref(key, overlay, name, w, h, steps)[0], f"{label}, batch frame {name}")
            assert (got[f, h:] == FILL).all(), f"{label}, batch frame {name}: wrote past its rows"
        gpu.set_split(64, 1, 1)
        # a tile is split when some ray of it took a step: a ray enters the
        # step loop on the GPU exactly when it does in the oracle (1x1's one
        # ray is exactly radial and ends before the loop: nothing to split)
        rs = wd.ref(key, overlay, "view", w, h, steps)[2]
        live = sum(int(rs[y:y + 16, x:x + 16].max() >= 1) for y in range(0, h, 16) for x in range(0, w, 16))
        assert live > 0 or (w, h) == (1, 1)

        def chk(_):
            assert split_count(gpu) == live * 64, (split_count(gpu), live)

        path_debug(gpu, wd, key, overlay, label + ", split", launches=2, after_first=chk, w=w, h=h, steps=steps)
    finally:
        reset(gpu, wd)


@pytest.mark.parametrize("key", ["small", "large"])
def test_padded_pitch_and_frame_stride(gpu, wd, key):
    """sr_render, sr_render_blocks_batch and sr_render_block_list through
    ctypes with pitch = 4 W + 32 and frame stride = pitch x rows + 256, into
    the middle of a larger buffer of sentinel bytes: the payload equals the
    oracle's rows and every other byte (row padding, the gaps between
    frames, the guard bands before and after) still holds the sentinel. The
    guard bands make an overrun a changed byte instead of a fault."""
    import torch

    abi, lib = wd.pkg.abi, gpu.lib
    prm = wd.params()
    cams = wd.cam_array(wd.batch)
    arr = (abi.Camera * 3)(*cams)
    refs = [wd.ref(key, False, c)[0] for c in wd.batch]
    pitch, guard, sentinel = 4 * W + 32, 4096, 0xA5
    assert pitch % 4 == 0

    def run(label, n_frames, rows, source_rows, call):
        """source_rows[k]: the frame row output row k holds (None: unwritten)."""
        stride = pitch * rows + 256
        size = 2 * guard + n_frames * stride
        buf = torch.full((size,), sentinel, dtype=torch.uint8, device="cuda")
        want = np.full(size, sentinel, dtype=np.uint8)
        for f in range(n_frames):
            for k, y in enumerate(source_rows):
                if y is not None:
                    o = guard + f * stride + k * pitch
                    want[o:o + 4 * W] = refs[f][y].reshape(-1)
        rc = call(C.c_void_p(buf.data_ptr() + guard), stride)
        assert rc == abi.SR_OK, (label, rc)
        (got,) = host(buf)
        payload = want != sentinel  # (a payload byte may equal the sentinel: counted with the rest, harmless)
        bad = got != want
        assert not bad.any(), (f"{label}: {int((bad & payload).sum())} payload bytes differ, "
                               f"{int((bad & ~payload).sum())} bytes outside the payload changed")

    try:
        setup(gpu, wd, key, False)
        st = gpu._stream(None)
        for y0, y1 in ((0, H), (7, 25)):
            run(f"{key}, sr_render rows [{y0}, {y1})", 1, y1 - y0, list(range(y0, y1)),
                lambda p, stride: lib.sr_render(gpu.ctx, C.byref(cams[0]), C.byref(prm), W, H, y0, y1, p, pitch, st))
        first, step = 1, 2
        blocks = list(range(first, NB8, step))
        src = [b * 8 + j if b * 8 + j < H else None for b in blocks for j in range(8)]
        for _ in range(2):
            run(f"{key}, sr_render_blocks_batch", 3, len(src), src,
                lambda p, stride: lib.sr_render_blocks_batch(gpu.ctx, arr, 3, C.byref(prm), W, H, 8, first, step, p,
                                                             pitch, stride, st))
        lst = (C.c_int * len(LIST))(*LIST)
        src = [b * 8 + j if 0 <= b and b * 8 + j < H else None for b in LIST for j in range(8)]
        for _ in range(2):
            run(f"{key}, sr_render_block_list", 3, len(src), src,
                lambda p, stride: lib.sr_render_block_list(gpu.ctx, arr, 3, C.byref(prm), W, H, 8, lst, len(LIST), p,
                                                           pitch, stride, st))
    finally:
        reset(gpu, wd)


def test_batch_capacity(gpu, wd):
    """32 frames in one launch (SR_MAX_BATCH), each equal to its own
    single-frame render; 33 are refused before anything is launched."""
    import torch

    abi = wd.pkg.abi
    w, h, prm = 20, 12, wd.params(300)
    try:
        setup(gpu, wd, "small", False)
        cams = [abi.camera_flyby((f + 0.5) / 33.0, 30.0, 10.0) for f in range(33)]
        single = [host(gpu.render(c, prm, w, h))[0] for c in cams[:32]]
        assert len({s.tobytes() for s in single}) == 32
        for _ in range(2):
            out, rows = gpu.render_blocks_batch(cams[:32], prm, w, h, 8, 0, 1)
        assert rows == h
        (got,) = host(out)
        for f in range(32):
            same(got[f, :h], single[f], f"batch of 32, frame {f}")
        out = torch.full((33, 16, w, 4), FILL, dtype=torch.uint8, device="cuda")
        with pytest.raises(abi.SRError) as e:
            gpu.render_blocks_batch(cams, prm, w, h, 8, 0, 1, out=out)
        assert e.value.status == abi.SR_E_CAPACITY
        assert (host(out)[0] == FILL).all()
    finally:
        reset(gpu, wd)


# ---- C. parameter edges
@pytest.mark.parametrize("steps", [0, 1, 2, 3, 4, 5, 7])
@pytest.mark.parametrize("latency", [False, True], ids=["default", "latency"])
@pytest.mark.parametrize("w,h", [(17, 9), (W, H)], ids=["17x9", f"{W}x{H}"])
@pytest.mark.parametrize("key", ["small", "large"])
def test_small_step_counts(gpu, wd, key, w, h, latency, steps):
    """max_steps around the fast loop's four steps per iteration and latency
    mode's two (the step table holds max_steps + 4 entries and the loop
    prefetches up to four ahead; with 0 steps the loop is never entered and
    no entry is read). 17x9 is odd by odd with the camera looking at the
    hole: the centre ray is exactly radial and ends black before the loop."""
    if key == "small" and (w, h) == (17, 9) and steps == 0:  # (the stress scene has an object on that ray)
        o = wd.ref(key, False, "view", w, h, steps)
        assert (o[0][4, 8, :3] == 0).all() and o[2][4, 8] == 0  # the case is the one described
    try:
        setup(gpu, wd, key, False)
        gpu.set_latency_mode(latency)
        path_debug(gpu, wd, key, False, f"{key}, {w}x{h}, {steps} steps, latency {latency}", w=w, h=h, steps=steps)
    finally:
        reset(gpu, wd)


@pytest.mark.parametrize("cull", [True, False], ids=["cull", "cull_off"])
@pytest.mark.parametrize("cam", ["r1.4", "r1.05", "r0.9"])
@pytest.mark.parametrize("key", ["small", "large"])
def test_cameras_near_the_horizon(gpu, wd, key, cam, cull):
    """Cameras at r = 1.4 and 1.05 looking inward with a 120 degree field
    (every ray ends black in the hole after a few steps) and at r = 0.9,
    inside the horizon (every ray runs all 300 steps, none black): whole
    frames with float bits and step counts."""
    steps = 300
    o = wd.ref(key, False, cam, W, H, steps)
    black = (o[0][..., :3] == 0).all(-1)
    if key == "small":  # the cases are the ones described (the stress scene's objects reach inside r = 2)
        if cam == "r0.9":
            assert (o[2] == steps).all() and not black.any()
        else:
            assert black.all() and o[2].min() >= 1 and o[2].max() <= (33 if cam == "r1.4" else 16)
    try:
        setup(gpu, wd, key, False)
        gpu.set_culling(cull)
        path_debug(gpu, wd, key, False, f"{key}, camera {cam}, culling {cull}", cam=cam, steps=steps)
    finally:
        reset(gpu, wd)


# ---- D. argument rejection on a live context
def test_arguments_rejected_on_a_live_context(gpu, wd):
    """Each bad call returns SR_E_INVALID before any launch (sr_api.cpp:
    sr_render / sr_render_blocks_batch / sr_render_block_list check their
    own arguments, build_frame the params, the pitch and the frame stride,
    all ahead of the first stream operation), writes nothing, and leaves the
    context as it was: the good render repeats byte for byte."""
    import torch

    abi, lib = wd.pkg.abi, gpu.lib
    INV = abi.SR_E_INVALID
    try:
        setup(gpu, wd, "small", False)
        gpu.set_split(4, 4, 1)
        prm, cam = wd.params(), wd.cams["view"]
        cams = (abi.Camera * 2)(wd.cams["view"], wd.cams["fly1"])
        st = gpu._stream(None)
        for _ in range(2):
            good, = host(gpu.render(cam, prm, W, H))
        same(good, wd.ref("small", False)[0], "the good render")
        buf = torch.full((2, 48, W, 4), FILL, dtype=torch.uint8, device="cuda")
        p, pitch = C.c_void_p(buf.data_ptr()), 4 * W

        def render(params=prm, y0=0, y1=H, pitch_=pitch):
            return lib.sr_render(gpu.ctx, C.byref(cam), C.byref(params), W, H, y0, y1, p, pitch_, st)

        assert render(pitch_=pitch - 4) == INV
        assert lib.sr_render_blocks_batch(gpu.ctx, cams, 2, C.byref(prm), W, H, 8, 0, 1, p, pitch, pitch * 48 - 4,
                                          st) == INV
        assert render(y0=5, y1=4) == INV
        assert render(y1=H + 1) == INV
        assert render(params=wd.params((1 << 24))) == INV  # SR_MAX_STEPS + 1
        assert render(params=wd.params(raytrace_type=4)) == INV
        lst = (C.c_int * 3)(0, NB8, 1)  # an entry equal to the block count
        assert lib.sr_render_block_list(gpu.ctx, cams, 2, C.byref(prm), W, H, 8, lst, 3, p, pitch, pitch * 24,
                                        st) == INV
        assert lib.sr_set_split(gpu.ctx, 4, 8, 1) == INV
        assert render(y0=9, y1=9) == abi.SR_OK  # no rows: nothing is written
        assert (host(buf)[0] == FILL).all()
        again, = host(gpu.render(cam, prm, W, H))
        assert np.array_equal(again, good)
        assert split_count(gpu) == 4 * 16  # the refused sr_set_split changed nothing
    finally:
        reset(gpu, wd)


def test_zz_diag_counters_zero(gpu):
    """After every render of this module on the shared context: no pixel
    stopped at an opaque-classified hit whose shaded alpha was not 1, and no
    stream-ordered free failed."""
    assert gpu.diag_counters() == {"hit_not_opaque": 0, "free_errors": 0}
