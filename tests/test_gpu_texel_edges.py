"""The step loop's opacity classification at texel-scale alpha edges.

hit_opacity_uniform (geodesic.hip) ends a ray at a textured hit when a
per-texel bitmap built at upload (precompute.cpp opacity_bits: every texel
within SR_OPQ_RADIUS = 2 of this one, wrapping like the sampler, has alpha
255) says the bilinear footprint reads alpha 1 exactly; it locates the
footprint with a binary32 approximation of the shaded uv. The other suites'
textures have opaque cells hundreds of texels wide. Here the arrays are 1x1
to 37x21 texels, two layers, random colours, and the alpha patterns put an
edge within the bitmap's radius of most texels:

  checker  255 / 0 per texel: no texel's neighbourhood is opaque
  pinhole  isolated 254 texels in a sea of 255
  islands  5x5 islands of 255 on an 8-texel period: one safe texel each
  seam     255 except the last column and the first row: the wrap-around

plus a 3-channel array (alpha 1 everywhere) and an array whose layer 0 is
smaller than the array (texture_sizes < max_texture_size: alpha-0 padding).
Widths 1, 3, 7, 13, 37 are no multiples of 8 (the bitmap's (w + 7) / 8
stride). Materials use texture_index 0, 1, 2 (clamped to the last layer) and
11 (>= SR_MAX_TEXTURES: sizes of layer 0) and the uv flags singly and
together; one textured primitive of each type fills a good part of a 64x40
frame, so a texel spans several pixels; both filter modes.

Every frame: bit-exact against the oracle with the same array (RGBA8, float
bits, step counts), culling on = culling off, diagnostic counters zero (no
ray stopped at a hit whose shaded alpha was not 1). A ray stopped too early
or too late changes its pixel and its step count.

Non-vacuity (stop_pass_shares, from oracle frames alone, also run without a
GPU by tests/test_scene_extremes_cases.py): for pinhole, islands and seam at
7x5 and above on the rectangle and the sphere, at least 2 % of the frame's
rays stop at the textured surface and at least 2 % pass through it.
"""
import ctypes as C

import numpy as np
import pytest

import extreme_cases as X
from test_gpu_parity import compare

pytestmark = pytest.mark.gpu

W, H = X.W, X.H
SIZES = [(1, 1), (3, 2), (7, 5), (13, 9), (37, 21)]  # (w, h)
PATTERNS = ["checker", "pinhole", "islands", "seam"]
PINHOLE_PERIOD = 4  # a 2x2 footprint holds a pinhole at 4 of 16 positions
TEXTURE_INDICES = [0, 1, 2, 11]
UV_FLAGS = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)]  # swap_uvs, invert_uv_x, invert_uv_y
COMBOS = [(t, f) for t in TEXTURE_INDICES for f in UV_FLAGS]

CAMERA, FACING, OBJECTS = X.TEXEL_CAMERA, X.TEXEL_FACING, X.TEXEL_OBJECTS
NON_VACUOUS = ("rectangle", "sphere")


def alpha_pattern(pattern, w, h):
    x = np.arange(w)[None, :] + 0 * np.arange(h)[:, None]
    y = 0 * np.arange(w)[None, :] + np.arange(h)[:, None]
    if pattern == "checker":
        return np.where((x + y) % 2 == 0, 255, 0)
    if pattern == "pinhole":
        return np.where((x % PINHOLE_PERIOD == 1) & (y % PINHOLE_PERIOD == 1), 254, 255)
    if pattern == "islands":
        return np.where((x % 8 < 5) & (y % 8 < 5), 255, 0)
    if pattern == "seam":
        return np.where((x == w - 1) | (y == 0), 0, 255)
    if pattern == "opaque":
        return np.full((h, w), 255)
    if pattern == "clear":
        return np.zeros((h, w), dtype=np.int64)
    raise ValueError(pattern)


def texture_array(pattern, w, h, channels=4):
    """[2, h, w, channels] uint8: random colours (a fixed seed per size), the
    pattern's alpha on layer 0 and the same pattern rolled by (1, 2) on layer 1."""
    rng = np.random.default_rng(1000 * w + h)
    arr = rng.integers(0, 256, size=(2, h, w, channels), dtype=np.uint8)
    if channels == 4:
        a = alpha_pattern(pattern, w, h)
        arr[0, :, :, 3] = a
        arr[1, :, :, 3] = np.roll(a, (1, 2), axis=(0, 1))
    return np.ascontiguousarray(arr)


def padded_array(w, h, inner):
    """Layer 0 an inner (w, h) image with the seam pattern, alpha-0 padding
    around it (scenes.pad_texture_array's layout); layer 1 the full size."""
    arr = texture_array("seam", w, h)
    iw, ih = inner
    arr[0, :, :, 3] = 0
    arr[0, :ih, :iw, 3] = alpha_pattern("seam", iw, ih)
    return arr


def textured_scene(pkg, obj, sizes, max_size, texture_index, flags):
    s = X.scene_alone(pkg, OBJECTS[obj])
    m = s.materials[0]
    m.texture_index = texture_index
    m.swap_uvs, m.invert_uv_x, m.invert_uv_y = flags
    for i in range(pkg.abi.MAX_TEXTURES):
        w, h = sizes[min(i, len(sizes) - 1)]
        s.texture_sizes[i][0], s.texture_sizes[i][1] = float(w), float(h)
    s.max_texture_size[0], s.max_texture_size[1] = float(max_size[0]), float(max_size[1])
    return s


def camera(pkg):
    pos, target, fov = CAMERA
    return pkg.scenes.camera_look(pos, tuple(t - p for p, t in zip(pos, target)), fov=fov)


def params_of(pkg, filter_mode):
    return pkg.abi.default_params(max_steps=400, max_revolutions=2, percent_black=-1.0, filter_mode=filter_mode)


def array_cases():
    """(id, array, texture_sizes per layer, max_texture_size)"""
    out = []
    for pattern in PATTERNS:
        for w, h in SIZES:
            out.append((f"{pattern}-{w}x{h}", texture_array(pattern, w, h), [(w, h)], (w, h)))
    out.append(("rgb-13x9", texture_array("opaque", 13, 9, channels=3), [(13, 9)], (13, 9)))
    out.append(("padded-13x9", padded_array(13, 9, (9, 6)), [(9, 6), (13, 9)], (13, 9)))
    return out


ARRAY_CASES = array_cases()


def combo_of(case_index, obj_index):
    """Every (texture_index, uv flags) pair meets every object over the cases."""
    return COMBOS[(case_index + 3 * obj_index) % len(COMBOS)]


def stop_pass_shares(pkg, oracle, bg, pattern, size, obj, texture_index, flags):
    """From oracle frames alone: the share of the frame's rays that stop at
    the textured surface and the share that pass through it. The surface
    matters where the step maps of the same array at alpha 255 everywhere and
    0 everywhere differ; there a ray stopped if its step count is the all-255
    one."""
    w, h = size
    scene = textured_scene(pkg, obj, [size], size, texture_index, flags)
    cam, params = camera(pkg), params_of(pkg, 0)
    steps = {}
    for p in (pattern, "opaque", "clear"):
        steps[p] = oracle.render(scene, cam, params, W, H, oracle.TextureSet(bg, texture_array(p, w, h)))[2]
    on = steps["opaque"] != steps["clear"]
    stop = on & (steps[pattern] == steps["opaque"])
    went = on & (steps[pattern] != steps["opaque"])
    return float(stop.mean()), float(went.mean())


def non_vacuous_cells():
    return [(p, s, o) for p in ("pinhole", "islands", "seam") for s in SIZES if s[0] >= 7 and s[1] >= 5
            for o in NON_VACUOUS]


@pytest.fixture(scope="module")
def gpu(pkg, textures):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    r = pkg.Renderer(0)
    r.set_background(textures[0])
    r.set_test_ray(pkg.abi.default_test_ray())
    yield r
    r.close()


def gpu_frames(gpu, cam, params):
    import torch

    outs = []
    for cull in (True, False):
        gpu.set_culling(cull)
        f, b, s = gpu.render_debug(cam, params, W, H)
        torch.cuda.synchronize()
        outs.append((b.cpu().numpy(), f.cpu().numpy(), s.cpu().numpy()))
    gpu.set_culling(True)
    return outs


def check_frame(gpu, oracle, otex, scene, cam, params, label):
    assert gpu.lib.sr_set_scene(gpu.ctx, C.byref(scene)) == 0
    culled, unculled = gpu_frames(gpu, cam, params)
    o = oracle.render(scene, cam, params, W, H, otex)
    compare(culled, o, label)
    for a, b, what in zip(culled, unculled, ("rgba8", "float", "steps")):
        assert np.array_equal(a.view(np.uint32) if what == "float" else a,
                              b.view(np.uint32) if what == "float" else b), f"{label}: {what} differs with culling off"
    return o


@pytest.mark.parametrize("case_index", range(len(ARRAY_CASES)), ids=[c[0] for c in ARRAY_CASES])
def test_texel_edges(pkg, gpu, oracle, textures, case_index):
    name, arr, sizes, max_size = ARRAY_CASES[case_index]
    gpu.set_texture_array(arr)
    otex = oracle.TextureSet(textures[0], arr)
    cam = camera(pkg)
    shown = 0
    for obj_index, obj in enumerate(OBJECTS):
        texture_index, flags = combo_of(case_index, obj_index)
        scene = textured_scene(pkg, obj, sizes, max_size, texture_index, flags)
        for filter_mode in (0, 1):
            label = f"{name} {obj} texture_index {texture_index} flags {flags} filter {filter_mode}"
            o = check_frame(gpu, oracle, otex, scene, cam, params_of(pkg, filter_mode), label)
            shown += int((o[2] < 400).sum())
    assert shown > 0


@pytest.mark.parametrize("texture_index", TEXTURE_INDICES)
@pytest.mark.parametrize("flags", UV_FLAGS, ids=lambda f: "swap%d_invx%d_invy%d" % f)
def test_texture_index_and_uv_flags(pkg, gpu, oracle, textures, texture_index, flags):
    """Every (texture_index, uv flags) pair on the islands array at 13x9 (an
    odd stride, islands cut by the wrap), rectangle and sphere, LERP."""
    arr = texture_array("islands", 13, 9)
    gpu.set_texture_array(arr)
    otex = oracle.TextureSet(textures[0], arr)
    for obj in NON_VACUOUS:
        scene = textured_scene(pkg, obj, [(13, 9)], (13, 9), texture_index, flags)
        check_frame(gpu, oracle, otex, scene, camera(pkg), params_of(pkg, 0),
                    f"islands-13x9 {obj} texture_index {texture_index} flags {flags}")


@pytest.mark.parametrize("cell", non_vacuous_cells(), ids=lambda c: f"{c[0]}-{c[1][0]}x{c[1][1]}-{c[2]}")
def test_rays_stop_and_pass(pkg, oracle, textures, cell):
    """The frames above are not vacuous (oracle frames alone; the same
    condition runs without a GPU in tests/test_scene_extremes_cases.py)."""
    pattern, size, obj = cell
    stop, went = stop_pass_shares(pkg, oracle, textures[0], pattern, size, obj, 0, (0, 0, 0))
    assert stop >= 0.02 and went >= 0.02, (cell, stop, went)


@pytest.mark.parametrize("size", [(1, 1), (2, 1), (3, 5), (257, 129)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("channels", [3, 4])
def test_small_skyboxes(pkg, gpu, oracle, textures, size, channels):
    """The skybox sampler at sizes where every lookup wraps (1x1, 2x1), an
    odd 3x5 and 257x129, 3 and 4 channels, both filters: the hole alone."""
    w, h = size
    bg = np.random.default_rng(7 * w + h).integers(0, 256, size=(h, w, channels), dtype=np.uint8)
    gpu.set_background(bg)
    arr = texture_array("seam", 7, 5)
    gpu.set_texture_array(arr)
    otex = oracle.TextureSet(bg, arr)
    scene = pkg.scenes.scene_black_hole_only()
    try:
        for filter_mode in (0, 1):
            check_frame(gpu, oracle, otex, scene, camera(pkg), params_of(pkg, filter_mode),
                        f"skybox {w}x{h}x{channels} filter {filter_mode}")
    finally:
        gpu.set_background(textures[0])


def test_zz_diag_counters_zero(gpu):
    """After every frame of this module on the shared context: no pixel
    stopped at an opaque-classified hit whose shaded alpha was not 1, and no
    stream-ordered free failed."""
    assert gpu.diag_counters() == {"hit_not_opaque": 0, "free_errors": 0}
