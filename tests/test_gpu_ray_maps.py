"""sr_ray_maps on the GPU (sr.h "Ray maps"): the lens map and the G-buffer of
the first surface from the retained rays, held to the unchanged CPU oracle.

The oracle has no such output. tests/ray_map_cases.py restates its own
arithmetic on top of the maps (get_bg's (u, v); calculate_lighting's light
loop), and tests/test_ray_map_cases.py shows on the oracle alone that both
statements reproduce its frames bit for bit and notice one ulp of every input.
Here the statements are fed the GPU's maps and must give the oracle's float
FragColor. No tolerance anywhere: floats are compared as bits, a NaN matches
a NaN.
"""
import ctypes as C

import numpy as np
import pytest

import extreme_cases as X
import pick_cases as PK
import projection_cases as PJ
import ray_map_cases as R
import shading_cases as S
from test_gpu_launch_matrix import World, host, reset
from test_gpu_parity import stacked_layers_scene

pytestmark = pytest.mark.gpu

F = np.float32
W, H, STEPS = R.W, R.H, 400
SKY, NONE = PK.SKY, PK.NONE
MAPS = ("end", "id", "sky_dir", "sky_uv", "hit_point", "hit_normal", "hit_view", "hit_base", "hit_step")
HIT_FLOATS = ("hit_point", "hit_normal", "hit_view", "hit_base")
QNAN = np.uint32(R.QNAN_BITS)
SENT_I, SENT_F = -77, F(-1234.5)
BR, LIST = 4, [2, -1, 0]
# cameras at the feature scene's objects: (position, target)
LOOKS = {"sphere": ((-6.0, 3.0, 7.0), (-6.0, 1.0, 0.0)), "cylinder": ((3.0, 8.0, 7.0), (0.0, 6.0, 0.0)),
         "box": ((11.0, 3.0, 3.0), (7.0, 0.0, -2.0)), "box-behind": ((9.0, -3.0, -8.0), (7.0, 0.0, -2.0)),
         "planes": ((2.0, 1.0, 9.0), (0.0, -3.0, -6.0)), "disks": ((1.0, 4.0, 9.0), (0.0, 0.0, -2.0)),
         "rectangle": ((4.5, 1.0, 13.0), (4.5, 0.0, 8.0))}
# a translucent rectangle in front of shading_cases.BACK that reaches beyond BACK's edge, seen by a wide camera:
# some of what shows through it is the sky
FRONT_WIDE = {**S.RECT, "pos": (-1.0, 1.0, 6.0), "width": 6.0, "height": 2.0}
FRONT_AWAY_WIDE = {**S.RECT_AWAY, "pos": (-1.0, -1.0, 6.0), "width": 6.0, "height": 2.0}


class Cells:
    """Scenes, cameras, skies and the oracle's frames, made once."""

    def __init__(self, pkg, oracle, textures):
        self.pkg, self.oracle = pkg, oracle
        self.wd = World(pkg, oracle, textures)
        sc, abi = pkg.scenes, pkg.abi
        self.arr = textures[1]
        layers = sc.feature_texture_array()[0]
        colours = layers[0, :150, :200].copy()
        colours[..., 3] = 255  # opaque texels: LERP filtering of four 1.0 alphas is exactly 1.0
        self.farr = sc.pad_texture_array([colours, layers[1, :, :, :3]])[0]
        self.sky = R.random_sky()
        # the 1 x 1 black and white skies of check_end, RGBA with alphas 255 and 0: a pixel whose colour is NaN
        # under both (a translucent surface's NaN colour plus anything) still shows in its alpha whether a
        # get_bg term was added
        self.skies = {"random": self.sky, "black": np.array([[[0, 0, 0, 255]]], dtype=np.uint8),
                      "white": np.array([[[255, 255, 255, 0]]], dtype=np.uint8)}
        self._tex, self._ref, self._scenes = {}, {}, {}
        self.cams = dict(self.wd.cams)
        self.cams["rect"] = sc.camera_look((0.0, 0.0, 12.0), (0.0, 0.0, -12.0), fov=90.0)  # shading_cases.CAM, wider
        for name, (pos, target) in LOOKS.items():  # at the feature scene's objects
            self.cams[name] = sc.camera_look(pos, tuple(t - p for p, t in zip(pos, target)), fov=70.0)
        makers = {
            "empty": sc.scene_black_hole_only,
            "none": lambda: X.empty_scene(pkg),
            "small": lambda: self.wd.scene("small"),
            "large": lambda: self.wd.scene("large"),
            "stacked": lambda: self.wd.scene("stacked"),
            "stacked-through": lambda: self._through(stacked_layers_scene(sc, abi)),
            "default-rig": lambda: R.rigged(pkg, sc.scene_default(True)),
            "large-rig": lambda: R.rigged(pkg, sc.scene_stress()),
            "features": self._textured,
            "front": lambda: self._two(FRONT_WIDE, alpha=0.25),
            "front-opaque": lambda: self._two(FRONT_WIDE),
            "front-alone": lambda: self._two(FRONT_WIDE, alpha=0.25, back=False),
            "behind": lambda: self._two(FRONT_AWAY_WIDE, double_sided=0),
        }
        self._makers = makers

    def _textured(self):
        """scenes.scene_features with a texture and a normal map on every material (its uv flags kept, the rest
        given some), every base colour opaque."""
        s = self.pkg.scenes.scene_features()
        for k, m in enumerate(s.materials):
            m.texture_index, m.normal_map_index = 0, 1
            m.color[3] = 1.0
        s.materials[2].invert_uv_x = s.materials[3].swap_uvs = 1
        s.materials[5].invert_uv_y = s.materials[5].swap_uvs = 1
        return s

    @staticmethod
    def _through(s):
        s.materials[1].color[3] = 0.5  # the layer behind translucent too: every ray goes on to the sky or the hole
        return s

    def _two(self, front, alpha=1.0, double_sided=1, back=True):
        s = X.empty_scene(self.pkg)
        X.plain_material(s.materials[1], (0.3, 0.8, 0.5, alpha))
        s.materials[1].double_sided_normals = double_sided
        X.plain_material(s.materials[2], S.BACK_COLOR)
        X.append_primitive(s, front, 1)
        if back:
            X.append_primitive(s, S.BACK, 2)
        return R.rig(self.pkg, s, (0.0, 0.0, 7.0))

    def scene(self, key):
        if key not in self._scenes:
            self._scenes[key] = self._makers[key]()
        return self._scenes[key]

    def tex(self, sky, features=False):
        k = (sky, features)
        if k not in self._tex:
            self._tex[k] = self.oracle.TextureSet(self.skies[sky], self.farr if features else self.arr)
        return self._tex[k]

    def params(self, steps=STEPS, **kw):
        p = self.wd.params(steps)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def ref(self, key, sky="random", cam="view", w=W, h=H, steps=STEPS, projection=None, fov=None, **prm):
        """The oracle's (float FragColor, steps) of a cell, read-only."""
        k = (key, sky, cam, w, h, steps, projection, fov, tuple(sorted(prm.items())))
        if k not in self._ref:
            tex = self.tex(sky, key == "features")
            p = self.params(steps, **prm)
            if projection is None:
                _, f, s = self.oracle.render(self.scene(key), self.cams[cam], p, w, h, tex)
            else:
                _, f, s = PJ.pixel_frame(self.pkg, self.oracle, self.scene(key), PJ.with_fov(self.pkg, self.cams[cam], fov),
                                         p, w, h, projection, tex)
            f.setflags(write=False)
            s.setflags(write=False)
            self._ref[k] = (f, s)
        return self._ref[k]


@pytest.fixture(scope="module")
def cells(pkg, oracle, textures):
    return Cells(pkg, oracle, textures)


@pytest.fixture(scope="module")
def gpu(pkg, cells):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    r = pkg.Renderer(0)
    r.set_background(cells.sky)
    r.set_texture_array(cells.arr)
    yield r
    r.close()


def use(gpu, cells, key):
    gpu.set_texture_array(cells.farr if key == "features" else cells.arr)
    gpu.set_scene(cells.scene(key))
    gpu.set_test_ray(cells.wd.test_rays[False])


def maps_of(gpu, which=MAPS):
    m = gpu.ray_maps(which)
    (pick,) = host(gpu.pick_map())
    out = dict(zip(m, host(*m.values())))
    for k in ("end", "id", "hit_step"):
        if k in out:
            out[k] = out[k][..., 0]
    out["pick"] = pick
    return out


def launch(gpu, cells, key, cam="view", w=W, h=H, steps=STEPS, **prm):
    use(gpu, cells, key)
    gpu.render(cells.cams[cam], cells.params(steps, **prm), w, h)
    return maps_of(gpu)


def is_qnan(a):
    return (R.bits(a) == QNAN).all(-1)


def check_ids_and_fill(m, label):
    """id is sr_pick_map's; the maps hold the quiet NaN and -1 where they are not valid."""
    assert np.array_equal(m["id"], m["pick"]), f"{label}: id differs from sr_pick_map on {int((m['id'] != m['pick']).sum())}"
    inv = m["id"] < 0
    for k in HIT_FLOATS:
        assert is_qnan(m[k][inv]).all(), (label, k)
    assert (m["hit_step"][inv] == -1).all() and (m["hit_step"][~inv] >= 0).all(), label
    nosky = m["end"] != R.END_SKY
    assert is_qnan(m["sky_dir"][nosky]).all() and is_qnan(m["sky_uv"][nosky]).all(), label
    assert set(np.unique(m["end"])) <= {R.END_NONE, R.END_SKY, R.END_OPAQUE}, label
    assert ((m["end"] == R.END_NONE) == (m["id"] == NONE)).all(), label
    assert (m["end"][m["id"] == SKY] == R.END_SKY).all(), label


def check_end(m, black, white, label):
    """SKY exactly where the oracle's frames under the black and the white sky differ (rgb or alpha, as bits),
    NONE where there is no ray, OPAQUE elsewhere."""
    sky = ~R.same_bits(black, white).all(-1)
    none = m["id"] == NONE
    want = np.where(none, R.END_NONE, np.where(sky, R.END_SKY, R.END_OPAQUE))
    bad = m["end"] != want
    assert not bad.any(), f"{label}: end differs on {int(bad.sum())} of {bad.size} pixels, first {np.argwhere(bad)[:4].tolist()}"
    return int(sky.sum())


def check_sky(oracle, cells, m, f, mode, label, min_share=R.MIN_SKY_SHARE):
    """The lens map: the oracle's sampler at sky_uv is its FragColor on pure-sky pixels; sky_uv is sky_uv_np(sky_dir)."""
    k = m["end"] == R.END_SKY
    uv = m["sky_uv"][k]
    assert R.same_bits(uv, R.sky_uv_np(m["sky_dir"][k])).all(), label
    pure = m["id"] == SKY
    got = np.stack([oracle.sample_texture(cells.sky, u, v, mode) for u, v in m["sky_uv"][pure]]) if pure.any() else f[pure]
    ok = R.same_bits(got, f[pure]).all(-1)
    assert ok.all(), f"{label}: {int((~ok).sum())} of {int(pure.sum())} pure-sky pixels differ from the oracle's FragColor"
    assert pure.sum() >= min_share * pure.size, (label, int(pure.sum()))


def check_gbuffer(scene, m, f, s, label, min_share=R.MIN_HIT_SHARE):
    """Deferred shading of the maps is the oracle's FragColor where the first surface is opaque; hit_step its steps."""
    k = (m["id"] >= 0) & (m["hit_base"][..., 3] == 1.0)
    rgb = R.deferred_frame(scene, np.where(k, m["id"], -1), m["hit_point"], m["hit_normal"], m["hit_view"], m["hit_base"])
    ok = R.same_bits(rgb[k], f[k][:, :3]).all(-1) & (f[k][:, 3] == 1.0)
    assert ok.all(), f"{label}: {int((~ok).sum())} of {int(k.sum())} opaque-first-hit pixels differ from the oracle's FragColor"
    assert np.array_equal(m["hit_step"][k], s[k]), f"{label}: hit_step differs on {int((m['hit_step'][k] != s[k]).sum())}"
    assert k.sum() >= min_share * k.size, (label, int(k.sum()))
    return k


# ---- the lens map and `end` against the oracle -------------------------------------
@pytest.mark.parametrize("mode", [0, 1], ids=["lerp", "weighted"])
@pytest.mark.parametrize("key", ["empty", "small", "large"])
def test_sky_and_end_against_the_oracle(pkg, oracle, gpu, cells, key, mode):
    try:
        m = launch(gpu, cells, key, filter_mode=mode)
        label = f"{key} filter {mode}"
        check_ids_and_fill(m, label)
        f, _ = cells.ref(key, "random", filter_mode=mode)
        # two of the stress scene's planes fill most of the view: its sky shows through translucent objects only
        share = 20 / (W * H) if key == "large" else R.MIN_SKY_SHARE
        check_sky(oracle, cells, m, f, mode, label, min_share=0.0 if key == "large" else share)
        n = check_end(m, cells.ref(key, "black", filter_mode=mode)[0], cells.ref(key, "white", filter_mode=mode)[0], label)
        assert n >= share * W * H
        assert gpu.diag_counters() == {"hit_not_opaque": 0, "free_errors": 0}
    finally:
        reset(gpu, cells.wd)


@pytest.mark.parametrize("steps", [7, 0])
@pytest.mark.parametrize("key", ["small", "large"])
def test_short_schedules(pkg, oracle, gpu, cells, key, steps):
    """7 steps: most rays end by frag:935 in mid-flight; 0 steps: all of them at once."""
    try:
        m = launch(gpu, cells, key, steps=steps)
        label = f"{key} {steps} steps"
        check_ids_and_fill(m, label)
        f, s = cells.ref(key, "random", steps=steps)
        check_sky(oracle, cells, m, f, 0, label, min_share=0.0 if key == "large" else 0.02)
        check_end(m, cells.ref(key, "black", steps=steps)[0], cells.ref(key, "white", steps=steps)[0], label)
        check_gbuffer(cells.scene(key), m, f, s, label, min_share=0.0)
    finally:
        reset(gpu, cells.wd)


def test_end_none_under_a_noise_mask(pkg, oracle, gpu, cells):
    try:
        m = launch(gpu, cells, "small", percent_black=0.4)
        check_ids_and_fill(m, "noise")
        share = (m["end"] == R.END_NONE).mean()
        assert 0.2 < share < 0.6, share
        check_end(m, cells.ref("small", "black", percent_black=0.4)[0], cells.ref("small", "white", percent_black=0.4)[0],
                  "noise")
    finally:
        reset(gpu, cells.wd)


def test_end_none_beyond_the_fisheye(pkg, oracle, gpu, cells):
    _, proj, w, h, fov = PJ.BY_ID["fisheye-48x48-fov360"]
    try:
        gpu.set_projection(proj)
        use(gpu, cells, "small")
        gpu.render(PJ.with_fov(pkg, cells.cams["view"], fov), cells.params(), w, h)
        m = maps_of(gpu)
        check_ids_and_fill(m, "fisheye")
        assert (m["end"][0, 0], m["end"][h // 2, w // 2]) != (R.END_NONE, R.END_NONE) and m["end"][0, 0] == R.END_NONE
        kw = {"w": w, "h": h, "projection": proj, "fov": fov}
        check_end(m, cells.ref("small", "black", **kw)[0], cells.ref("small", "white", **kw)[0], "fisheye")
    finally:
        gpu.set_projection(pkg.abi.PROJECTION_RECTILINEAR)
        reset(gpu, cells.wd)


@pytest.mark.parametrize("mode", ["flat", "half-width", "half-height"])
def test_flat_and_split_modes(pkg, oracle, gpu, cells, mode):
    prm = {"flat": {"raytrace_type": 1}, "half-width": {"raytrace_type": 2, "curved_percentage": 0.5},
           "half-height": {"raytrace_type": 3, "curved_percentage": 0.4}}[mode]
    try:
        m = launch(gpu, cells, "default-rig", **prm)
        check_ids_and_fill(m, mode)
        f, s = cells.ref("default-rig", "random", **prm)
        check_sky(oracle, cells, m, f, 0, mode)
        check_end(m, cells.ref("default-rig", "black", **prm)[0], cells.ref("default-rig", "white", **prm)[0], mode)
        k = check_gbuffer(cells.scene("default-rig"), m, f, s, mode)
        flat = PJ.flat_mask(cells.params(**prm), W, H)
        assert (m["hit_step"][k & flat] == 0).all()
        # the flat half: the sky direction is the camera ray itself
        _, d = pkg.abi.camera_rays(cells.cams["view"], "rectilinear", W, H)
        sel = flat & (m["end"] == R.END_SKY)
        assert sel.sum() >= R.MIN_SKY_SHARE * W * H
        assert R.same_bits(m["sky_dir"][sel], R.norm3(d)[sel]).all()
    finally:
        reset(gpu, cells.wd)


@pytest.mark.parametrize("key,cam,resumed", [("stacked-through", "view", True), ("front", "rect", False),
                                             ("front-alone", "rect", False)])
def test_the_lens_map_through_translucency(pkg, oracle, gpu, cells, key, cam, resumed):
    """A ray seen through translucent surfaces ends where the same ray of the empty scene ends."""
    try:
        empty = launch(gpu, cells, "empty" if resumed else "none", cam)
        m = launch(gpu, cells, key, cam)
        check_ids_and_fill(m, key)
        sky = m["end"] == R.END_SKY
        assert sky.sum() >= R.MIN_SKY_SHARE * W * H, int(sky.sum())
        assert (empty["end"][sky] == R.END_SKY).all()
        for k in ("sky_dir", "sky_uv"):
            assert R.same_bits(m[k][sky], empty[k][sky]).all(), (key, k)
        through = sky & (m["id"] >= 0)  # sky pixels seen through a surface
        # (in front of the rectangle behind it only the part that reaches beyond its edge shows the sky)
        assert through.sum() >= (R.MIN_SKY_SHARE * W * H if key != "front" else 20), int(through.sum())
        if resumed:  # every ray's log filled: the end of each comes from the resume path
            assert (m["id"] == 0).all() and (m["hit_base"][..., 3] == F(0.3)).all()
        check_end(m, cells.ref(key, "black", cam)[0], cells.ref(key, "white", cam)[0], key)
    finally:
        reset(gpu, cells.wd)


def test_stacked_layers_end_at_the_opaque_one(pkg, oracle, gpu, cells):
    try:
        m = launch(gpu, cells, "stacked")
        check_ids_and_fill(m, "stacked")
        assert (m["end"] == R.END_OPAQUE).mean() >= 0.95 and (m["id"] == 0).all()
        check_end(m, cells.ref("stacked", "black")[0], cells.ref("stacked", "white")[0], "stacked")
    finally:
        reset(gpu, cells.wd)


# ---- the G-buffer against the oracle ------------------------------------------------
@pytest.mark.parametrize("flat", [False, True], ids=["curved", "flat"])
@pytest.mark.parametrize("key", ["default-rig", "large-rig"])
def test_gbuffer_against_the_oracle(pkg, oracle, gpu, cells, key, flat):
    prm = {"raytrace_type": 1} if flat else {}
    cam = "view"
    try:
        m = launch(gpu, cells, key, cam, **prm)
        label = f"{key} {'flat' if flat else 'curved'}"
        check_ids_and_fill(m, label)
        f, s = cells.ref(key, "random", cam, **prm)
        k = check_gbuffer(cells.scene(key), m, f, s, label)
        check_sky(oracle, cells, m, f, 0, label, min_share=0.0)
        if flat:
            assert (m["hit_step"][m["id"] >= 0] == 0).all()
        seen = set(int(v) for v in np.unique(m["id"][k]))
        print(f"MEASURED {label}: {int(k.sum())} opaque first hits of objects {sorted(seen)}")
        assert len(seen) >= 2, seen
        assert gpu.diag_counters() == {"hit_not_opaque": 0, "free_errors": 0}
    finally:
        reset(gpu, cells.wd)
        gpu.set_texture_array(cells.arr)


def test_gbuffer_of_textured_and_normal_mapped_primitives(pkg, oracle, gpu, cells):
    """The feature scene from cameras that look at each of its textured objects: the box's faces, the uv flags,
    the planes' texture windows and the normal maps, curved and flat."""
    seen = set()
    try:
        for name in LOOKS:
            for prm in ({}, {"raytrace_type": 1}):
                m = launch(gpu, cells, "features", name, 33, 17, **prm)
                label = f"features {name} {prm}"
                check_ids_and_fill(m, label)
                f, s = cells.ref("features", "random", name, 33, 17, **prm)
                k = check_gbuffer(cells.scene("features"), m, f, s, label, min_share=0.0)
                seen |= set(int(v) for v in np.unique(m["id"][k]))
        print(f"MEASURED features: opaque first hits of objects {sorted(seen)}")
        assert seen >= set(range(8)), seen  # every object: the planes, sphere, disks, cylinder, rectangle and box
    finally:
        reset(gpu, cells.wd)
        gpu.set_texture_array(cells.arr)


def test_gbuffer_under_the_fisheye(pkg, oracle, gpu, cells):
    _, proj, w, h, fov = PJ.BY_ID["fisheye-33x17-own"]
    try:
        gpu.set_projection(proj)
        use(gpu, cells, "default-rig")
        gpu.render(cells.cams["view"], cells.params(), w, h)
        m = maps_of(gpu)
        check_ids_and_fill(m, "fisheye")
        f, s = cells.ref("default-rig", "random", w=w, h=h, projection=proj, fov=fov)
        check_gbuffer(cells.scene("default-rig"), m, f, s, "fisheye")
        check_sky(oracle, cells, m, f, 0, "fisheye")
    finally:
        gpu.set_projection(pkg.abi.PROJECTION_RECTILINEAR)
        reset(gpu, cells.wd)


def test_gbuffer_of_a_row_band(pkg, oracle, gpu, cells):
    try:
        use(gpu, cells, "default-rig")
        gpu.render(cells.cams["view"], cells.params(), W, H, 7, 25)
        m = maps_of(gpu)
        assert m["id"].shape == (18, W) and m["hit_base"].shape == (18, W, 4)
        check_ids_and_fill(m, "band")
        f, s = cells.ref("default-rig", "random")
        check_gbuffer(cells.scene("default-rig"), m, f[7:25], s[7:25], "band")
        check_sky(oracle, cells, m, f[7:25], 0, "band", min_share=0.0)
    finally:
        reset(gpu, cells.wd)


def rows_of(frame, blocks, br, h):
    """The rows a block list packs (None for the rows left unwritten)."""
    out = []
    for b in blocks:
        for j in range(br):
            y = b * br + j
            out.append(y if b >= 0 and y < h else None)
    return out


def padded_maps(gpu, abi, frames, rows, w, pad=5, extra=11):
    """sr_ray_maps with pitch w + pad and stride pitch * rows + extra pixels into sentinel-filled buffers ->
    {map: [frames, rows, w, n]}; everything else must still hold the sentinel."""
    import torch

    pitch, stride = w + pad, (w + pad) * rows + extra
    bufs, ptrs = {}, abi.RayMapPtrs()
    for key, (n, dtype) in abi.RAY_MAPS.items():
        fill = SENT_I if dtype == "int32" else float(SENT_F)
        bufs[key] = torch.full((frames * stride + 3, n), fill, dtype=getattr(torch, dtype), device="cuda")
        setattr(ptrs, key, bufs[key].data_ptr())
    assert gpu.lib.sr_ray_maps(gpu.ctx, C.byref(ptrs), pitch, stride, gpu._stream(None)) == 0
    out = {}
    for key, a in zip(bufs, host(*bufs.values())):
        sent = SENT_I if a.dtype == np.int32 else SENT_F
        assert (a[frames * stride:] == sent).all(), key
        a = a[:frames * stride].reshape(frames, stride, -1)
        assert (a[:, pitch * rows:] == sent).all(), key + ": wrote between the frames"
        a = a[:, :pitch * rows].reshape(frames, rows, pitch, -1)
        assert (a[:, :, w:] == sent).all(), key + ": wrote into the pitch padding"
        out[key] = np.ascontiguousarray(a[:, :, :w])
    return out


@pytest.mark.parametrize("kind", ["batch", "list"])
def test_gbuffer_of_batches_and_padded_block_lists(pkg, oracle, gpu, cells, kind):
    names = cells.wd.batch
    cams = [cells.cams[c] for c in names]
    scene = cells.scene("default-rig")
    try:
        use(gpu, cells, "default-rig")
        if kind == "batch":
            gpu.render_blocks_batch(cams, cells.params(), W, H, 8, 1, 2)
            blocks, br = list(range(1, (H + 7) // 8, 2)), 8
        else:
            gpu.render_block_list(cams, cells.params(), W, H, BR, LIST)
            blocks, br = LIST, BR
        ys = rows_of(None, blocks, br, H)
        dense = maps_of(gpu)
        got = padded_maps(gpu, pkg.abi, len(cams), len(ys), W)
        written = np.array([y is not None for y in ys])
        take = np.array([y if y is not None else 0 for y in ys])
        for fi, name in enumerate(names):
            m = {k: (v[fi, ..., 0] if k in ("end", "id", "hit_step") else v[fi]) for k, v in got.items()}
            for k, v in m.items():  # the padded call and the dense one agree; unwritten rows keep the sentinel
                sent = SENT_I if v.dtype == np.int32 else SENT_F
                assert (v[~written] == sent).all(), (kind, name, k)
                assert R.same_bits(v[written], dense[k][fi][written]).all() if v.dtype != np.int32 else \
                    np.array_equal(v[written], dense[k][fi][written]), (kind, name, k)
            m = {k: v[written] for k, v in m.items()}
            m["pick"] = dense["pick"][fi][written]
            check_ids_and_fill(m, f"{kind} {name}")
            f, s = cells.ref("default-rig", "random", name)
            check_gbuffer(scene, m, f[take[written]], s[take[written]], f"{kind} {name}", min_share=0.0)
            check_sky(oracle, cells, m, f[take[written]], 0, f"{kind} {name}", min_share=0.0)
    finally:
        reset(gpu, cells.wd)


@pytest.mark.parametrize("size", [(33, 17), (1, 1)])
def test_small_frames(pkg, oracle, gpu, cells, size):
    w, h = size
    try:
        m = launch(gpu, cells, "default-rig", "view", w, h)
        check_ids_and_fill(m, str(size))
        f, s = cells.ref("default-rig", "random", "view", w, h)
        check_gbuffer(cells.scene("default-rig"), m, f, s, str(size), min_share=0.0)
        check_sky(oracle, cells, m, f, 0, str(size), min_share=0.0)
    finally:
        reset(gpu, cells.wd)


# ---- the first surface ----------------------------------------------------------------
@pytest.mark.parametrize("flat", [False, True], ids=["curved", "flat"])
def test_translucent_first_surface(pkg, oracle, gpu, cells, flat):
    prm = {"raytrace_type": 1} if flat else {}
    try:
        opaque = launch(gpu, cells, "front-opaque", "rect", **prm)
        m = launch(gpu, cells, "front", "rect", **prm)
        check_ids_and_fill(m, "front")
        assert np.array_equal(m["id"], opaque["id"])
        front = m["id"] == 0
        assert front.sum() >= R.MIN_HIT_SHARE * W * H
        for k in ("hit_point", "hit_normal", "hit_view"):
            assert R.same_bits(m[k], opaque[k]).all(), k
        assert np.array_equal(m["hit_step"], opaque["hit_step"])
        assert (m["hit_base"][front][:, 3] == F(0.25)).all() and (opaque["hit_base"][front][:, 3] == 1.0).all()
        assert R.same_bits(m["hit_base"][..., :3], opaque["hit_base"][..., :3]).all()
        # what shows through: the rectangle behind or the sky beyond its edge (a flat ray does not look behind:
        # the sky); the opaque twin's G-buffer is the oracle's frame
        check_end(m, cells.ref("front", "black", "rect", **prm)[0], cells.ref("front", "white", "rect", **prm)[0], "front")
        assert (opaque["end"][front] == R.END_OPAQUE).all()
        assert ((m["end"][front] == R.END_SKY).all() if flat else (m["end"][front] == R.END_OPAQUE).any())
        f, s = cells.ref("front-opaque", "random", "rect", **prm)
        check_gbuffer(cells.scene("front-opaque"), opaque, f, s, "front-opaque")
        f, s = cells.ref("front", "random", "rect", **prm)
        check_gbuffer(cells.scene("front"), m, f, s, "front")
    finally:
        reset(gpu, cells.wd)


@pytest.mark.parametrize("flat", [False, True], ids=["curved", "flat"])
def test_single_sided_surface_seen_from_behind(pkg, oracle, gpu, cells, flat):
    prm = {"raytrace_type": 1} if flat else {}
    try:
        m = launch(gpu, cells, "behind", "rect", **prm)
        check_ids_and_fill(m, "behind")
        assert not (m["id"] == 0).any()
        f, s = cells.ref("behind", "random", "rect", **prm)
        k = check_gbuffer(cells.scene("behind"), m, f, s, "behind", min_share=0.0)
        if flat:  # the shader does not look behind a flat ray's closest hit: the background
            assert (m["id"] == 1).sum() > 0 and (m["id"] == SKY).sum() >= R.MIN_SKY_SHARE * W * H
        else:     # the step loop goes on to the rectangle behind
            assert (m["id"][k] == 1).all() and k.sum() >= R.MIN_HIT_SHARE * W * H
            assert (np.abs(m["hit_point"][k][:, 2] - S.BACK["pos"][2]) < 1e-3).all()
        check_end(m, cells.ref("behind", "black", "rect", **prm)[0], cells.ref("behind", "white", "rect", **prm)[0], "behind")
    finally:
        reset(gpu, cells.wd)


# ---- state ----------------------------------------------------------------------------
def test_the_retained_frame_survives(pkg, gpu, cells):
    try:
        use(gpu, cells, "stacked-through")  # every pixel walked on by the resume path
        gpu.render(cells.cams["view"], cells.params(), W, H)
        (before,) = host(gpu.reshade())
        state = gpu.pixel_state().copy()
        a = maps_of(gpu)
        assert gpu.can_reshade()
        b = maps_of(gpu)
        (after,) = host(gpu.reshade())
        assert np.array_equal(before, after) and gpu.can_reshade()
        assert np.array_equal(gpu.pixel_state().view(np.uint32), state.view(np.uint32)), "the pixel state was written"
        for k in MAPS:
            assert R.same_bits(a[k], b[k]).all() if a[k].dtype != np.int32 else np.array_equal(a[k], b[k]), k
        assert gpu.diag_counters() == {"hit_not_opaque": 0, "free_errors": 0}
    finally:
        reset(gpu, cells.wd)


def test_maps_follow_a_shading_only_scene_change(pkg, gpu, cells):
    sc, abi = pkg.scenes, pkg.abi
    old = cells.scene("features")
    new = sc.struct_from_bytes(abi.Scene, sc.struct_bytes(old))
    for m in new.materials:
        m.color[0], m.color[1], m.color[2] = m.color[2], 0.75, m.color[0]
        m.normal_map_index = 1 if m.normal_map_index < 0 else -1
    assert abi.scene_shading_only(old, new)
    cams = cells.cams
    try:
        first = launch(gpu, cells, "features", "sphere")
        gpu.set_scene(new)
        assert gpu.can_reshade()
        got = maps_of(gpu)
        gpu.render(cams["sphere"], cells.params(), W, H)  # the new scene's own launch
        want = maps_of(gpu)
        for k in MAPS:
            same = R.same_bits(got[k], want[k]).all() if got[k].dtype != np.int32 else np.array_equal(got[k], want[k])
            assert same, k
        for k in ("end", "id", "sky_dir", "sky_uv", "hit_point", "hit_view", "hit_step"):
            same = R.same_bits(got[k], first[k]).all() if got[k].dtype != np.int32 else np.array_equal(got[k], first[k])
            assert same, k
        valid = first["id"] >= 0
        assert not R.same_bits(got["hit_base"][valid], first["hit_base"][valid]).all()
        assert not R.same_bits(got["hit_normal"][valid], first["hit_normal"][valid]).all()
    finally:
        reset(gpu, cells.wd)
        gpu.set_texture_array(cells.arr)


def test_subsets_streams_and_renders_in_between(pkg, gpu, cells):
    import torch

    abi = pkg.abi
    try:
        full = launch(gpu, cells, "large")
        for which in (("end", "sky_uv"), ("id",), ("hit_base",), ("hit_step", "hit_normal"), ("sky_dir",), ("hit_point", "end")):
            got = padded_maps_subset(gpu, abi, which, W, H)
            for k in MAPS:
                if k in which:
                    v = got[k][..., 0] if k in ("end", "id", "hit_step") else got[k]
                    assert R.same_bits(v, full[k]).all() if v.dtype != np.int32 else np.array_equal(v, full[k]), (which, k)
                else:
                    assert k not in got
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        a = gpu.ray_maps(MAPS, stream=s1)
        b = gpu.ray_maps(MAPS, stream=s2)
        gpu.render(cells.cams["fly1"], cells.params(), W, H, stream=s1)
        c = gpu.ray_maps(MAPS, stream=s2)
        gpu.render(cells.cams["view"], cells.params(), W, H)
        d = gpu.ray_maps(MAPS)
        torch.cuda.synchronize()
        other = launch(gpu, cells, "large", "fly1")
        for k in MAPS:
            x, y, z, v = (t.cpu().numpy() for t in (a[k], b[k], c[k], d[k]))
            if k in ("end", "id", "hit_step"):
                x, y, z, v = x[..., 0], y[..., 0], z[..., 0], v[..., 0]
            eq = (lambda p, q: np.array_equal(p, q)) if x.dtype == np.int32 else (lambda p, q: R.same_bits(p, q).all())
            assert eq(x, full[k]) and eq(y, full[k]) and eq(v, full[k]) and eq(z, other[k]), k
    finally:
        reset(gpu, cells.wd)


def padded_maps_subset(gpu, abi, which, w, rows):
    """The maps of `which` alone into sentinel-framed buffers (one sentinel element before and after)."""
    import torch

    bufs, ptrs = {}, abi.RayMapPtrs()
    for key in which:
        n, dtype = abi.RAY_MAPS[key]
        fill = SENT_I if dtype == "int32" else float(SENT_F)
        bufs[key] = torch.full((rows * w + 2, n), fill, dtype=getattr(torch, dtype), device="cuda")
        setattr(ptrs, key, bufs[key][1:].data_ptr())
    assert gpu.lib.sr_ray_maps(gpu.ctx, C.byref(ptrs), w, 0, gpu._stream(None)) == 0
    out = {}
    for key, a in zip(bufs, host(*bufs.values())):
        sent = SENT_I if a.dtype == np.int32 else SENT_F
        assert (a[0] == sent).all() and (a[-1] == sent).all(), key
        out[key] = a[1:-1].reshape(rows, w, -1)
    return out


def test_not_ready_and_rejections(pkg, gpu, cells):
    import torch

    abi, lib = pkg.abi, gpu.lib
    cam, prm, w, h = cells.cams["view"], cells.params(100), 33, 17
    n = len(LIST) * BR
    bufs = {k: torch.full((2 * n * (w + 1) + 8, c), SENT_I if d == "int32" else float(SENT_F), dtype=getattr(torch, d),
                          device="cuda") for k, (c, d) in abi.RAY_MAPS.items()}

    def ptrs(shift=None, only=None):
        p = abi.RayMapPtrs()
        for k, t in bufs.items():
            if only is None or k in only:
                setattr(p, k, t.data_ptr() + (2 if k == shift else 0))
        return p

    def call(p, pitch=w, stride=0, ctx=True):
        return lib.sr_ray_maps(gpu.ctx if ctx else None, C.byref(p) if p is not None else None, pitch, stride, None)

    NR, INV = abi.SR_E_NOT_READY, abi.SR_E_INVALID
    try:
        use(gpu, cells, "small")  # sr_set_test_ray drops whatever was retained
        assert call(ptrs()) == NR
        gpu.render_ss(cam, prm, w, h, 2)
        assert gpu.can_reshade() and call(ptrs()) == NR  # a retained supersampled launch
        gpu.render(cam, prm, w, h)
        gpu.set_texture_array(cells.arr)
        assert call(ptrs()) == NR
        gpu.render(cam, prm, w, h)
        moved = pkg.scenes.struct_from_bytes(abi.Scene, pkg.scenes.struct_bytes(cells.scene("small")))
        moved.spheres[0].radius += 0.5
        gpu.set_scene(moved)
        assert call(ptrs()) == NR  # a geometry change
        gpu.set_scene(cells.scene("small"))
        gpu.render_adaptive(cam, prm, w, h, 2, 8)
        assert call(ptrs()) == NR
        gpu.render(cam, prm, w, h)
        gpu.wave_costs(cam, prm, w, h)
        assert call(ptrs()) == NR
        gpu.render(cam, prm, w, h, 5, 5, out=torch.zeros((1, w, 4), dtype=torch.uint8, device="cuda"))  # zero rows
        assert call(ptrs()) == NR
        gpu.render(cam, prm, w, h)
        assert call(ptrs(), ctx=False) == INV
        assert call(None) == INV
        assert call(abi.RayMapPtrs()) == INV  # all pointers null
        assert call(ptrs(), pitch=w - 1) == INV
        for k in MAPS:
            assert call(ptrs(shift=k)) == INV, k  # a pointer not 4-byte aligned
            assert call(ptrs(shift=k, only=(k,))) == INV, k
        gpu.render_block_list([cam, cam], prm, w, h, BR, LIST)
        assert call(ptrs(), pitch=w + 1, stride=(w + 1) * n - 1) == INV  # a short frame stride
        assert call(ptrs(), pitch=w - 1, stride=w * n) == INV
        torch.cuda.synchronize()
        for k, t in bufs.items():
            a = t.cpu().numpy()
            assert (a == (SENT_I if a.dtype == np.int32 else SENT_F)).all(), f"a refused call wrote {k}"
        assert gpu.can_reshade()
        assert call(ptrs(), pitch=w + 1, stride=(w + 1) * n) == abi.SR_OK
        assert call(ptrs(only=("id",)), pitch=w, stride=w * n) == abi.SR_OK
        torch.cuda.synchronize()
    finally:
        reset(gpu, cells.wd)
