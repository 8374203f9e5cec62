"""sr_trace_ray_maps (sr.h "Ray maps of ray queries") on the GPU: the lens map
and the G-buffer of caller-supplied rays, held to the frame path, to the
unchanged CPU oracle and to sr_trace_rays.

Two references, neither new. A camera's own rays must give sr_ray_maps' maps
of the rendered frame, all nine, every pixel. Scattered rays (origins and
directions of their own, the non-finite ones included) are 1x1 oracle frames
(tests/trace_cases.py), and the maps are what makes the oracle's arithmetic
restated in numpy (tests/ray_map_cases.py) give those frames' FragColor;
tests/test_trace_map_cases.py shows on the oracle alone that the statements
hold for such rays. No tolerance anywhere: floats are compared as bits, a NaN
matches a NaN.
"""
import ctypes as C

import numpy as np
import pytest

import pick_cases as K
import projection_cases as PJ
import ray_map_cases as R
import trace_cases as T
import trace_map_cases as M
from test_gpu_ray_maps import LOOKS, Cells

pytestmark = pytest.mark.gpu

F = np.float32
MAPS = ("end", "id", "sky_dir", "sky_uv", "hit_point", "hit_normal", "hit_view", "hit_base", "hit_step")
INTS = ("end", "id", "hit_step")
HITS = ("hit_point", "hit_normal", "hit_view", "hit_base", "hit_step")
HIT_FLOATS = HITS[:4]
QNAN = np.uint32(R.QNAN_BITS)
SENT = 0x5A
W, H = T.W, T.H


@pytest.fixture(scope="module")
def tm(pkg, oracle, textures):
    return M.TraceMaps(pkg, oracle, textures)


@pytest.fixture(scope="module")
def cells(pkg, oracle, textures):
    return Cells(pkg, oracle, textures)


@pytest.fixture(scope="module")
def gpu(pkg, textures):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    r = pkg.Renderer(0)
    r.set_background(R.random_sky())  # the references' sky: sr_trace_rays beside the maps looks it up
    r.set_texture_array(textures[1])
    yield r
    r.close()


def dev(a):
    import torch

    return torch.from_numpy(np.array(a, dtype=np.float32, order="C")).cuda()  # (a copy: the references are read-only)


def squeeze(m):
    return {k: (v[..., 0] if k in INTS else v) for k, v in m.items()}


def traced(gpu, O, V, params, which=MAPS, stream=None):
    """Renderer.trace_ray_maps of host rays -> {map: host array}, [N] for the int maps and [N, n] for the others."""
    import torch

    got = gpu.trace_ray_maps(dev(O), dev(V), params, which, stream=stream)
    torch.cuda.synchronize()
    assert tuple(got) == tuple(which)
    return squeeze({k: v.cpu().numpy() for k, v in got.items()})


def trace(gpu, O, V, params):
    import torch

    got = gpu.trace_rays(dev(O), dev(V), params, rgba32=True, rgba8=False, steps=True, ids=True)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in got.items()}


def differing(a, b):
    bad = (a != b) if a.dtype == np.int32 else ~R.same_bits(a, b)
    return bad.reshape(len(a), -1).any(-1)


def same_maps(got, want, label, keys=MAPS, sel=None):
    for k in keys:
        a, b = (got[k], want[k]) if sel is None else (got[k][sel], want[k][sel])
        bad = differing(a, b)
        assert not bad.any(), f"{label}: {k} differs on {int(bad.sum())} of {len(bad)} rays, first {np.flatnonzero(bad)[:4].tolist()}"


def setup(gpu, scene, test_ray, cull=True, arr=None):
    gpu.set_culling(cull)
    gpu.set_projection("rectilinear")
    gpu.set_split(0)
    gpu.set_latency_mode(False)
    if arr is not None:
        gpu.set_texture_array(arr)
    gpu.set_scene(scene)
    gpu.set_test_ray(test_ray)


def is_qnan(a):
    return (R.bits(a) == QNAN).all(-1)


def check_fill(m, label):
    """The quiet NaN and -1 exactly where a map is not valid; end is SKY or OPAQUE, id never NONE."""
    inv = m["id"] < 0
    for k in HIT_FLOATS:
        assert is_qnan(m[k][inv]).all(), (label, k)
    assert (m["hit_step"][inv] == -1).all() and (m["hit_step"][~inv] >= 0).all(), label
    nosky = m["end"] != R.END_SKY
    assert is_qnan(m["sky_dir"][nosky]).all() and is_qnan(m["sky_uv"][nosky]).all(), label
    assert set(np.unique(m["end"])) <= {R.END_SKY, R.END_OPAQUE}, label
    assert (m["id"] != K.NONE).all() and (m["id"] >= K.NONE).all(), label
    assert (m["end"][m["id"] == K.SKY] == R.END_SKY).all(), label


def check_against_the_oracle(oracle, tm, scene, m, f, s, sky, label, filter_mode=0):
    """end by check_end's rule; sky_uv is sky_uv_np(sky_dir); the sampler at sky_uv is the FragColor of the
    pure-sky rays; deferred shading of the maps is the FragColor where the first surface is opaque, with
    hit_step the oracle's steps."""
    want = np.where(sky, R.END_SKY, R.END_OPAQUE)
    bad = m["end"] != want
    assert not bad.any(), f"{label}: end differs on {int(bad.sum())} of {bad.size} rays, first {np.flatnonzero(bad)[:4].tolist()}"
    k = m["end"] == R.END_SKY
    assert R.same_bits(m["sky_uv"][k], R.sky_uv_np(m["sky_dir"][k])).all(), label
    pure = m["id"] == K.SKY
    got = np.stack([oracle.sample_texture(tm.sky, u, v, filter_mode) for u, v in m["sky_uv"][pure]])
    ok = R.same_bits(got, f[pure]).all(-1)
    assert ok.all(), f"{label}: {int((~ok).sum())} of {int(pure.sum())} pure-sky rays differ from the oracle"
    k = (m["id"] >= 0) & (m["hit_base"][..., 3] == 1.0)
    rgb = R.deferred_frame(scene, np.where(k, m["id"], -1), m["hit_point"], m["hit_normal"], m["hit_view"], m["hit_base"])
    ok = R.same_bits(rgb[k], f[k][:, :3]).all(-1) & (f[k][:, 3] == 1.0)
    assert ok.all(), f"{label}: {int((~ok).sum())} of {int(k.sum())} opaque-first-surface rays differ from the oracle"
    assert np.array_equal(m["hit_step"][k], s[k]), f"{label}: hit_step differs on {int((m['hit_step'][k] != s[k]).sum())}"
    return int(pure.sum()), int(k.sum())


# ---- 1. camera rays equal the frame path ---------------------------------------------------
# (scene key of test_gpu_ray_maps.Cells, overlay, camera, w, h, projection case of projection_cases or None)
FRAME_CELLS = [(key, overlay, "view", W, H, None) for key, overlay in T.CAMERA_SETS]
FRAME_CELLS += [("features", False, look, 34, 22, None) for look in LOOKS]
FRAME_CELLS += [("stacked-through", False, "view", W, H, None), ("front", False, "rect", W, H, None),
                ("behind", False, "rect", W, H, None)]
FRAME_CELLS += [("small", False, "view", None, None, case) for case in
                ("equirect-64x32-fov360", "fisheye-41x41-fov180", "fisheye-48x48-fov360")]
# (raytrace_type, steps, culling): curved at 0, 1, 7 and 400 steps and flat, each with culling on and off
LAUNCHES = [(T.CURVED, steps, cull) for steps in (0, 1, 7, 400) for cull in (True, False)] + \
           [(T.FLAT, 400, True), (T.FLAT, 400, False)]


def frame_maps(gpu, cam, params, w, h, projection, cull):
    """sr_ray_maps after sr_render of the camera -> {map: [w * h(, n)]}, row-major."""
    import torch

    gpu.set_projection(projection)
    gpu.set_culling(cull)
    gpu.render(cam, params, w, h)
    m = gpu.ray_maps(MAPS)
    torch.cuda.synchronize()
    gpu.set_projection("rectilinear")
    return squeeze({k: v.cpu().numpy().reshape(w * h, -1) for k, v in m.items()})


@pytest.mark.parametrize("key,overlay,camera,w,h,case", FRAME_CELLS,
                         ids=[f"{c[0]}-{'overlay-' if c[1] else ''}{c[5] or c[2]}" for c in FRAME_CELLS])
def test_camera_rays_equal_the_frame_path(gpu, pkg, cells, key, overlay, camera, w, h, case):
    """trace_ray_maps(camera_rays(cam)) == sr_ray_maps after sr_render of the same camera: all nine maps, every
    pixel. Only the fisheye's pixels without a ray (a NaN direction) are left out, and held to sr_trace_rays.

    The frames of the whole-sphere projections are rendered with culling off at 7 steps: with culling on the
    frame kernels miss what the reference's arithmetic does to rays near the outward radius under a step angle of
    a radian (tests/test_gpu_trace.py test_fisheye_pixels_without_a_ray); the traced side runs both settings."""
    projection, fov = PJ.RECTILINEAR, None
    if case is not None:
        _, projection, w, h, fov = PJ.BY_ID[case]
    cam = PJ.with_fov(pkg, cells.cams[camera], fov)
    O, V = pkg.camera_rays(cam, projection, w, h)
    O, V = O.reshape(-1, 3), V.reshape(-1, 3)
    ray = ~np.isnan(V).any(-1)
    assert not (np.signbit(V) & (V == 0)).any(), "a -0 component: the trace's 0 + V would lose its sign"
    if case == "fisheye-48x48-fov360":
        assert (~ray).sum() == 500 and (np.isnan(V).all(-1) == ~ray).all()
    else:
        assert ray.all()
    wide = fov == 360.0
    try:
        for mode, steps, cull in LAUNCHES:
            label = f"{key} {case or camera} mode {mode} steps {steps} cull {cull}"
            prm = cells.params(steps, raytrace_type=mode)
            setup(gpu, cells.scene(key), cells.wd.test_rays[overlay], arr=cells.farr if key == "features" else cells.arr)
            want = frame_maps(gpu, cam, prm, w, h, projection, cull and not (wide and steps == 7))
            gpu.set_culling(cull)
            got = traced(gpu, O, V, prm)
            same_maps(got, want, label, sel=ray)
            check_fill(got, label)
            if not ray.all():  # no ray in the frame; the traced ray is what NaN arithmetic gives
                assert (want["end"][~ray] == R.END_NONE).all() and (want["id"][~ray] == K.NONE).all()
                assert np.array_equal(got["id"][~ray], trace(gpu, O, V, prm)["ids"][~ray]), label
                assert (got["end"][~ray] != R.END_NONE).all(), label
    finally:
        setup(gpu, cells.scene("small"), cells.wd.test_rays[False], arr=cells.arr)


# ---- 2. scattered rays equal the oracle ----------------------------------------------------
@pytest.mark.parametrize("cull", (True, False), ids=("cull", "nocull"))
@pytest.mark.parametrize("mode", (T.CURVED, T.FLAT), ids=("curved", "flat"))
@pytest.mark.parametrize("key,overlay", T.SCATTERED)
def test_scattered_sets_equal_the_oracle(gpu, oracle, tm, key, overlay, mode, cull):
    """The scattered sets under the rig, all 680 rays, one 1x1 oracle frame per ray and sky, in both filter
    modes (a textured surface's alpha, and with it `end`, is the filter's)."""
    scene = tm.scene(key)
    setup(gpu, scene, tm.tr.wd.test_rays[overlay], cull)
    O, V, _ = tm.rays(key)
    for prm in ({}, {"filter_mode": 1}):
        label = f"{key} overlay={overlay} mode={mode} cull={cull} {prm}"
        params = tm.params(raytrace_type=mode, **prm)
        gpu.set_culling(cull)
        m = traced(gpu, O, V, params)
        t = trace(gpu, O, V, params)
        gpu.set_culling(True)
        f, s = tm.ref(key, overlay, mode, **prm)
        # the two entry points agree with the oracle's frames and with each other
        assert R.same_bits(t["rgba32"], f).all() and np.array_equal(t["steps"], s), label
        assert np.array_equal(m["id"], t["ids"]), f"{label}: id differs from sr_trace_rays on {int((m['id'] != t['ids']).sum())}"
        check_fill(m, label)
        pure, lit = check_against_the_oracle(oracle, tm, scene, m, f, s, tm.ends_in_sky(key, overlay, mode, **prm), label,
                                             filter_mode=int(params.filter_mode))
        print(f"MEASURED {label}: {pure} pure-sky rays, {lit} opaque first surfaces of {len(O)}")
        assert pure >= 10 and lit >= 10
    # the oracle's codes are decoded from its frames of the recoloured scene (pick_cases' method), on which
    # tests/test_gpu_trace.py holds sr_trace_rays' ids to them: recolouring makes every object double-sided
    # but the flagged ones and has its own overlay, so the codes are that scene's
    label = f"{key} overlay={overlay} mode={mode} cull={cull} recoloured"
    setup(gpu, tm.tr.pick_passes(key)[0], tm.tr.pick_test_ray(overlay), cull)
    params = tm.params(raytrace_type=mode)
    m, only = traced(gpu, O, V, params), traced(gpu, O, V, params, ("id",))
    ids = trace(gpu, O, V, params)["ids"]
    gpu.set_culling(True)
    codes, ok = tm.tr.scattered_codes(key, overlay, mode)
    bad = (m["id"] != codes) & ok
    assert not bad.any(), f"{label}: {int(bad.sum())} of {int(ok.sum())} ids differ from the oracle's codes"
    assert np.array_equal(m["id"], ids) and np.array_equal(only["id"], ids), label
    check_fill(m, label)


# ---- 3. shapes ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full(gpu, tm):
    """The maps of the ("default", overlay) set, held to the oracle above."""
    setup(gpu, tm.scene("default"), tm.tr.wd.test_rays[True])
    O, V, _ = tm.rays("default")
    return traced(gpu, O, V, tm.params())


@pytest.mark.parametrize("n", (1, 63, 64, 65, 257))
def test_ray_counts(gpu, tm, full, n):
    setup(gpu, tm.scene("default"), tm.tr.wd.test_rays[True])
    O, V, _ = tm.rays("default")
    got = traced(gpu, O[:n], V[:n], tm.params())
    for k in MAPS:
        assert got[k].shape[0] == n
    same_maps(got, {k: v[:n] for k, v in full.items()}, f"n={n}")


def test_wave_mates_do_not_matter(gpu, tm, full):
    """A permuted set gives permuted maps; a ray alone gives the maps it has among unrelated wave-mates."""
    setup(gpu, tm.scene("default"), tm.tr.wd.test_rays[True])
    O, V, _ = tm.rays("default")
    perm = np.random.default_rng(11).permutation(len(O))
    got = traced(gpu, O[perm], V[perm], tm.params())
    same_maps(got, {k: v[perm] for k, v in full.items()}, "permuted")
    classes = [np.flatnonzero(full["id"] >= 0), np.flatnonzero(full["id"] == K.SKY), np.flatnonzero(full["id"] == K.HOLE),
               np.flatnonzero(np.isin(full["id"], (K.TR_FLAT, K.TR_CURVED))), np.flatnonzero(~T.finite_rays(O, V))]
    for idx in classes:
        assert len(idx) >= 2
        for i in idx[[0, -1]]:
            alone = traced(gpu, O[i:i + 1], V[i:i + 1], tm.params())
            same_maps(alone, {k: v[i:i + 1] for k, v in full.items()}, f"ray {i} alone")


# ---- 4. subsets -----------------------------------------------------------------------------
class Raw:
    """Sentinel-filled device buffers, every pointer 4-byte but not 16-byte aligned, and sr_trace_ray_maps called
    on raw pointers."""

    def __init__(self, gpu, abi, O, V, offset=4, pad=64):
        import torch

        self.gpu, self.abi, self.n, self.offset = gpu, abi, len(O), offset
        self.size = {k: 4 * c for k, (c, _) in abi.RAY_MAPS.items()}
        self.buf = {k: torch.full((offset + self.n * sz + pad,), SENT, dtype=torch.uint8, device="cuda")
                    for k, sz in self.size.items()}
        self.inputs = []
        for a in (O, V):
            raw = np.full(offset + a.size * 4, SENT, dtype=np.uint8)
            raw[offset:] = np.ascontiguousarray(a, dtype=np.float32).view(np.uint8).reshape(-1)
            self.inputs.append(torch.from_numpy(raw).cuda())

    def ptr(self, k, shift=0):
        return self.buf[k].data_ptr() + self.offset + shift

    def maps(self, which, shift=None):
        p = self.abi.RayMapPtrs()
        for k in which:
            setattr(p, k, self.ptr(k, 2 if k == shift else 0))
        return p

    def call(self, params, which, n=None, o=None, d=None, maps=None, ctx=True, null_maps=False):
        o = C.c_void_p(self.inputs[0].data_ptr() + self.offset) if o is None else o
        d = C.c_void_p(self.inputs[1].data_ptr() + self.offset) if d is None else d
        maps = self.maps(which) if maps is None else maps
        return self.gpu.lib.sr_trace_ray_maps(self.gpu.ctx if ctx else None, o, d, self.n if n is None else n,
                                              C.byref(params) if params is not None else None,
                                              None if null_maps else C.byref(maps), self.gpu._stream(None))

    def host(self):
        import torch

        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.buf.items()}

    def untouched(self):
        return all((v == SENT).all() for v in self.host().values())

    def written(self, which, label):
        """{map: [n(, c)]} of `which`; the bytes around them and every other buffer still hold the sentinel."""
        out, h = {}, self.host()
        for k, sz in self.size.items():
            lo, hi = self.offset, self.offset + self.n * sz
            assert (h[k][:lo] == SENT).all() and (h[k][hi:] == SENT).all(), (label, k, "wrote around its entries")
            if k not in which:
                assert (h[k][lo:hi] == SENT).all(), (label, k, "written though not requested")
                continue
            c, dtype = self.abi.RAY_MAPS[k]
            out[k] = h[k][lo:hi].copy().view(dtype).reshape(self.n, c)
        for a in self.inputs:
            assert (a.cpu().numpy()[:self.offset] == SENT).all()
        return squeeze(out)


def test_only_requested_maps_are_written(gpu, pkg, tm, cells):
    """Each single map and the hit maps without `end`, into sentinel-framed buffers; on the stacked translucent
    layers the hit maps' bytes are the same whether or not the ray is walked to its end (the early exit)."""
    setup(gpu, tm.scene("default"), tm.tr.wd.test_rays[True])
    O, V, _ = tm.rays("default")
    n = 130
    O, V = O[:n], V[:n]
    want = traced(gpu, O, V, tm.params())
    for which in [(k,) for k in MAPS] + [HITS, ("id",) + HITS, MAPS]:
        raw = Raw(gpu, pkg.abi, O, V)
        for k in MAPS:
            assert raw.ptr(k) % 16 != 0 and raw.ptr(k) % 4 == 0
        assert raw.call(tm.params(), which) == pkg.abi.SR_OK
        same_maps(raw.written(which, which), want, str(which), which)
    try:
        setup(gpu, cells.scene("stacked-through"), cells.wd.test_rays[False])
        O, V = pkg.camera_rays(cells.cams["view"], "rectilinear", 34, 22)
        O, V = O.reshape(-1, 3), V.reshape(-1, 3)
        walked = traced(gpu, O, V, cells.params())
        first = traced(gpu, O, V, cells.params(), HITS)
        assert (walked["id"] == 0).all() and (walked["end"] != R.END_OPAQUE).mean() > 0.5  # every ray goes on behind
        for k in HITS:
            assert walked[k].tobytes() == first[k].tobytes(), k
    finally:
        setup(gpu, cells.scene("small"), cells.wd.test_rays[False])


# ---- 5. state -------------------------------------------------------------------------------
def test_the_retained_frame_survives(gpu, tm, cells):
    """sr_render, then a trace-maps launch on other rays: the pixel state, sr_reshade, sr_ray_maps, sr_pick_map,
    the learned launch order and sr_diag_counters are as before, byte for byte."""
    import torch

    setup(gpu, cells.scene("stacked-through"), cells.wd.test_rays[False])  # its pixels' ends come from the resume path
    cam, prm = cells.cams["view"], cells.params()
    gpu.render(cam, prm, W, H)
    gpu.render(cam, prm, W, H)

    def snapshot():
        shade, picks, maps = gpu.reshade(), gpu.pick_map(), gpu.ray_maps(MAPS)
        torch.cuda.synchronize()
        out = {"reshade": shade.cpu().numpy(), "pick": picks.cpu().numpy(), "state": gpu.pixel_state().copy(),
               "order": np.array(gpu.last_order()), "diag": gpu.diag_counters()}
        out.update({"map " + k: v.cpu().numpy() for k, v in maps.items()})
        return out

    before = snapshot()
    assert before["diag"] == {"hit_not_opaque": 0, "free_errors": 0}
    O, V, _ = tm.rays("large")
    got = traced(gpu, O, V, tm.params(150))
    assert len(got["id"]) == len(O) and gpu.can_reshade()
    after = snapshot()
    for k, v in before.items():
        assert (v == after[k]) if k == "diag" else v.tobytes() == after[k].tobytes(), k
    setup(gpu, cells.scene("small"), cells.wd.test_rays[False])


def test_setters_between_launches_take_effect(gpu, pkg, cells):
    """A shading-only sr_set_scene changes hit_base and hit_normal and nothing else; sr_set_texture_array takes
    effect; a context that never had a background gives the same maps."""
    sc, abi = pkg.scenes, pkg.abi
    old = cells.scene("features")
    new = sc.struct_from_bytes(abi.Scene, sc.struct_bytes(old))
    for m in new.materials:
        m.color[0], m.color[1], m.color[2] = m.color[2], 0.75, m.color[0]
        m.normal_map_index = 1 if m.normal_map_index < 0 else -1
    assert abi.scene_shading_only(old, new)
    O, V = pkg.camera_rays(cells.cams["sphere"], "rectilinear", 34, 22)
    O, V = O.reshape(-1, 3), V.reshape(-1, 3)
    prm = cells.params()
    try:
        setup(gpu, old, cells.wd.test_rays[False], arr=cells.farr)
        first = traced(gpu, O, V, prm)
        valid = first["id"] >= 0
        assert valid.sum() >= 0.05 * len(O)
        gpu.set_scene(new)
        got = traced(gpu, O, V, prm)
        same_maps(got, first, "shading-only change", ("end", "id", "sky_dir", "sky_uv", "hit_point", "hit_view", "hit_step"))
        assert differing(got["hit_base"][valid], first["hit_base"][valid]).any()
        assert differing(got["hit_normal"][valid], first["hit_normal"][valid]).any()
        gpu.set_scene(old)
        gpu.set_texture_array(cells.arr)
        other = traced(gpu, O, V, prm)
        assert differing(other["hit_base"][valid], first["hit_base"][valid]).any()
        # (a textured surface's alpha is the array's: `end` and the sky maps may change with it)
        same_maps(other, first, "another texture array", ("id", "hit_point", "hit_view", "hit_step"))
        gpu.set_texture_array(cells.farr)
        same_maps(traced(gpu, O, V, prm), first, "the first array again")
        bare = pkg.Renderer(0)
        try:
            bare.set_texture_array(cells.farr)
            bare.set_scene(old)
            same_maps(traced(bare, O, V, prm), first, "no background")
        finally:
            bare.close()
    finally:
        setup(gpu, cells.scene("small"), cells.wd.test_rays[False], arr=cells.arr)


# ---- 6. params and context settings ---------------------------------------------------------
def test_ignored_params_and_context_settings(gpu, tm, full):
    """crosshair, percent_black, curved_percentage, a projection, split tiles, the latency mode and a scene
    sequence leave the bytes alone."""
    setup(gpu, tm.scene("default"), tm.tr.wd.test_rays[True])
    O, V, _ = tm.rays("default")
    same_maps(traced(gpu, O, V, tm.params(crosshair=1, percent_black=0.75, curved_percentage=0.2)), full, "ignored params")
    gpu.set_projection("fisheye")
    gpu.set_split(8, 16, 1)
    gpu.set_latency_mode(True)
    gpu.set_scene_sequence([tm.scene("large"), tm.scene("default")])
    try:
        same_maps(traced(gpu, O, V, tm.params()), full, "projection, split tiles, latency mode and a sequence set")
    finally:
        gpu.set_projection("rectilinear")
        gpu.set_split(0)
        gpu.set_latency_mode(False)
        gpu.set_scene_sequence([])


@pytest.mark.parametrize("prm", ({"max_revolutions": 0}, {"u_f": -0.01}, {"max_steps": 57, "max_revolutions": 1},
                                 {"max_steps": 100}, {"max_steps": 126}, {"max_steps": 7}, {"max_steps": 150, "max_revolutions": 3},
                                 {"u_f": 0.05}, {"filter_mode": 1}),
                         ids=("revolutions0", "u_f-negative", "57x1", "100x2", "126x2", "7x2", "150x3", "u_f0.05", "weighted"))
def test_honoured_params(gpu, oracle, tm, prm):
    """max_steps, max_revolutions, u_f and filter_mode are the call's (tests/test_gpu_trace.py's sets): the
    oracle's frames of the same params."""
    key, overlay = "default", False
    scene = tm.scene(key)
    setup(gpu, scene, tm.tr.wd.test_rays[overlay])
    O, V, _ = tm.rays(key)
    p = dict(prm)
    steps = p.pop("max_steps", T.STEPS)
    params = tm.params(steps, **p)
    m = traced(gpu, O, V, params)
    t = trace(gpu, O, V, params)
    f, s = tm.ref(key, overlay, T.CURVED, "random", steps, **p)
    assert R.same_bits(t["rgba32"], f).all() and np.array_equal(t["steps"], s), str(prm)
    assert np.array_equal(m["id"], t["ids"]), str(prm)
    check_fill(m, str(prm))
    check_against_the_oracle(oracle, tm, scene, m, f, s, tm.ends_in_sky(key, overlay, T.CURVED, steps, **p), str(prm),
                             filter_mode=int(params.filter_mode))
    if "filter_mode" not in prm:
        assert not R.same_bits(f, tm.ref(key, overlay)[0]).all(), "the parameter changes nothing in this set"


# ---- 7. streams -----------------------------------------------------------------------------
def test_launches_around_a_render_and_a_trace_on_two_streams(gpu, tm, full):
    """Trace-maps launches queued before and after sr_render and sr_trace_rays, on one stream and across two,
    with no host wait between."""
    import torch

    setup(gpu, tm.scene("default"), tm.tr.wd.test_rays[True])
    O, V, _ = tm.rays("default")
    do, dv = dev(O), dev(V)
    cam, prm = tm.tr.wd.cams["view"], tm.params()
    frame_ref = gpu.render(cam, prm, W, H)
    trace_ref = gpu.trace_rays(do, dv, prm, rgba32=True)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for first, second in ((s1, s1), (s1, s2)):
        a = gpu.trace_ray_maps(do, dv, prm, stream=first)
        frame = gpu.render(cam, prm, W, H, stream=second)
        b = gpu.trace_ray_maps(do, dv, prm, stream=second)
        t = gpu.trace_rays(do, dv, prm, rgba32=True, stream=first)
        c = gpu.trace_ray_maps(do, dv, prm, stream=first)
        torch.cuda.synchronize()
        for got in (a, b, c):
            same_maps(squeeze({k: v.cpu().numpy() for k, v in got.items()}), full, "queued")
        assert torch.equal(frame, frame_ref) and t["rgba32"].cpu().numpy().tobytes() == trace_ref["rgba32"].cpu().numpy().tobytes()


# ---- 8. rejections --------------------------------------------------------------------------
def test_rejections_leave_the_buffers_untouched(gpu, pkg, tm, full):
    """Every rejection of sr.h on a live context: nothing written; n_rays = 0 is SR_OK."""
    import torch

    abi = pkg.abi
    setup(gpu, tm.scene("default"), tm.tr.wd.test_rays[True])
    O, V, _ = tm.rays("default")
    n = 70
    raw = Raw(gpu, abi, O[:n], V[:n], offset=0)
    good = tm.params()
    INV = abi.SR_E_INVALID
    cases = {
        "n < 0": dict(n=-1),
        "n above SR_TRACE_MAX_RAYS": dict(n=abi.TRACE_MAX_RAYS + 1),
        "null origins": dict(o=C.c_void_p(0)),
        "null dirs": dict(d=C.c_void_p(0)),
        "misaligned origins": dict(o=C.c_void_p(raw.inputs[0].data_ptr() + 2)),
        "misaligned dirs": dict(d=C.c_void_p(raw.inputs[1].data_ptr() + 1)),
        "null context": dict(ctx=False),
        "null maps": dict(null_maps=True),
        "all nine pointers null": dict(maps=abi.RayMapPtrs()),
    }
    for label, kw in cases.items():
        assert raw.call(good, MAPS, **kw) == INV, label
    for k in MAPS:
        assert raw.call(good, MAPS, maps=raw.maps(MAPS, shift=k)) == INV, f"misaligned {k}"
        assert raw.call(good, MAPS, maps=raw.maps((k,), shift=k)) == INV, f"misaligned {k} alone"
    assert raw.call(None, MAPS) == INV, "null params"
    for label, prm in (("half width", tm.params(raytrace_type=2)), ("half height", tm.params(raytrace_type=3)),
                       ("raytrace_type 4", tm.params(raytrace_type=4)), ("max_steps < 0", tm.params(-1)),
                       ("max_steps above SR_MAX_STEPS", tm.params(1 << 24)), ("filter_mode", tm.params(filter_mode=7))):
        assert raw.call(prm, MAPS) == INV, label
    assert raw.untouched()
    assert raw.call(good, MAPS, n=0) == abi.SR_OK
    assert raw.call(good, MAPS, n=0, o=C.c_void_p(0), d=C.c_void_p(0)) == abi.SR_OK
    assert raw.untouched()
    out = gpu.trace_ray_maps(torch.empty((0, 3), device="cuda"), torch.empty((0, 3), device="cuda"), good)
    assert out["hit_base"].shape == (0, 4) and out["id"].shape == (0, 1)
    with pytest.raises(ValueError):
        gpu.trace_ray_maps(dev(O[:n]), dev(V[:n]), good, which=("colour",))
    r = pkg.Renderer(0)  # a context without a scene: as sr_trace_rays
    try:
        raw2 = Raw(r, abi, O[:n], V[:n], offset=0)
        assert raw2.call(good, MAPS) == abi.SR_E_NOT_READY
        assert raw2.untouched()
    finally:
        r.close()
    # the context still works
    same_maps(traced(gpu, O[:n], V[:n], good), {k: v[:n] for k, v in full.items()}, "after the rejections")
