"""sr_trace_rays (sr.h "Ray queries") on the GPU: caller-supplied rays against
the oracle, the frame kernels and itself.

The references are tests/trace_cases.py's: an oracle frame for a camera-ray
set, one 1x1 oracle frame per ray for a scattered set, pick codes decoded from
the oracle's frames of the recoloured scenes. Nothing has a tolerance: float
FragColor bits per channel (NaN matches NaN), RGBA8 bytes, step counts, ids.
"""
import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest

import pick_cases as K
import projection_cases as P
import trace_cases as T

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
OUTS = ("rgba32", "rgba8", "steps", "ids")
SENT = 0x5A


@pytest.fixture(scope="module")
def tr(pkg, oracle, textures):
    return T.Traces(pkg, oracle, textures)


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


def dev(a):
    import torch

    return torch.from_numpy(np.array(a, dtype=np.float32, order="C")).cuda()  # (a copy: the references are read-only)


def trace(gpu, O, V, params, outs=OUTS, stream=None):
    """Renderer.trace_rays of host rays -> {name: host array}."""
    import torch

    got = gpu.trace_rays(dev(O), dev(V), params, **{k: k in outs for k in OUTS}, stream=stream)
    torch.cuda.synchronize()
    assert set(got) == set(outs)
    return {k: v.cpu().numpy() for k, v in got.items()}


def same_float(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def check(got, ref, label, codes=None):
    """got (trace's dict) against (rgba8, float rgba, steps) and, where given, (codes, decoded mask)."""
    b, f, s = ref
    msg = [f"{label}:"]
    bad = 0
    if "rgba32" in got:
        n = int((~same_float(got["rgba32"], f)).any(-1).sum())
        msg.append(f"float FragColor differs on {n}")
        bad += n
    if "rgba8" in got:
        n = int((got["rgba8"] != b).any(-1).sum())
        msg.append(f"RGBA8 on {n}")
        bad += n
    if "steps" in got:
        n = int((got["steps"] != s).sum())
        msg.append(f"steps on {n}")
        bad += n
    if codes is not None:
        want, ok = codes
        n = int(((got["ids"] != want) & ok).sum())
        msg.append(f"ids on {n}")
        bad += n
    assert bad == 0, " ".join(msg) + f" of {len(b)} rays"


def setup(gpu, tr, scene, test_ray, cull=True):
    gpu.set_culling(cull)
    gpu.set_projection("rectilinear")
    gpu.set_split(0)
    gpu.set_latency_mode(False)
    gpu.set_scene(scene)
    gpu.set_test_ray(test_ray)


def restore_textures(gpu, textures):
    bg, arr = textures
    gpu.set_background(bg)
    gpu.set_texture_array(arr)


# ---- exact against the oracle, culling on and off ------------------------------------
@pytest.mark.parametrize("cull", (True, False), ids=("cull", "nocull"))
@pytest.mark.parametrize("key,overlay", T.CAMERA_SETS)
def test_camera_sets_equal_the_oracle(gpu, tr, key, overlay, cull):
    """The 68x44 view's own rays: the oracle's frame, with culling on and off."""
    setup(gpu, tr, tr.wd.scene(key), tr.wd.test_rays[overlay], cull)
    O, V = tr.camera_set(key, overlay)
    got = trace(gpu, O, V, tr.params())
    check(got, tr.camera_ref(key, overlay), f"{key} overlay={overlay} cull={cull}")
    gpu.set_culling(True)


@pytest.mark.parametrize("cull", (True, False), ids=("cull", "nocull"))
@pytest.mark.parametrize("mode", (T.CURVED, T.FLAT), ids=("curved", "flat"))
@pytest.mark.parametrize("key,overlay", T.SCATTERED)
def test_scattered_sets_equal_the_oracle(gpu, tr, key, overlay, mode, cull):
    """Scattered origins and directions, one 1x1 oracle frame per ray."""
    setup(gpu, tr, tr.scene(key), tr.wd.test_rays[overlay], cull)
    O, V, _ = tr.rays(key)
    got = trace(gpu, O, V, tr.params(raytrace_type=mode), outs=("rgba32", "rgba8", "steps"))
    check(got, tr.scattered_ref(key, overlay, mode), f"{key} overlay={overlay} mode={mode} cull={cull}")
    gpu.set_culling(True)


@pytest.mark.parametrize("cull", (True, False), ids=("cull", "nocull"))
@pytest.mark.parametrize("mode", (T.CURVED, T.FLAT), ids=("curved", "flat"))
@pytest.mark.parametrize("key,overlay", T.SCATTERED)
def test_scattered_ids_equal_the_oracle(gpu, tr, textures, key, overlay, mode, cull):
    """The ids of the scattered sets on the recoloured scene (pick_cases'
    method), from a full launch and from an ids-only launch."""
    setup(gpu, tr, tr.pick_passes(key)[0], tr.pick_test_ray(overlay), cull)
    gpu.set_background(tr.picks.bg)
    O, V, _ = tr.rays(key)
    codes = tr.scattered_codes(key, overlay, mode)
    prm = tr.params(raytrace_type=mode)
    full = trace(gpu, O, V, prm)
    only = trace(gpu, O, V, prm, outs=("ids",))
    restore_textures(gpu, textures)
    gpu.set_culling(True)
    bad = (full["ids"] != codes[0]) & codes[1]
    assert not bad.any(), f"{int(bad.sum())} of {len(bad)} ids differ from the oracle's codes"
    assert np.array_equal(only["ids"], full["ids"]), "an ids-only launch reports other ids"
    assert (full["ids"] != K.NONE).all()


@pytest.mark.parametrize("case_id", ("default", "stress", "overlay", "translucent-front", "single-sided-behind",
                                     "single-sided-behind-flat", "flat"))
def test_pick_cases_ids(gpu, tr, pkg, textures, case_id):
    """pick_cases' frames as camera rays: a translucent front surface, a
    single-sided surface seen from behind, the overlay, the flat mode."""
    pk = tr.picks
    case = pk.cases[case_id]
    setup(gpu, tr, pk.passes(case)[0], pk.test_rays[case["overlay"]])
    gpu.set_background(pk.bg)
    seen = set()
    try:
        for cam in case["cams"]:
            O, V = pkg.camera_rays(pk.cams[cam], "rectilinear", case["w"], case["h"])
            zero = (np.signbit(V) & (V == 0)).any(-1).reshape(-1)
            want, ok = pk.codes(case, cam)
            full = trace(gpu, O.reshape(-1, 3), V.reshape(-1, 3), pk.params(case), outs=("ids", "rgba8"))
            only = trace(gpu, O.reshape(-1, 3), V.reshape(-1, 3), pk.params(case), outs=("ids",))
            use = ok.reshape(-1) & ~zero
            assert use.mean() > 0.9
            bad = (full["ids"] != want.reshape(-1)) & use
            assert not bad.any(), f"{case_id}/{cam}: {int(bad.sum())} ids differ"
            assert np.array_equal(only["ids"], full["ids"])
            seen |= set(np.unique(full["ids"][use]).tolist())
    finally:
        restore_textures(gpu, textures)
    assert set(case["covers"]) <= seen, (case_id, sorted(set(case["covers"]) - seen))


# ---- against the frame kernels ---------------------------------------------------------
def frame_and_trace(gpu, tr, pkg, projection, cam, steps, w, h, frame_cull=True):
    """(trace's outputs, the frame's (rgba8, float, steps), its pick map, V), rays row-major."""
    import torch

    setup(gpu, tr, tr.wd.scene("small"), tr.wd.test_rays[False], frame_cull)
    prm = tr.params(steps)
    gpu.set_projection(projection)
    f, b, s = gpu.render_debug(cam, prm, w, h)
    ids = gpu.pick_map()
    torch.cuda.synchronize()
    ref = tuple(a.cpu().numpy().reshape(-1, *a.shape[2:]) for a in (b, f, s))
    ids = ids.cpu().numpy().reshape(-1)
    gpu.set_culling(True)
    O, V = pkg.camera_rays(cam, projection, w, h)
    O, V = O.reshape(-1, 3), V.reshape(-1, 3)
    got = trace(gpu, O, V, prm)  # (the context's projection does not matter to a trace launch)
    gpu.set_projection("rectilinear")
    return got, ref, ids, V


@pytest.mark.parametrize("steps", (0, 1, 7, 2000))
@pytest.mark.parametrize("projection", (P.RECTILINEAR, P.EQUIRECT, P.FISHEYE), ids=("pinhole", "equirect", "fisheye"))
def test_camera_rays_equal_the_frame_kernels(gpu, tr, pkg, projection, steps):
    """trace_rays(camera_rays(...)) == sr_render_debug of the same camera and
    params, and sr_pick_map after it: the 33x17 frames of projection_cases
    (the "view" camera, its own fov) under the three projections."""
    w, h = 33, 17
    got, ref, ids, V = frame_and_trace(gpu, tr, pkg, projection, tr.wd.cams["view"], steps, w, h)
    assert not np.isnan(V).any()
    assert not (np.signbit(V) & (V == 0)).any()  # 0 + V: a -0 component would be another ray (sr.h)
    check(got, ref, f"projection {projection} steps {steps}", (ids, np.ones(len(ids), dtype=bool)))


@pytest.mark.parametrize("steps", (0, 1, 7, 2000))
def test_fisheye_pixels_without_a_ray(gpu, tr, pkg, steps):
    """The same at fov 360, where the fisheye's corner pixels have no ray:
    sr_camera_rays gives them a NaN direction, by which they are excluded.

    At 7 steps the frame is rendered with culling off. With culling on the
    frame kernels (unchanged here) miss what the reference's arithmetic does to
    rays that leave within a few degrees of the outward radius under a step
    angle of a radian or more: 8 of this frame's 537 rays differ from the
    oracle at 7 steps (20 from the "view" camera; up to 54 at 5 steps, 4 at
    12, none at 25 or 2000), while the culling-off frame and the trace launch
    equal it. A trace launch culls only up to SR_TRACE_DPHI_MAX for this
    reason (device_scene.h; test_coarse_schedules_equal_the_oracle)."""
    w, h = 33, 17
    cam = P.with_fov(pkg, tr.wd.cams["fly1"], 360.0)
    got, ref, ids, V = frame_and_trace(gpu, tr, pkg, P.FISHEYE, cam, steps, w, h, frame_cull=steps != 7)
    ray = ~np.isnan(V).any(-1)
    assert (np.isnan(V).all(-1) == ~ray).all() and 0 < (~ray).sum() < 0.1 * len(ray)
    assert (ids[~ray] == K.NONE).all() and (ref[2][~ray] == 0).all()
    use = ray & ~(np.signbit(V) & (V == 0)).any(-1)
    assert use.sum() >= 0.9 * ray.sum()
    check({k: v[use] for k, v in got.items()}, tuple(a[use] for a in ref), f"fisheye 360 steps {steps}",
          (ids[use], np.ones(int(use.sum()), dtype=bool)))


@pytest.mark.parametrize("steps", (2, 5, 7, 12, 25, 63, 126))
@pytest.mark.parametrize("projection,camera", ((P.EQUIRECT, "view"), (P.FISHEYE, "view"), (P.FISHEYE, "fly1")),
                         ids=("equirect-view", "fisheye-view", "fisheye-fly1"))
def test_coarse_schedules_equal_the_oracle(gpu, tr, pkg, projection, camera, steps):
    """Rays in every direction (a whole sphere's, fov 360) under step angles
    from 6.3 rad down to 0.1: the oracle's 1x1 frames, with culling on. Rays
    near the outward radius are flung back into the hole by the reference's
    arithmetic at the coarse end; a trace launch runs the reference's loop
    above SR_TRACE_DPHI_MAX (63 steps: 0.2 rad; 126: just below 0.1)."""
    w, h = 33, 17
    cam = P.with_fov(pkg, tr.wd.cams[camera], 360.0)
    setup(gpu, tr, tr.wd.scene("small"), tr.wd.test_rays[False])
    O, V = pkg.camera_rays(cam, projection, w, h)
    ray = ~np.isnan(V).any(-1).reshape(-1)
    O, V = O.reshape(-1, 3)[ray], V.reshape(-1, 3)[ray]
    prm = tr.params(steps)
    got = trace(gpu, O, V, prm, outs=("rgba32", "rgba8", "steps"))
    check(got, T.ray_frames(tr.pkg, tr.oracle, tr.wd.scene("small"), O, V, prm, tr.tex, tr.wd.test_rays[False]),
          f"{camera} projection {projection} steps {steps}")


# ---- ray counts, wave shapes, wave-mates --------------------------------------------------
@pytest.mark.parametrize("n", (1, 63, 64, 65, 257))
def test_ray_counts(gpu, tr, n):
    """The first n rays of a set give the first n results (the full set: above)."""
    key, overlay = "default", True
    setup(gpu, tr, tr.scene(key), tr.wd.test_rays[overlay])
    O, V, _ = tr.rays(key)
    got = trace(gpu, O[:n], V[:n], tr.params(), outs=("rgba32", "rgba8", "steps"))
    check(got, tuple(a[:n] for a in tr.scattered_ref(key, overlay)), f"n={n}")


@pytest.mark.parametrize("key,overlay", (("default", True), ("large", False)))
def test_wave_mates_do_not_matter(gpu, tr, key, overlay):
    """A random permutation of a set gives the same outputs, permuted."""
    setup(gpu, tr, tr.scene(key), tr.wd.test_rays[overlay])
    O, V, _ = tr.rays(key)
    perm = np.random.default_rng(11).permutation(len(O))
    a = trace(gpu, O, V, tr.params())
    b = trace(gpu, O[perm], V[perm], tr.params())
    for k in OUTS:
        assert a[k][perm].tobytes() == b[k].tobytes(), k
    check(b, tuple(x[perm] for x in tr.scattered_ref(key, overlay)), "permuted")


# ---- buffers --------------------------------------------------------------------------------
class Raw:
    """Sentinel-filled device buffers and sr_trace_rays called on raw pointers at a byte offset."""

    SIZE = {"rgba32": 16, "rgba8": 4, "steps": 4, "ids": 4}

    def __init__(self, gpu, n, offset=4, pad=64):
        import torch

        self.gpu, self.n, self.offset, self.pad = gpu, n, offset, pad
        self.buf = {k: torch.full((offset + n * sz + pad,), SENT, dtype=torch.uint8, device="cuda")
                    for k, sz in self.SIZE.items()}

    def rays(self, O, V):
        import torch

        out = []
        for a in (O, V):
            raw = np.full(self.offset + a.size * 4, SENT, dtype=np.uint8)
            raw[self.offset:] = np.ascontiguousarray(a, dtype=np.float32).view(np.uint8).reshape(-1)
            out.append(torch.from_numpy(raw).cuda())
        self.inputs = out
        return out

    def ptr(self, k):
        return C.c_void_p(self.buf[k].data_ptr() + self.offset)

    def call(self, params, outs, n=None, o=None, d=None, **replace):
        args = {k: (self.ptr(k) if k in outs else None) for k in OUTS}
        args.update(replace)
        o = C.c_void_p(self.inputs[0].data_ptr() + self.offset) if o is None else o
        d = C.c_void_p(self.inputs[1].data_ptr() + self.offset) if d is None else d
        return self.gpu.lib.sr_trace_rays(self.gpu.ctx, o, d, self.n if n is None else n,
                                          C.byref(params) if params is not None else None, args["rgba32"],
                                          args["rgba8"], args["steps"], args["ids"], self.gpu._stream(None))

    def host(self):
        import torch

        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.buf.items()}

    def untouched(self):
        return all((v == SENT).all() for v in self.host().values())


def test_only_requested_outputs_are_written(gpu, tr, pkg):
    """Sentinel buffers, every pointer 4-byte but not 16-byte aligned: a launch
    writes the requested outputs' n entries and nothing else; an ids-only
    launch gives the full launch's ids."""
    key, overlay = "default", False
    setup(gpu, tr, tr.scene(key), tr.wd.test_rays[overlay])
    O, V, _ = tr.rays(key)
    n = 130
    ref = tr.scattered_ref(key, overlay)
    for outs in (OUTS, ("rgba8",), ("rgba32", "steps"), ("ids",)):
        raw = Raw(gpu, n)
        raw.rays(O[:n], V[:n])
        for k in OUTS:
            assert raw.ptr(k).value % 16 != 0 and raw.ptr(k).value % 4 == 0
        assert raw.call(tr.params(), outs) == pkg.abi.SR_OK
        h = raw.host()
        for k, sz in Raw.SIZE.items():
            body = h[k][raw.offset:raw.offset + n * sz]
            assert (h[k][:raw.offset] == SENT).all() and (h[k][raw.offset + n * sz:] == SENT).all(), (outs, k)
            if k not in outs:
                assert (body == SENT).all(), (outs, k, "written though not requested")
        if "rgba8" in outs:
            assert np.array_equal(h["rgba8"][4:4 + 4 * n].reshape(n, 4), ref[0][:n])
        if "steps" in outs:
            assert np.array_equal(h["steps"][4:4 + 4 * n].view(np.int32), ref[2][:n])
        if "rgba32" in outs:
            assert same_float(h["rgba32"][4:4 + 16 * n].view(np.float32).reshape(n, 4), ref[1][:n]).all()
        if "ids" in outs:
            ids = h["ids"][4:4 + 4 * n].view(np.int32)
            if len(outs) == 4:
                full_ids = ids.copy()
            else:
                assert np.array_equal(ids, full_ids)
        for a in raw.inputs:
            assert (a.cpu().numpy()[:raw.offset] == SENT).all()


# ---- params -----------------------------------------------------------------------------------
def test_ignored_params_and_context_settings(gpu, tr):
    """crosshair, percent_black, curved_percentage, a projection, split tiles
    and the latency mode leave a trace launch's bytes unchanged."""
    key, overlay = "default", True
    setup(gpu, tr, tr.scene(key), tr.wd.test_rays[overlay])
    O, V, _ = tr.rays(key)
    ref = tr.scattered_ref(key, overlay)
    check(trace(gpu, O, V, tr.params(crosshair=1, percent_black=0.75, curved_percentage=0.2)), ref, "ignored params")
    gpu.set_projection("fisheye")
    gpu.set_split(8, 16, 1)
    gpu.set_latency_mode(True)
    try:
        check(trace(gpu, O, V, tr.params()), ref, "projection, split tiles and latency mode set")
    finally:
        gpu.set_projection("rectilinear")
        gpu.set_split(0)
        gpu.set_latency_mode(False)


@pytest.mark.parametrize("prm", ({"max_revolutions": 0}, {"u_f": -0.01}, {"max_steps": 57, "max_revolutions": 1},
                                 {"max_steps": 100}, {"max_steps": 126}, {"max_steps": 7}, {"max_steps": 150, "max_revolutions": 3},
                                 {"u_f": 0.05}, {"filter_mode": 1}),
                         ids=("revolutions0", "u_f-negative", "57x1", "100x2", "126x2", "7x2", "150x3", "u_f0.05", "weighted"))
def test_honoured_params(gpu, tr, prm):
    """max_steps, max_revolutions, u_f and filter_mode are the call's: the
    oracle's frames of the same params (the first two run the reference's loop)."""
    key, overlay = "default", False
    setup(gpu, tr, tr.scene(key), tr.wd.test_rays[overlay])
    O, V, _ = tr.rays(key)
    p = dict(prm)
    steps = p.pop("max_steps", T.STEPS)
    got = trace(gpu, O, V, tr.params(steps, **p), outs=("rgba32", "rgba8", "steps"))
    ref = T.ray_frames(tr.pkg, tr.oracle, tr.scene(key), O, V, tr.params(steps, **p), tr.tex, tr.wd.test_rays[overlay])
    check(got, ref, str(prm))
    if "filter_mode" not in prm:
        assert (ref[0] != tr.scattered_ref(key, overlay)[0]).any(), "the parameter changes nothing in this set"


# ---- context state ------------------------------------------------------------------------------
def test_a_trace_keeps_the_retained_frame(gpu, tr, pkg):
    """sr_render of scene A, a trace launch, sr_reshade: the reshade's bytes
    are those without the trace, sr_can_reshade stays 1, the learned launch
    order stays, and sr_diag_counters stays 0."""
    import torch

    setup(gpu, tr, tr.wd.scene("small"), tr.wd.test_rays[False])
    cam, prm, w, h = tr.wd.cams["view"], tr.params(), T.W, T.H
    frame = gpu.render(cam, prm, w, h)
    plain = gpu.reshade()
    picks = gpu.pick_map()
    frame = gpu.render(cam, prm, w, h)
    order = gpu.last_order()
    assert gpu.can_reshade()
    O, V, _ = tr.rays("default")
    got = trace(gpu, O, V, tr.params(150))
    assert gpu.can_reshade() and np.array_equal(gpu.last_order(), order)
    after, picks_after = gpu.reshade(), gpu.pick_map()
    torch.cuda.synchronize()
    assert torch.equal(after, plain) and torch.equal(after, frame) and torch.equal(picks_after, picks)
    assert np.array_equal(frame.cpu().numpy(), tr.wd.ref("small", False)[0])
    assert len(got["steps"]) == len(O)
    assert gpu.diag_counters() == {"hit_not_opaque": 0, "free_errors": 0}


def test_traces_around_a_render_on_one_and_two_streams(gpu, tr):
    """Traces queued before and after sr_render, on one stream and across two, with no host wait between."""
    import torch

    key, overlay = "default", False
    setup(gpu, tr, tr.wd.scene("small"), tr.wd.test_rays[overlay])  # the default scene's geometry, its own materials
    O, V, _ = tr.rays(key)
    do, dv = dev(O), dev(V)
    ref = T.ray_frames(tr.pkg, tr.oracle, tr.wd.scene("small"), O, V, tr.params(), tr.tex, tr.wd.test_rays[overlay])
    frame_ref = tr.wd.ref("small", overlay)[0]
    cam = tr.wd.cams["view"]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for first, second in ((s1, s1), (s1, s2)):
        a = gpu.trace_rays(do, dv, tr.params(), rgba32=True, steps=True, ids=True, stream=first)
        frame = gpu.render(cam, tr.params(), T.W, T.H, stream=second)
        b = gpu.trace_rays(do, dv, tr.params(), rgba32=True, steps=True, ids=True, stream=first)
        torch.cuda.synchronize()
        for got in (a, b):
            check({k: v.cpu().numpy() for k, v in got.items() if k != "ids"}, ref, "queued")
        assert torch.equal(a["ids"], b["ids"])
        assert np.array_equal(frame.cpu().numpy(), frame_ref)


def test_setters_between_traces_take_effect(gpu, tr, pkg, textures):
    """sr_set_scene, sr_set_test_ray, sr_set_background and sr_set_texture_array between traces."""
    O, V, _ = tr.rays("default")
    prm = tr.params()
    sc = pkg.scenes

    def ref(scene, overlay, tex):
        return T.ray_frames(tr.pkg, tr.oracle, scene, O, V, prm, tex, tr.wd.test_rays[overlay])

    setup(gpu, tr, tr.scene("default"), tr.wd.test_rays[False])
    first = trace(gpu, O, V, prm)
    check(first, tr.scattered_ref("default", False), "start")
    try:
        gpu.set_scene(tr.wd.scene("general"))
        got = trace(gpu, O, V, prm)
        check(got, ref(tr.wd.scene("general"), False, tr.tex), "after sr_set_scene")
        assert (got["rgba8"] != first["rgba8"]).any()
        gpu.set_test_ray(tr.wd.test_rays[True])
        got2 = trace(gpu, O, V, prm)
        check(got2, ref(tr.wd.scene("general"), True, tr.tex), "after sr_set_test_ray")
        assert (got2["rgba8"] != got["rgba8"]).any()
        bg2 = np.ascontiguousarray(textures[0][::-1, ::-1])
        gpu.set_background(bg2)
        got3 = trace(gpu, O, V, prm)
        check(got3, ref(tr.wd.scene("general"), True, tr.oracle.TextureSet(bg2, textures[1])), "after sr_set_background")
        assert (got3["rgba8"] != got2["rgba8"]).any()
        arr2 = sc.feature_texture_array()[0]
        gpu.set_scene(tr.scene("default"))
        gpu.set_texture_array(arr2)
        got4 = trace(gpu, O, V, prm)
        check(got4, ref(tr.scene("default"), True, tr.oracle.TextureSet(bg2, arr2)), "after sr_set_texture_array")
    finally:
        restore_textures(gpu, textures)


# ---- rejections -----------------------------------------------------------------------------------
def test_rejections_leave_the_buffers_untouched(gpu, tr, pkg):
    """Every rejection of sr.h on a live context: SR_E_INVALID, nothing written; n_rays = 0 is SR_OK."""
    import torch

    abi = pkg.abi
    setup(gpu, tr, tr.scene("default"), tr.wd.test_rays[False])
    O, V, _ = tr.rays("default")
    n = 70
    raw = Raw(gpu, n, offset=0)
    raw.rays(O[:n], V[:n])
    good = tr.params()
    odd = C.c_void_p(raw.buf["rgba32"].data_ptr() + 2)
    cases = {
        "n < 0": dict(n=-1),
        "n above SR_TRACE_MAX_RAYS": dict(n=abi.TRACE_MAX_RAYS + 1),
        "null origins": dict(o=C.c_void_p(0)),
        "null dirs": dict(d=C.c_void_p(0)),
        "misaligned origins": dict(o=C.c_void_p(raw.inputs[0].data_ptr() + 2)),
        "misaligned dirs": dict(d=C.c_void_p(raw.inputs[1].data_ptr() + 1)),
        "misaligned rgba32": dict(rgba32=odd),
        "misaligned rgba8": dict(rgba8=C.c_void_p(raw.buf["rgba8"].data_ptr() + 2)),
        "misaligned steps": dict(steps=C.c_void_p(raw.buf["steps"].data_ptr() + 1)),
        "misaligned ids": dict(ids=C.c_void_p(raw.buf["ids"].data_ptr() + 3)),
    }
    for label, kw in cases.items():
        assert raw.call(good, OUTS, **kw) == abi.SR_E_INVALID, label
    assert raw.call(good, ()) == abi.SR_E_INVALID, "all outputs NULL"
    assert raw.call(None, OUTS) == abi.SR_E_INVALID, "null params"
    for label, prm in (("half width", tr.params(raytrace_type=2)), ("half height", tr.params(raytrace_type=3)),
                       ("raytrace_type 4", tr.params(raytrace_type=4)), ("max_steps < 0", tr.params(-1)),
                       ("max_steps above SR_MAX_STEPS", tr.params(1 << 24)), ("filter_mode", tr.params(filter_mode=7))):
        assert raw.call(prm, OUTS) == abi.SR_E_INVALID, label
    assert gpu.lib.sr_trace_rays(None, None, None, 0, C.byref(good), None, None, None, None, None) == abi.SR_E_INVALID
    assert raw.untouched()
    assert raw.call(good, OUTS, n=0) == abi.SR_OK
    assert raw.call(good, OUTS, n=0, o=C.c_void_p(0), d=C.c_void_p(0)) == abi.SR_OK
    assert raw.untouched()
    out = gpu.trace_rays(torch.empty((0, 3), device="cuda"), torch.empty((0, 3), device="cuda"), good, ids=True)
    assert out["rgba8"].shape == (0, 4) and out["ids"].shape == (0,)
    # a context without a scene: as sr_render
    r = pkg.Renderer(0)
    try:
        raw2 = Raw(r, n, offset=0)
        raw2.rays(O[:n], V[:n])
        assert raw2.call(good, OUTS) == abi.SR_E_NOT_READY
        out8 = torch.empty((4, 4, 4), dtype=torch.uint8, device="cuda")
        assert r.lib.sr_render(r.ctx, C.byref(tr.wd.cams["view"]), C.byref(good), 4, 4, 0, 4,
                               C.c_void_p(out8.data_ptr()), 16, r._stream(None)) == abi.SR_E_NOT_READY
        assert raw2.untouched()
    finally:
        r.close()
    # the context still works
    check(trace(gpu, O, V, good), tr.scattered_ref("default", False), "after the rejections")


# ---- the consumer ------------------------------------------------------------------------------------
def test_thin_lens_tool_with_no_aperture_is_the_plain_frame(gpu, tr, pkg):
    """tools/render.py's thin-lens path with R = 0 and K = 1: the plain render's bytes at 68x44;
    with an aperture the frame changes."""
    import torch

    spec = importlib.util.spec_from_file_location("sr_tools_render", ROOT / "tools" / "render.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    setup(gpu, tr, tr.wd.scene("small"), tr.wd.test_rays[False])
    cam, prm = pkg.abi.default_camera(), tr.params()
    plain = gpu.render(cam, prm, T.W, T.H)
    lens = tool.thin_lens_frame(pkg, gpu, cam, prm, T.W, T.H, 0.0, 5.0, 1)
    blur = tool.thin_lens_frame(pkg, gpu, cam, prm, T.W, T.H, 0.3, 5.0, 2)
    torch.cuda.synchronize()
    assert lens.shape == plain.shape == (T.H, T.W, 4) and lens.dtype == torch.uint8
    assert torch.equal(lens, plain)
    assert blur.shape == plain.shape and not torch.equal(blur, plain)
