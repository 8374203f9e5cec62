"""sr_set_projection on the GPU: every launch path under the equirectangular and
the fisheye projection against the unchanged oracle, one pixel at a time
(tests/projection_cases.py), with no tolerance: RGBA8 bytes always, float
FragColor bits (NaN == NaN) and step counts wherever the path returns them.

A. Frames: the cases of projection_cases.CELLS through sr_render_debug, two
   launches in a row (the second runs the order the first learned).
B. Launch paths on the 68x44 frames: row bands, culling off, the latency
   mode, split tiles; a three-camera batch and a padded block list at 33x17.
C. Supersampling, phases, accumulation and the adaptive launch.
D. What hangs on uv: split modes, the noise mask, the crosshair.
E. Retained frames: reshade, pick, a changed projection.
F. Wave costs, two ranks' priced lists, switching back, arguments.
"""
import ctypes as C

import numpy as np
import pytest

import pick_cases as K
import projection_cases as P
from test_gpu_launch_matrix import FILL, block_rows_of, host, same, split_count
from test_gpu_parity import compare

pytestmark = pytest.mark.gpu

PROJ = [P.EQUIRECT, P.FISHEYE]
PROJ_IDS = [P.NAMES[p] for p in PROJ]
W, H, FOV = 68, 44, 120.0  # the frames of section B (projection_cases.BIG)
BATCH = ("view", "fly1", "fly5")


@pytest.fixture(scope="module")
def pj(pkg, oracle, textures):
    return P.Projected(pkg, oracle, textures)


def _renderer(pkg, textures):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    r = pkg.Renderer(0)
    r.set_background(textures[0])
    r.set_texture_array(textures[1])
    return r


@pytest.fixture(scope="module")
def gpu(pkg, textures):
    r = _renderer(pkg, textures)
    yield r
    r.close()


@pytest.fixture(scope="module")
def gpu2(pkg, textures):
    r = _renderer(pkg, textures)
    yield r
    r.close()


@pytest.fixture(autouse=True)
def _state(gpu, gpu2, pj, textures):
    """Every test starts from, and leaves, the default context state."""
    yield
    for r in (gpu, gpu2):
        r.set_projection(P.RECTILINEAR)
        r.set_split(0)
        r.set_latency_mode(False)
        r.set_culling(True)
        r.set_test_ray(pj.wd.test_rays[False])
        r.set_background(textures[0])


def use(r, pj, key, overlay, projection):
    r.set_scene(pj.wd.scene(key))
    r.set_test_ray(pj.wd.test_rays[overlay])
    r.set_projection(projection)
    assert r.get_projection() == projection


def debug(r, cam, prm, w, h, y0=0, y1=None):
    f, b, s = host(*r.render_debug(cam, prm, w, h, y0, y1))
    return b, f, s


# ---- A. frames ----------------------------------------------------------------------
FRAMES = [(key, ov, cid) for (key, ov), ids in P.CELLS.items() for cid in ids]


@pytest.mark.parametrize("key,overlay,cid", FRAMES,
                         ids=[f"{k}-{'overlay' if o else 'plain'}-{c}" for k, o, c in FRAMES])
def test_frames(gpu, pj, key, overlay, cid):
    _, projection, w, h, fov = P.BY_ID[cid]
    use(gpu, pj, key, overlay, projection)
    cam, prm = pj.cam("view", fov), pj.params()
    ref = pj.case_ref(key, overlay, cid)
    for launch in range(2):
        compare(debug(gpu, cam, prm, w, h), ref, f"{key}, overlay {overlay}, {cid}, launch {launch}")
    if cid == "fisheye-48x48-fov360":
        ray = P.local_dirs(projection, fov, w, h)[1]
        assert int((~ray).sum()) == 500 and not ref[2][~ray].any()


# ---- B. launch paths ------------------------------------------------------------------
def big_ref(pj, key, projection):
    return pj.ref(key, False, projection, W, H, FOV)


@pytest.mark.parametrize("path", ["rows", "cull_off", "latency", "split4x4", "split16x64"])
@pytest.mark.parametrize("projection", PROJ, ids=PROJ_IDS)
@pytest.mark.parametrize("key", ["small", "large"])
def test_paths(gpu, pj, key, projection, path):
    use(gpu, pj, key, False, projection)
    cam, prm = pj.cam("view", FOV), pj.params()
    rb, rf, rs = big_ref(pj, key, projection)
    label = f"{key}, {P.NAMES[projection]}, {path}"
    if path == "rows":
        for y0, y1 in ((5, 6), (7, 25), (40, H)):
            (got,) = host(gpu.render(cam, prm, W, H, y0, y1))
            same(got, rb[y0:y1], f"{label} [{y0}, {y1})")
        compare(debug(gpu, cam, prm, W, H, 7, 25), (rb[7:25], rf[7:25], rs[7:25]), f"{label}, debug [7, 25)")
        return
    if path == "cull_off":
        gpu.set_culling(False)
    elif path == "latency":
        gpu.set_latency_mode(True)
    elif path == "split4x4":
        gpu.set_split(4, 4, 1)
    elif path == "split16x64":
        gpu.set_split(64, 16, 1)
    for launch in range(2):
        out = debug(gpu, cam, prm, W, H)
        if launch == 0 and path.startswith("split"):
            assert split_count(gpu) > 0, f"{label}: no tile was split"
        compare(out, (rb, rf, rs), f"{label}, launch {launch}")


LIST = [2, -1, 0, 1, -1]  # block 2 holds the 33x17 frame's last row


@pytest.mark.parametrize("projection", PROJ, ids=PROJ_IDS)
@pytest.mark.parametrize("key", ["small", "large"])
def test_batch_and_block_list(gpu, pj, key, projection):
    import torch

    w, h = 33, 17
    use(gpu, pj, key, False, projection)
    cams, prm = [pj.cam(n) for n in BATCH], pj.params()
    refs = [pj.ref(key, False, projection, w, h, cam=n)[0] for n in BATCH]
    assert not np.array_equal(refs[0], refs[1]) and not np.array_equal(refs[1], refs[2])
    label = f"{key}, {P.NAMES[projection]}"
    for first, step in ((0, 1), (1, 2)):
        nb = len(range(first, 3, step))
        out = torch.full((3, nb * 8, w, 4), FILL, dtype=torch.uint8, device="cuda")
        for _ in range(2):
            _, rows = gpu.render_blocks_batch(cams, prm, w, h, 8, first, step, out=out)
        (got,) = host(out)
        for f, name in enumerate(BATCH):
            want = block_rows_of(refs[f], first, step, h)
            assert rows == len(want)
            same(got[f, :rows], want, f"{label}, batch ({first}, {step}) frame {name}")
            assert (got[f, rows:] == FILL).all()
    out = torch.full((3, len(LIST) * 8, w, 4), FILL, dtype=torch.uint8, device="cuda")
    for _ in range(2):
        gpu.render_block_list(cams, prm, w, h, 8, LIST, out=out)
    (got,) = host(out)
    for f, name in enumerate(BATCH):
        want = np.full((len(LIST) * 8, w, 4), FILL, dtype=np.uint8)
        for s, b in enumerate(LIST):
            if b >= 0:
                n = min(8, h - b * 8)
                want[s * 8:s * 8 + n] = refs[f][b * 8:b * 8 + n]
        same(got[f], want, f"{label}, block list frame {name}")


# ---- C. supersampling and phases --------------------------------------------------------
@pytest.mark.parametrize("projection", PROJ, ids=PROJ_IDS)
def test_supersampling_and_phases(gpu, pj, projection):
    w, h = 17, 11
    use(gpu, pj, "small", False, projection)
    cam, prm = pj.cam("view"), pj.params()
    label = P.NAMES[projection]
    resolved = {}
    for ss in (2, 3):
        samples = pj.ref("small", False, projection, ss * w, ss * h)[0]
        resolved[ss] = P.box_average(samples, ss)
        (got,) = host(gpu.render_ss(cam, prm, w, h, ss))
        same(got, resolved[ss], f"{label}, render_ss {ss}")
    samples = pj.ref("small", False, projection, 2 * w, 2 * h)[0]
    phases = [(x, y) for y in range(2) for x in range(2)]
    for x, y in phases:
        (got,) = host(gpu.render_phase(cam, prm, w, h, 2, x, y))
        same(got, samples[y::2, x::2], f"{label}, phase ({x}, {y})")
    (band,) = host(gpu.render_phase(cam, prm, w, h, 2, 1, 0, 3, 9))
    same(band, samples[0::2, 1::2][3:9], f"{label}, phase (1, 0) rows [3, 9)")
    acc = gpu.render_accumulate(cam, prm, w, h, 2, phases[:3])
    acc = gpu.render_accumulate(cam, prm, w, h, 2, phases[3:], accum=acc)
    (got,) = host(gpu.accum_resolve(acc, 4))
    same(got, resolved[2], f"{label}, accumulate")
    plain = pj.ref("small", False, projection, w, h)[0]
    frame, mask = host(*gpu.render_adaptive(cam, prm, w, h, 2, -1))
    assert mask.all()
    same(frame, resolved[2], f"{label}, adaptive, every tile")
    frame, mask = host(*gpu.render_adaptive(cam, prm, w, h, 2, 255))
    assert not mask.any()
    same(frame, plain, f"{label}, adaptive, no tile")
    (got,) = host(gpu.render(cam, prm, w, h))
    same(got, plain, f"{label}, render")


# ---- D. what hangs on uv ------------------------------------------------------------------
@pytest.mark.parametrize("mode", [dict(raytrace_type=P.HALF_WIDTH, curved_percentage=0.4),
                                  dict(raytrace_type=P.HALF_HEIGHT, curved_percentage=0.6),
                                  dict(raytrace_type=P.FLAT)], ids=["half-width", "half-height", "flat"])
@pytest.mark.parametrize("projection", PROJ, ids=PROJ_IDS)
def test_split_modes(gpu, pj, projection, mode):
    w, h = 33, 17
    use(gpu, pj, "small", False, projection)
    ref = pj.ref("small", False, projection, w, h, **mode)
    flat = P.flat_mask(pj.params(**mode), w, h)
    assert flat.any() and (ref[2][flat] == 0).all() and (mode["raytrace_type"] == P.FLAT or (ref[2][~flat] > 0).any())
    compare(debug(gpu, pj.cam("view"), pj.params(**mode), w, h), ref, f"{P.NAMES[projection]}, {mode}")


@pytest.mark.parametrize("projection", PROJ, ids=PROJ_IDS)
def test_noise_mask(gpu, pj, projection):
    """The mask is a function of uvv alone: the masked set is the rectilinear
    oracle frame's (0 steps with the mask on, some with it off). An even
    frame: no pixel looks straight at the hole, so no frame has a radial
    (flat, 0-step) pixel that the mask would not reach."""
    w, h = 34, 22
    use(gpu, pj, "small", False, projection)
    cam = pj.cam("view")
    scene, tr = pj.wd.scene("small"), pj.wd.test_rays[False]
    on = pj.oracle.render(scene, cam, pj.params(percent_black=0.4), w, h, pj.tex, tr)[2]
    off = pj.oracle.render(scene, cam, pj.params(), w, h, pj.tex, tr)[2]
    assert (off > 0).all()
    masked = on == 0
    assert 0.2 < masked.mean() < 0.6
    rb, rf, rs = pj.ref("small", False, projection, w, h)
    assert (rs > 0).all()
    want = (np.where(masked[..., None], 0, rb).astype(np.uint8), np.where(masked[..., None], 0, rf).astype(np.float32),
            np.where(masked, 0, rs).astype(np.int32))
    compare(debug(gpu, cam, pj.params(percent_black=0.4), w, h), want, f"{P.NAMES[projection]}, noise mask")


@pytest.mark.parametrize("projection", PROJ, ids=PROJ_IDS)
def test_crosshair(gpu, pj, projection):
    """The crosshair changes exactly the pixels it changes in the rectilinear frame of that size."""
    w, h = 36, 36
    use(gpu, pj, "small", False, projection)
    cam = pj.cam("view")
    scene, tr = pj.wd.scene("small"), pj.wd.test_rays[False]
    on = pj.oracle.render(scene, cam, pj.params(crosshair=1), w, h, pj.tex, tr)[1]
    off = pj.oracle.render(scene, cam, pj.params(), w, h, pj.tex, tr)[1]
    assert not np.isnan(on).any() and not np.isnan(off).any()
    changed = (on != off).any(-1)
    assert changed.sum() == 4 * 2 * 10  # four arms, two pixels wide, |d| = 5.5 .. 14.5
    rb, rf, rs = pj.ref("small", False, projection, w, h)
    assert not np.isnan(rf).any()
    b, f, s = debug(gpu, cam, pj.params(crosshair=1), w, h)
    assert np.array_equal((f != rf).any(-1), changed), f"{P.NAMES[projection]}: the crosshair's pixels moved"
    assert np.array_equal(s, rs) and np.array_equal(b[~changed], rb[~changed])
    assert (f[changed] >= 0.5).all()  # the crosshair's grey under whatever the ray adds


# ---- E. retained frames ---------------------------------------------------------------------
def relit(pkg, scene):
    """A shading-only change: other light colours, every material's rgb and Phong terms."""
    s = P.copy_struct(pkg, pkg.abi.Scene, scene)
    for i in range(int(s.num_lights)):
        s.lights[i].color[0], s.lights[i].color[1], s.lights[i].color[2] = 0.25, 1.0, 0.5
    for m in s.materials:
        m.color[0], m.color[1], m.color[2] = m.color[2], m.color[0], 0.75
        m.ambient, m.diffuse = 0.5, 0.25
    assert pkg.abi.load().sr_scene_shading_only(C.byref(scene), C.byref(s)) == 1
    return s


@pytest.mark.parametrize("projection", PROJ, ids=PROJ_IDS)
def test_reshade_after_a_projected_launch(pkg, gpu, pj, projection):
    w, h = 33, 17
    use(gpu, pj, "small", False, projection)
    cam, prm = pj.cam("view"), pj.params()
    compare(debug(gpu, cam, prm, w, h), pj.ref("small", False, projection, w, h), "the launch")
    new = relit(pkg, pj.wd.scene("small"))
    gpu.set_scene(new)
    assert gpu.can_reshade()
    gpu.set_projection(projection)  # the same value keeps the frame
    assert gpu.can_reshade()
    want = pj.ref("small", False, projection, w, h, scene=new, tag="relit")
    assert not np.array_equal(want[0], pj.ref("small", False, projection, w, h)[0])
    f, b, s = host(*gpu.reshade_debug())
    compare((b, f, s), want, f"{P.NAMES[projection]}, reshade_debug")
    (got,) = host(gpu.reshade())
    same(got, want[0], f"{P.NAMES[projection]}, reshade")
    assert gpu.diag_counters()["hit_not_opaque"] == 0


@pytest.mark.parametrize("cid", ["equirect-64x32-fov360", "fisheye-48x48-fov360"])
def test_pick_map(pkg, oracle, textures, gpu2, pj, cid):
    """The object-code scene of tests/pick_cases.py through the per-pixel
    method: the decoded oracle frame is the pick map; SR_PICK_NONE without a ray."""
    import torch

    _, projection, w, h, fov = P.BY_ID[cid]
    scene = pj.wd.scene("small")
    (coded,) = K.recoloured(pkg, scene)
    tex = oracle.TextureSet(K.sky_texel(), textures[1])
    ref = pj.ref("small", False, projection, w, h, fov, scene=coded, tex=tex, tag="codes")
    codes, ok = K.decode([ref[1]], int(scene.num_objects))
    assert ok.all()
    ray = P.local_dirs(projection, fov, w, h)[1]
    assert (codes[~ray] == K.NONE).all() and (codes[ray] != K.NONE).all()
    assert {K.SKY, K.HOLE} <= set(codes.ravel().tolist()) and (codes >= 0).any()
    gpu2.set_scene(coded)
    gpu2.set_background(K.sky_texel())
    gpu2.set_projection(projection)
    compare(debug(gpu2, pj.cam("view", fov), pj.params(), w, h), ref, f"{cid}, the coded frame")
    (got,) = host(gpu2.pick_map())
    assert np.array_equal(got, codes), f"{cid}: {int((got != codes).sum())} of {codes.size} codes differ"
    # a changed projection: the retained frame is gone, nothing is written
    gpu2.set_projection(P.RECTILINEAR)
    assert not gpu2.can_reshade()
    buf = torch.full((h, w), 77, dtype=torch.int32, device="cuda")
    abi = pkg.abi
    assert gpu2.lib.sr_pick_map(gpu2.ctx, C.c_void_p(buf.data_ptr()), w * 4, 0, None) == abi.SR_E_NOT_READY
    assert gpu2.lib.sr_reshade(gpu2.ctx, C.c_void_p(buf.data_ptr()), w * 4, 0, None) == abi.SR_E_NOT_READY
    assert gpu2.lib.sr_reshade_debug(gpu2.ctx, None, C.c_void_p(buf.data_ptr()), None, None) == abi.SR_E_NOT_READY
    torch.cuda.synchronize()
    assert (buf == 77).all()
    gpu2.set_projection(projection)  # setting it back does not bring the frame back
    assert not gpu2.can_reshade()
    assert gpu2.diag_counters()["hit_not_opaque"] == 0


# ---- F. wave costs, ranks, switching back, arguments ---------------------------------------------
@pytest.mark.parametrize("projection", PROJ, ids=PROJ_IDS)
def test_wave_costs(pkg, gpu, pj, projection):
    """Every surface of the untextured default scene is opaque (alpha 1, double
    sided): a ray stops at its first hit in the step loop as in the shader, no
    ray is resumed, and a wave's cost is its longest reference ray."""
    scene = pkg.scenes.scene_default(False)
    used = {int(o.material_index) for o in scene.objects[:scene.num_objects]}
    assert all(scene.materials[m].color[3] == 1.0 and scene.materials[m].texture_index < 0 for m in used)
    gpu.set_scene(scene)
    gpu.set_projection(projection)
    cam, prm = pj.cam("view", FOV), pj.params()
    rs = pj.ref("untextured", False, projection, W, H, FOV, scene=scene, tag="untextured")[2]
    (a,) = host(gpu.wave_costs(cam, prm, W, H))
    assert a.shape == ((H + 7) // 8, (W + 7) // 8, 2)
    pad = np.zeros((a.shape[0] * 8, a.shape[1] * 8), dtype=np.int64)
    pad[:H, :W] = rs
    mx = pad.reshape(a.shape[0], 8, a.shape[1], 8).max(axis=(1, 3))
    assert np.array_equal(a[..., 0], mx), f"{int((a[..., 0] != mx).sum())} of {mx.size} waves differ"
    # not the pinhole's costs
    gpu.set_projection(P.RECTILINEAR)
    (r,) = host(gpu.wave_costs(cam, prm, W, H))
    assert not np.array_equal(r[..., 0], a[..., 0])


def test_two_ranks_priced_lists(pkg, gpu, gpu2, pj):
    import torch

    D = pkg.dist
    for r in (gpu, gpu2):
        use(r, pj, "small", False, P.EQUIRECT)
    cam, prm = pj.cam("view", FOV), pj.params()
    lists = D.balanced_blocks(D.block_costs(gpu.wave_costs(cam, prm, W, H)), 2)
    assert sorted(b for l in lists for b in l if b >= 0) == list(range((H + 7) // 8))
    tiles = []
    for r, lst in zip((gpu, gpu2), lists):
        for _ in range(2):  # the second launch runs the list's learned order
            t = r.render_block_list([cam], prm, W, H, 8, lst)
        tiles.append(t)
    (frame,) = host(D.assemble_blocks_abi(torch.stack(tiles), lists, H, 8))
    same(frame[0], big_ref(pj, "small", P.EQUIRECT)[0], "two ranks, reassembled on the device")


def test_switching_back(pkg, textures, gpu, pj):
    """After a panorama the pinhole's frames are a fresh context's, byte for
    byte (and the oracle's): no order, no retained state leaks."""
    use(gpu, pj, "small", False, P.EQUIRECT)
    cam, prm = pj.cam("view", FOV), pj.params()
    for _ in range(2):
        gpu.render(cam, prm, W, H)
    gpu.set_projection(P.FISHEYE)
    gpu.render(cam, prm, W, H)
    gpu.set_projection(P.RECTILINEAR)
    assert gpu.get_projection() == P.RECTILINEAR
    fresh = _renderer(pkg, textures)
    try:
        fresh.set_scene(pj.wd.scene("small"))
        assert fresh.get_projection() == P.RECTILINEAR
        want = debug(fresh, cam, prm, W, H)
        for launch in range(2):
            b, f, s = debug(gpu, cam, prm, W, H)
            assert b.tobytes() == want[0].tobytes() and f.tobytes() == want[1].tobytes() and s.tobytes() == want[2].tobytes()
    finally:
        fresh.close()
    ora = pj.oracle.render(pj.wd.scene("small"), cam, prm, W, H, pj.tex, pj.wd.test_rays[False])
    compare(want, ora, "the pinhole after the panoramas")


def test_arguments_rejected_on_a_live_context(pkg, gpu, pj):
    abi = pkg.abi
    use(gpu, pj, "small", False, P.FISHEYE)
    gpu.render(pj.cam("view"), pj.params(), 17, 11)
    assert gpu.can_reshade()
    for bad in (-1, 3, 1 << 20):
        assert gpu.lib.sr_set_projection(gpu.ctx, bad) == abi.SR_E_INVALID
        assert gpu.get_projection() == P.FISHEYE and gpu.can_reshade()
    with pytest.raises(ValueError):
        gpu.set_projection("cubemap")
    with pytest.raises(abi.SRError):
        gpu.set_projection(5)
    gpu.set_projection("equirect")
    assert gpu.get_projection() == P.EQUIRECT and not gpu.can_reshade()
    assert gpu.lib.sr_set_projection(None, 0) == abi.SR_E_INVALID and gpu.lib.sr_get_projection(None) == abi.SR_E_INVALID


def test_zz_diag_counters_zero(gpu, gpu2):
    for r in (gpu, gpu2):
        d = r.diag_counters()
        assert d["hit_not_opaque"] == 0 and d["free_errors"] == 0
