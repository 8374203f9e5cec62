"""sr_reshade / sr_reshade_debug / sr_can_reshade on the GPU (sr.h "Retained
frames"): a launch of scene A, then sr_set_scene(B) with B = relit(A)
(shading-only fields, every one of them) and a background of another size,
then a reshade from the retained rays.

The reference of every comparison is the CPU oracle's frame of the CURRENT
scene and background (tests/reshade_cases.py Pairs, rendered once), and
nothing has a tolerance: RGBA8 bytes, float bits per channel with NaN = NaN
and step counts (test_gpu_shading_extremes.compare_strict). The supersampled
kinds are held to numpy's box rule on the oracle's sample frame.
tests/test_reshade_cases.py shows that every pair's frames differ on more
than 10 % of the pixels, so a reshade that did nothing cannot pass.

1. cells: the five of test_gpu_supersample at 17x11 / 300 steps and one at
   68x44 / 400; 2. resumed rays, three reshades in a row; 3. modes; 4. every
retained kind, into sentinel-filled buffers with a padded pitch and stride;
5. the shading-only pairs of tests/shading_cases.py; 6. what drops the
retained frame; 7. what brings it back; 8. streams and contexts; 9. argument
rejection on a live context.
"""
import ctypes as C

import numpy as np
import pytest

import reshade_cases as R
import shading_cases as S
from test_gpu_launch_matrix import host, reset, same
from test_gpu_shading_extremes import DIAG_ZERO, check_stores, compare_strict
from test_gpu_supersample import box_reference

pytestmark = pytest.mark.gpu

SENT = 0xA5
BR, LIST = 4, [2, -1, 0]  # block 2 holds the frame's last 3 rows
ROWS = (3, 9)


@pytest.fixture(scope="module")
def pairs(pkg, oracle, textures):
    return R.Pairs(pkg, oracle, textures)


def _renderer(pkg, textures):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    bg, arr = textures
    r = pkg.Renderer(0)
    r.set_background(bg)
    r.set_texture_array(arr)
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


def to_a(r, pairs, pair):
    r.set_scene(pairs.scene("A", pair["key"]))
    r.set_test_ray(pairs.wd.test_rays[pair["overlay"]])
    r.set_background(pairs.bg_a)


def to_b(r, pairs, pair):
    """The shading-only change: the retained frame outlives it."""
    r.set_scene(pairs.scene("B", pair["key"]))
    r.set_background(pairs.bg_b)


def restore(r, pairs):
    reset(r, pairs.wd)
    r.set_background(pairs.bg_a)


def debug_a(r, pairs, pair, cam="view", launches=1):
    """The A launch through render_debug, checked against the oracle's A."""
    for _ in range(launches):
        f, b, s = r.render_debug(pairs.wd.cams[cam], pairs.params(pair), pair["w"], pair["h"])
    f, b, s = host(f, b, s)
    compare_strict((b, f, s), pairs.frame("A", pair, cam), pair["id"] + ": the launch of A")


def reshade_debug(r):
    f, b, s = host(*r.reshade_debug())
    return b, f, s


def sentinel(n):
    import torch

    return torch.full((n,), SENT, dtype=torch.uint8, device="cuda")


def not_ready(pkg, r, label):
    """sr_can_reshade 0, sr_reshade and sr_pick_map SR_E_NOT_READY, nothing written."""
    abi = pkg.abi
    assert r.lib.sr_can_reshade(r.ctx) == 0, label
    buf = sentinel(4 * 17 * 11 * 4)
    assert r.lib.sr_reshade(r.ctx, C.c_void_p(buf.data_ptr()), 17 * 4, 17 * 4 * 11, None) == abi.SR_E_NOT_READY, label
    assert r.lib.sr_reshade_debug(r.ctx, None, C.c_void_p(buf.data_ptr()), None, None) == abi.SR_E_NOT_READY, label
    assert r.lib.sr_pick_map(r.ctx, C.c_void_p(buf.data_ptr()), 17 * 4, 17 * 4 * 11, None) == abi.SR_E_NOT_READY, label
    (got,) = host(buf)
    assert (got == SENT).all(), label + ": written to"


# ---- 1. cells
@pytest.mark.parametrize("pair", R.CELL_PAIRS, ids=[p["id"] for p in R.CELL_PAIRS])
def test_cell(pkg, gpu, gpu2, pairs, pair):
    cam, prm, w, h = pairs.wd.cams["view"], pairs.params(pair), pair["w"], pair["h"]
    try:
        to_a(gpu, pairs, pair)
        debug_a(gpu, pairs, pair)
        to_b(gpu, pairs, pair)
        assert gpu.can_reshade() and gpu.lib.sr_can_reshade(gpu.ctx) == 1
        want = pairs.frame("B", pair)
        compare_strict(reshade_debug(gpu), want, pair["id"] + ": sr_reshade_debug against the oracle of B")
        (got,) = host(gpu.reshade())
        same(got, want[0], pair["id"] + ": sr_reshade against the oracle of B")
        to_a(gpu2, pairs, pair)
        to_b(gpu2, pairs, pair)
        (fresh,) = host(gpu2.render(cam, prm, w, h))
        same(got, fresh, pair["id"] + ": sr_reshade against a fresh sr_render of B")
        assert gpu.diag_counters() == DIAG_ZERO and gpu2.diag_counters() == DIAG_ZERO
    finally:
        restore(gpu, pairs)
        restore(gpu2, pairs)


# ---- 2. resumed rays: the resume counter is reset by every reshade
def test_resumed_rays_three_times(pkg, gpu, pairs):
    pair = R.BY_ID["cell-stacked"]
    try:
        to_a(gpu, pairs, pair)
        debug_a(gpu, pairs, pair)
        to_b(gpu, pairs, pair)
        want = pairs.frame("B", pair)  # (every ray of this scene fills its hit log and is resumed)
        for k in range(3):
            compare_strict(reshade_debug(gpu), want, f"{pair['id']}: reshade {k + 1} of 3")
        (got,) = host(gpu.reshade())
        same(got, want[0], pair["id"] + ": sr_reshade after three")
        assert gpu.can_reshade()
        assert gpu.diag_counters() == DIAG_ZERO
    finally:
        restore(gpu, pairs)


# ---- 3. modes
MODES = [p["id"] for p in R.MODE_PAIRS] + ["latency", "cull-off", "split"]


@pytest.mark.parametrize("mode", MODES)
def test_mode(pkg, gpu, pairs, mode):
    pair = R.BY_ID.get(mode, R.BY_ID["cell-small-68x44"])
    try:
        to_a(gpu, pairs, pair)
        launches = 1
        if mode == "latency":
            gpu.set_latency_mode(True)
        elif mode == "cull-off":
            gpu.set_culling(False)
        elif mode == "split":
            gpu.set_split(4, 16, 1)
            launches = 2  # the second launch runs the split tiles the first one chose
        debug_a(gpu, pairs, pair, launches=launches)
        if mode == "split":
            codes = gpu.last_order()
            assert int(((codes >= 0) & ((codes & 0x80) != 0)).sum()) > 0, "no tile was split"
        # none of these matters to the retained frame
        gpu.set_latency_mode(mode != "latency")
        gpu.set_culling(mode != "cull-off")
        gpu.set_split(0 if mode == "split" else 4, 16, 1)
        to_b(gpu, pairs, pair)
        assert gpu.can_reshade()
        compare_strict(reshade_debug(gpu), pairs.frame("B", pair), f"{mode}: sr_reshade_debug against the oracle of B")
        assert gpu.diag_counters() == DIAG_ZERO
    finally:
        restore(gpu, pairs)


# ---- 4. every retained kind, into padded sentinel-filled buffers
def reshade_padded(r, frames, rows, w, label, pad=12, extra=40):
    """sr_reshade with pitch 4 w + pad and frame stride pitch rows + extra ->
    [frames, rows, w, 4]; every byte outside the rows' pixels stays SENT."""
    pitch = 4 * w + pad
    stride = pitch * rows + extra
    buf = sentinel(frames * stride + 16)
    rc = r.lib.sr_reshade(r.ctx, C.c_void_p(buf.data_ptr()), pitch, stride, r._stream(None))
    assert rc == 0, (label, rc)
    (a,) = host(buf)
    assert (a[frames * stride:] == SENT).all(), label + ": wrote past the last frame"
    a = a[:frames * stride].reshape(frames, stride)
    assert (a[:, pitch * rows:] == SENT).all(), label + ": wrote between the frames"
    a = a[:, :pitch * rows].reshape(frames, rows, pitch)
    assert (a[:, :, 4 * w:] == SENT).all(), label + ": wrote into the pitch padding"
    return np.ascontiguousarray(a[:, :, :4 * w]).reshape(frames, rows, w, 4)


def blocks_want(refs, blocks, br, h, w):
    """[frames, len(blocks) * br, w, 4]: SENT where the launch writes nothing."""
    want = np.full((len(refs), len(blocks) * br, w, 4), SENT, dtype=np.uint8)
    for f, rb in enumerate(refs):
        for s, b in enumerate(blocks):
            if b >= 0:
                n = min(br, h - b * br)
                want[f, s * br:s * br + n] = rb[b * br:b * br + n]
    return want


KINDS = ["rows", "blocks", "batch", "list", "phase", "ss2", "ss3", "list_ss"]


@pytest.mark.parametrize("kind", KINDS)
def test_kind(pkg, gpu, pairs, kind):
    pair = R.KIND_PAIR
    w, h, prm = pair["w"], pair["h"], pairs.params(pair)
    cams = pairs.wd.cam_array(R.BATCH)
    view = pairs.wd.cams["view"]

    def refs(which, ss=1, names=("view",)):
        return [pairs.resolved(which, pair, c, ss) for c in names]

    try:
        to_a(gpu, pairs, pair)
        y0, y1 = ROWS
        if kind == "rows":
            (a,) = host(gpu.render(view, prm, w, h, y0, y1))
            want_a, want_b = (np.stack([r[y0:y1] for r in refs(x)]) for x in "AB")
        elif kind == "blocks":
            out, rows = gpu.render_blocks(view, prm, w, h, BR, 0, 2, out=sentinel(2 * BR * w * 4).view(2 * BR, w, 4))
            (a,) = host(out)
            assert rows == 7
            want_a, want_b = (blocks_want(refs(x), [0, 2], BR, h, w) for x in "AB")
        elif kind == "batch":
            out, _ = gpu.render_blocks_batch(cams, prm, w, h, BR, 0, 2, out=sentinel(3 * 2 * BR * w * 4).view(3, 2 * BR, w, 4))
            (a,) = host(out)
            want_a, want_b = (blocks_want(refs(x, 1, R.BATCH), [0, 2], BR, h, w) for x in "AB")
        elif kind == "list":
            n = len(LIST) * BR
            (a,) = host(gpu.render_block_list(cams, prm, w, h, BR, LIST, out=sentinel(3 * n * w * 4).view(3, n, w, 4)))
            want_a, want_b = (blocks_want(refs(x, 1, R.BATCH), LIST, BR, h, w) for x in "AB")
        elif kind == "phase":
            (a,) = host(gpu.render_phase(view, prm, w, h, 2, 1, 0, y0, y1))
            want_a, want_b = (pairs.frame(x, pair, "view", 2)[0][0::2, 1::2][y0:y1][None] for x in "AB")
        elif kind in ("ss2", "ss3"):
            ss = int(kind[2])
            (a,) = host(gpu.render_ss(view, prm, w, h, ss, y0, y1))
            want_a, want_b = (np.stack([r[y0:y1] for r in refs(x, ss)]) for x in "AB")
        else:
            n = len(LIST) * BR
            (a,) = host(gpu.render_block_list_ss(cams, prm, w, h, BR, LIST, 2, out=sentinel(3 * n * w * 4).view(3, n, w, 4)))
            want_a, want_b = (blocks_want(refs(x, 2, R.BATCH), LIST, BR, h, w) for x in "AB")
        same(a.reshape(want_a.shape), want_a, f"{kind}: the launch of A")
        to_b(gpu, pairs, pair)
        assert gpu.can_reshade()
        frames, rows = want_b.shape[0], want_b.shape[1]
        got = reshade_padded(gpu, frames, rows, w, kind)
        same(got, want_b, f"{kind}: sr_reshade against the oracle of B")
        (dense,) = host(gpu.reshade(out=sentinel(want_b.size).view(want_b.shape if frames > 1 else want_b.shape[1:])))
        same(dense.reshape(want_b.shape), want_b, f"{kind}: Renderer.reshade")
        assert gpu.can_reshade()
        assert gpu.diag_counters() == DIAG_ZERO
    finally:
        restore(gpu, pairs)


# ---- 5. the shading-only pairs of tests/shading_cases.py, in a chain
@pytest.fixture(scope="module")
def gpu_std(pkg):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    r = pkg.Renderer(0)
    r.set_test_ray(pkg.abi.default_test_ray())
    r.set_texture_array(S.textures_of(pkg, "std")[1])
    yield r
    r.close()


@pytest.mark.parametrize("names", R.SHADING_PAIRS, ids=[f"{a}->{b}" for a, b in R.SHADING_PAIRS])
def test_shading_extremes(pkg, gpu_std, pairs, names):
    a, b = (S.BY_NAME[n] for n in names)
    r = gpu_std
    r.set_scene(S.build(pkg, a))
    r.set_background(pairs.shading_tex("A")[0])
    f, b8, s = host(*r.render_debug(S.camera_of(pkg, a), S.params_of(pkg, a), S.W, S.H))
    compare_strict((b8, f, s), pairs.shading_frame("A", names[0]), names[0] + ": the launch of A")
    r.set_scene(S.build(pkg, b))
    r.set_background(pairs.shading_tex("B")[0])
    assert r.can_reshade()
    got = reshade_debug(r)
    compare_strict(got, pairs.shading_frame("B", names[1]), f"{names[0]} -> {names[1]}: sr_reshade_debug")
    check_stores(got, names[1])
    assert r.diag_counters() == DIAG_ZERO


# ---- 6. what drops the retained frame, 7. and a fresh launch brings it back
def _geometry(field):
    def change(pkg, r, pairs, pair):
        sc = pkg.scenes
        s = sc.struct_from_bytes(pkg.abi.Scene, sc.struct_bytes(pairs.scene("A", pair["key"])))
        field(s)
        assert not pkg.abi.scene_shading_only(pairs.scene("A", pair["key"]), s)
        r.set_scene(s)
    return change


def _mat(name, value):
    def f(s):
        m = s.materials[int(s.objects[0].material_index)]
        if name == "alpha":
            m.color[3] = value
        else:
            setattr(m, name, value if getattr(m, name) != value else value + 1)
    return f


def _obj_pos(s):
    s.spheres[0].transform.pos[0] += 0.5
    s.boxes[0].transform.pos[0] += 0.5
    s.rectangles[0].plane.transform.pos[0] += 0.5


def _radius(s):
    s.spheres[0].radius += 0.25
    s.disks[0].radius += 0.25
    s.cylinders[0].radius += 0.25


def _tex_sizes(s):
    s.texture_sizes[0][0] += 1.0


def _fewer(s):
    s.num_objects -= 1


def _view(pairs, pair):
    return pairs.wd.cams["view"], pairs.params(pair), pair["w"], pair["h"]


DROPS = {
    "transform": _geometry(_obj_pos),
    "radius": _geometry(_radius),
    "color3": _geometry(_mat("alpha", 0.5)),
    "texture_index": _geometry(_mat("texture_index", 1)),
    "invert_uv_x": _geometry(_mat("invert_uv_x", 1)),
    "invert_uv_y": _geometry(_mat("invert_uv_y", 1)),
    "swap_uvs": _geometry(_mat("swap_uvs", 1)),
    "double_sided_normals": _geometry(_mat("double_sided_normals", 0)),
    "flip_normals": _geometry(_mat("flip_normals", 1)),
    "texture_sizes": _geometry(_tex_sizes),
    "num_objects": _geometry(_fewer),
    "set_texture_array": lambda pkg, r, pairs, pair: r.set_texture_array(pairs.arr),
    "set_test_ray": lambda pkg, r, pairs, pair: r.set_test_ray(pairs.wd.test_rays[False]),
    "render_adaptive": lambda pkg, r, pairs, pair: r.render_adaptive(*_view(pairs, pair), 2, 8),
    "render_adaptive_255": lambda pkg, r, pairs, pair: r.render_adaptive(*_view(pairs, pair), 2, 255),
    "render_accumulate": lambda pkg, r, pairs, pair: r.render_accumulate(*_view(pairs, pair), 2, [(0, 0), (1, 1)]),
    "wave_costs": lambda pkg, r, pairs, pair: r.wave_costs(*_view(pairs, pair)),
    "zero_rows": lambda pkg, r, pairs, pair: r.render(*_view(pairs, pair), 3, 3, out=sentinel(64)),
}


def test_not_ready_before_the_first_launch(pkg, textures, pairs):
    r = _renderer(pkg, textures)
    try:
        not_ready(pkg, r, "a new context")
        r.set_scene(pairs.scene("A", "small"))
        not_ready(pkg, r, "a scene, no launch")
    finally:
        r.close()


@pytest.mark.parametrize("drop", sorted(DROPS))
def test_invalidation_and_regaining(pkg, gpu, pairs, drop):
    pair = R.BY_ID["cell-small"]
    cam, prm, w, h = _view(pairs, pair)
    try:
        to_a(gpu, pairs, pair)
        gpu.render(cam, prm, w, h)
        assert gpu.can_reshade()
        DROPS[drop](pkg, gpu, pairs, pair)
        not_ready(pkg, gpu, drop)
        # 7. a fresh launch of whatever the context holds now is retained again
        (fresh,) = host(gpu.render(cam, prm, w, h))
        assert gpu.can_reshade(), drop
        (again,) = host(gpu.reshade())
        same(again, fresh, drop + ": sr_reshade after a fresh sr_render")
        assert gpu.diag_counters() == DIAG_ZERO
    finally:
        restore(gpu, pairs)


# ---- 8. streams and contexts
def test_other_stream_without_host_sync(pkg, gpu, pairs):
    import torch

    pair = R.BY_ID["cell-small-68x44"]
    cam, prm, w, h = _view(pairs, pair)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        to_a(gpu, pairs, pair)
        to_b(gpu, pairs, pair)
        torch.cuda.synchronize()
        first = gpu.render(cam, prm, w, h, stream=s1)
        second = gpu.reshade(stream=s2)  # ordered after the launch by the context, not by the host
        third = gpu.render(cam, prm, w, h, stream=s1)
        fourth = gpu.reshade(stream=s2)
        first, second, third, fourth = host(first, second, third, fourth)
        want = pairs.frame("B", pair)[0]
        for k, got in enumerate((first, second, third, fourth)):
            same(got, want, f"launch {k} of render / reshade on two streams")
    finally:
        restore(gpu, pairs)


def test_two_contexts_interleaved(pkg, gpu, gpu2, pairs):
    p1, p2 = R.BY_ID["cell-small"], R.BY_ID["cell-large"]
    try:
        to_a(gpu, pairs, p1)
        to_a(gpu2, pairs, p2)
        gpu.render(*_view(pairs, p1))
        gpu2.render(*_view(pairs, p2))
        to_b(gpu, pairs, p1)
        to_b(gpu2, pairs, p2)
        outs = [gpu.reshade(), gpu2.reshade(), gpu.reshade()]
        outs.append(gpu2.render(*_view(pairs, p2)))
        outs.append(gpu.reshade())
        outs.append(gpu2.reshade())
        outs = host(*outs)
        for k, (got, p) in enumerate(zip(outs, (p1, p2, p1, p2, p1, p2))):
            same(got, pairs.frame("B", p)[0], f"interleaved launch {k} ({p['id']})")
        assert gpu.diag_counters() == DIAG_ZERO and gpu2.diag_counters() == DIAG_ZERO
    finally:
        restore(gpu, pairs)
        restore(gpu2, pairs)


def test_other_paths_before_a_new_launch(pkg, gpu, pairs):
    """Whatever ran before, the retained frame is the last launch's."""
    pair = R.KIND_PAIR
    _, prm, w, h = _view(pairs, pair)
    try:
        to_a(gpu, pairs, pair)
        view = pairs.wd.cams["view"]
        gpu.render(view, prm, w, h)
        gpu.wave_costs(view, prm, w, h)
        gpu.render_adaptive(view, prm, w, h, 2, 8)
        gpu.render_ss(view, prm, w, h, 3)
        gpu.render_block_list(pairs.wd.cam_array(R.BATCH), prm, w, h, BR, LIST)
        (a,) = host(gpu.render(pairs.wd.cams["fly1"], prm, w, h))
        same(a, pairs.frame("A", pair, "fly1")[0], "the new launch of A")
        to_b(gpu, pairs, pair)
        compare_strict(reshade_debug(gpu), pairs.frame("B", pair, "fly1"), "sr_reshade_debug of the new launch")
        assert gpu.diag_counters() == DIAG_ZERO
    finally:
        restore(gpu, pairs)


# ---- 9. argument rejection on a live context
def test_rejections(pkg, gpu, pairs):
    abi, lib = pkg.abi, gpu.lib
    pair = R.KIND_PAIR
    cam, prm, w, h = _view(pairs, pair)
    INV = abi.SR_E_INVALID
    try:
        to_a(gpu, pairs, pair)
        buf = sentinel(3 * 16 * w * 4 * 4)
        p = C.c_void_p(buf.data_ptr())
        assert lib.sr_reshade(None, p, 4 * w, 0, None) == INV and lib.sr_can_reshade(None) == 0
        gpu.render(cam, prm, w, h)
        assert lib.sr_reshade(gpu.ctx, None, 4 * w, 0, None) == INV
        assert lib.sr_reshade(gpu.ctx, p, 4 * w - 1, 0, None) == INV
        assert lib.sr_reshade_debug(gpu.ctx, None, None, None, None) == INV
        assert lib.sr_reshade(gpu.ctx, p, 4 * w, 0, None) == abi.SR_OK  # one frame: the stride is not read
        buf.fill_(SENT)
        n = len(LIST) * BR
        gpu.render_block_list(pairs.wd.cam_array(R.BATCH), prm, w, h, BR, LIST)
        assert lib.sr_reshade(gpu.ctx, p, 4 * w, 4 * w * n - 1, None) == INV  # a short stride
        assert lib.sr_reshade(gpu.ctx, p, 4 * w + 4, 4 * w * n, None) == INV  # short for this pitch
        assert lib.sr_reshade(gpu.ctx, p, 4 * w - 4, 4 * w * n, None) == INV
        assert lib.sr_reshade_debug(gpu.ctx, None, p, None, None) == INV  # a batch
        gpu.render_ss(cam, prm, w, h, 2)
        assert lib.sr_reshade_debug(gpu.ctx, None, p, None, None) == INV  # supersampled
        assert lib.sr_reshade(gpu.ctx, p, 4 * w - 1, 0, None) == INV
        assert lib.sr_pick_map(gpu.ctx, p, 4 * w, 0, None) == abi.SR_E_NOT_READY
        (got,) = host(buf)
        assert (got == SENT).all(), "a rejected call wrote"
        assert gpu.can_reshade()  # a rejected call leaves the retained frame alone
        (ok,) = host(gpu.reshade())
        same(ok, box_reference(pairs.frame("A", pair, "view", 2)[0], 2), "sr_reshade after the rejections")
    finally:
        restore(gpu, pairs)
