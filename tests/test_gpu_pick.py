"""sr_pick_map on the GPU (sr.h "Retained frames"): the code of the first
surface on every pixel's ray, from the retained rays.

The reference is the decode of the CPU oracle's frames of the picking scenes
(tests/pick_cases.py: every object an unlit colour of its own, so the frame
says which surface came first), every pixel, no tolerance.
tests/test_pick_cases.py shows on the oracle alone that every pixel decodes
to exactly one code and that each code a case claims is on at least 1 % of a
frame. The map does not depend on colours: the context holds pass 0 of a
scene with more than nine objects, the reference is decoded from all passes.
"""
import ctypes as C

import numpy as np
import pytest

import pick_cases as P
import reshade_cases as R
from test_gpu_launch_matrix import host, reset

pytestmark = pytest.mark.gpu

SENT = -77
BR, LIST = 4, [2, -1, 0]


@pytest.fixture(scope="module")
def picks(pkg, oracle, textures):
    return P.Picks(pkg, oracle, textures)


@pytest.fixture(scope="module")
def gpu(pkg, picks):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    r = pkg.Renderer(0)
    r.set_background(picks.bg)
    r.set_texture_array(picks.arr)
    yield r
    r.close()


def setup(r, picks, case):
    r.set_scene(picks.passes(case)[0])
    r.set_test_ray(picks.test_rays[case["overlay"]])


def equal(got, want, label):
    assert got.shape == want.shape, (label, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), (f"{label}: {int(bad.sum())} of {bad.size} codes differ, first (y, x, got, want) "
                           f"{[(int(y), int(x), int(got[y, x]), int(want[y, x])) for y, x in np.argwhere(bad)[:6]]}")


CASES = ["stress", "default", "flat", "half-width", "overlay", "noise", "translucent-front", "single-sided-behind",
         "single-sided-behind-flat"]


@pytest.mark.parametrize("name", CASES)
def test_pick_map_equals_the_decoded_oracle(pkg, gpu, picks, name):
    case = picks.cases[name]
    try:
        setup(gpu, picks, case)
        seen = set()
        for cam in case["cams"]:
            want, ok = picks.codes(case, cam)
            assert ok.all()
            gpu.render(picks.cams[cam], picks.params(case), case["w"], case["h"])
            (got,) = host(gpu.pick_map())
            assert got.dtype == np.int32
            equal(got, want, f"{name} {cam}")
            seen |= set(int(v) for v in np.unique(got))
        assert seen >= set(case["covers"]), (name, sorted(seen))
        assert gpu.diag_counters() == {"hit_not_opaque": 0, "free_errors": 0}
    finally:
        reset(gpu, picks.wd)


def padded_map(r, frames, rows, w, label, pad=8, extra=24):
    """sr_pick_map with pitch 4 w + pad and stride pitch rows + extra ->
    int32 [frames, rows, w]; everything else stays SENT."""
    import torch

    pitch = 4 * w + pad
    stride = pitch * rows + extra
    buf = torch.full(((frames * stride) // 4 + 4,), SENT, dtype=torch.int32, device="cuda")
    rc = r.lib.sr_pick_map(r.ctx, C.c_void_p(buf.data_ptr()), pitch, stride, r._stream(None))
    assert rc == 0, (label, rc)
    (a,) = host(buf)
    assert (a[frames * stride // 4:] == SENT).all(), label
    a = a[:frames * stride // 4].reshape(frames, stride // 4)
    assert (a[:, pitch * rows // 4:] == SENT).all(), label + ": wrote between the frames"
    a = a[:, :pitch * rows // 4].reshape(frames, rows, pitch // 4)
    assert (a[:, :, w:] == SENT).all(), label + ": wrote into the pitch padding"
    return np.ascontiguousarray(a[:, :, :w])


def blocks_want(maps, blocks, br, h, w):
    want = np.full((len(maps), len(blocks) * br, w), SENT, dtype=np.int32)
    for f, m in enumerate(maps):
        for s, b in enumerate(blocks):
            if b >= 0:
                n = min(br, h - b * br)
                want[f, s * br:s * br + n] = m[b * br:b * br + n]
    return want


@pytest.mark.parametrize("kind", ["rows", "batch", "list"])
def test_kinds_padded(pkg, gpu, picks, kind):
    case = picks.cases["kinds"]
    w, h, prm = case["w"], case["h"], picks.params(case)
    names = case["cams"]
    cams = [picks.cams[c] for c in names]
    maps = [picks.codes(case, c)[0] for c in names]
    try:
        setup(gpu, picks, case)
        if kind == "rows":
            gpu.render(cams[0], prm, w, h, 3, 9)
            want = maps[0][3:9][None]
        elif kind == "batch":
            gpu.render_blocks_batch(cams, prm, w, h, BR, 0, 2)
            want = blocks_want(maps, [0, 2], BR, h, w)
        else:
            gpu.render_block_list(cams, prm, w, h, BR, LIST)
            want = blocks_want(maps, LIST, BR, h, w)
        got = padded_map(gpu, want.shape[0], want.shape[1], w, kind)
        for f in range(want.shape[0]):
            equal(got[f], want[f], f"{kind} frame {f}")
        dense = host(gpu.pick_map())[0].reshape(want.shape)
        written = want != SENT
        assert (dense[written] == want[written]).all() and (dense[~written] == pkg.abi.PICK_NONE).all()
    finally:
        reset(gpu, picks.wd)


def test_map_survives_a_relight_and_reshades(pkg, gpu, picks):
    case = picks.cases["default"]
    cam, prm, w, h = picks.cams["view"], picks.params(case), case["w"], case["h"]
    try:
        setup(gpu, picks, case)
        gpu.render(cam, prm, w, h)
        (before,) = host(gpu.pick_map())
        equal(before, picks.codes(case, "view")[0], "before")
        relit = R.relit(pkg, picks.passes(case)[0])
        assert pkg.abi.scene_shading_only(picks.passes(case)[0], relit)
        gpu.set_scene(relit)
        (mid,) = host(gpu.pick_map())
        a, = host(gpu.reshade())
        b, = host(gpu.reshade())
        (after,) = host(gpu.pick_map())
        equal(mid, before, "after a shading-only sr_set_scene")
        equal(after, before, "after two reshades")
        assert (a == b).all() and gpu.can_reshade()
    finally:
        reset(gpu, picks.wd)


def test_not_ready_and_rejections(pkg, gpu, picks):
    import torch

    abi, lib = pkg.abi, gpu.lib
    case = picks.cases["kinds"]
    cam, prm, w, h = picks.cams["view"], picks.params(case), case["w"], case["h"]
    buf = torch.full((3 * 16 * w + 8,), SENT, dtype=torch.int32, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    try:
        setup(gpu, picks, case)  # sr_set_test_ray drops whatever was retained
        assert lib.sr_pick_map(gpu.ctx, p, 4 * w, 0, None) == abi.SR_E_NOT_READY
        gpu.render_ss(cam, prm, w, h, 2)
        assert gpu.can_reshade()
        assert lib.sr_pick_map(gpu.ctx, p, 4 * w, 0, None) == abi.SR_E_NOT_READY  # the picking surface is the plain frame
        gpu.render(cam, prm, w, h)
        gpu.set_texture_array(picks.arr)
        assert lib.sr_pick_map(gpu.ctx, p, 4 * w, 0, None) == abi.SR_E_NOT_READY
        gpu.render(cam, prm, w, h)
        moved = pkg.scenes.struct_from_bytes(abi.Scene, pkg.scenes.struct_bytes(picks.passes(case)[0]))
        moved.spheres[0].radius += 0.5
        gpu.set_scene(moved)
        assert lib.sr_pick_map(gpu.ctx, p, 4 * w, 0, None) == abi.SR_E_NOT_READY
        gpu.render_adaptive(cam, prm, w, h, 2, 8)
        assert lib.sr_pick_map(gpu.ctx, p, 4 * w, 0, None) == abi.SR_E_NOT_READY
        gpu.set_scene(picks.passes(case)[0])
        gpu.render(cam, prm, w, h)
        INV = abi.SR_E_INVALID
        assert lib.sr_pick_map(None, p, 4 * w, 0, None) == INV
        assert lib.sr_pick_map(gpu.ctx, None, 4 * w, 0, None) == INV
        assert lib.sr_pick_map(gpu.ctx, p, 4 * w - 4, 0, None) == INV
        assert lib.sr_pick_map(gpu.ctx, p, 4 * w + 2, 0, None) == INV  # no multiple of 4
        assert lib.sr_pick_map(gpu.ctx, C.c_void_p(buf.data_ptr() + 2), 4 * w, 0, None) == INV
        gpu.render_block_list([cam, cam], prm, w, h, BR, LIST)
        n = len(LIST) * BR
        assert lib.sr_pick_map(gpu.ctx, p, 4 * w, 4 * w * n - 4, None) == INV  # a short stride
        assert lib.sr_pick_map(gpu.ctx, p, 4 * w, 4 * w * n + 2, None) == INV
        (got,) = host(buf)
        assert (got == SENT).all(), "a refused call wrote"
        assert lib.sr_pick_map(gpu.ctx, p, 4 * w, 4 * w * n, None) == abi.SR_OK
    finally:
        reset(gpu, picks.wd)


def test_renderer_pick(pkg, gpu, picks):
    case = picks.cases["default"]
    want = picks.codes(case, "view")[0]
    try:
        setup(gpu, picks, case)
        gpu.render(picks.cams["view"], picks.params(case), case["w"], case["h"])
        ys, xs = np.nonzero(want >= 0)
        pixels = [(int(xs[0]), int(ys[0])), (int(xs[-1]), int(ys[-1])), (0, 0)]
        hole = np.argwhere(want == P.HOLE)
        pixels.append((int(hole[0][1]), int(hole[0][0])))
        for x, y in pixels:
            assert gpu.pick(x, y) == int(want[y, x]), (x, y)
        assert want[0, 0] == P.SKY
    finally:
        reset(gpu, picks.wd)
