"""Adaptive supersampling (sr_render_adaptive) and the device tile selection
(sr_edge_tiles) on the GPU.

The reference of every frame comparison is numpy applying sr.h's definition to
the CPU oracle's frames of the same scene, camera, params and test ray: P is
the oracle's W x H frame, R the box resolve of its (ss W) x (ss H) frame, the
flagged tiles are test_edge_tiles.rule on P, and the output is R in the
flagged tiles and P elsewhere. Frame and tile mask are compared byte for
byte; nothing has a tolerance.

Output 68x44 at 400 steps: 5x3 tiles, a last tile column 4 pixels wide and a
last tile row 12 rows high. Every cell first asserts, on the reference alone,
that it cannot pass vacuously (reference_of): at least two flagged and two
unflagged tiles, R != P on at least 25 % of the flagged pixels (returning P
fails) and, for the small and large scenes, on at least 25 % of the unflagged
ones (supersampling everything fails); at least one such pixel otherwise.
"""
import ctypes as C

import numpy as np
import pytest

from test_edge_tiles import rule
from test_gpu_launch_matrix import World, host, reset, same, setup
from test_gpu_supersample import box_reference

pytestmark = pytest.mark.gpu

W, H, STEPS = 68, 44, 400
GX, GY = (W + 15) // 16, (H + 15) // 16
# (scene, overlay, threshold, flagged tiles of the reference)
CELLS = [("small", False, 192, 10), ("large", False, 128, 5), ("stacked", False, 64, 4), ("small", True, 192, 13),
         ("large", True, 128, 8)]
CELL_IDS = ["small", "large", "stacked", "small-overlay", "large-overlay"]
MIN_SHARE = 0.25
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def wd(pkg, oracle, textures):
    w = World(pkg, oracle, textures)
    w.adaptive_refs = {}
    return w


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


def pixel_mask(tiles, w, h):
    return np.repeat(np.repeat(tiles, 16, 0), 16, 1)[:h, :w]


def reference_of(wd, key, ov, ss, threshold, grow=0, w=W, h=H, checked=True, min_unflagged=None):
    """(frame, uint8 tile mask) of the definition on the oracle's frames
    (read-only). checked: the conditions that keep a comparison from passing
    vacuously; min_unflagged: the least share of unflagged pixels where R != P
    (None: one pixel)."""
    k = (key, ov, ss, threshold, grow, w, h)
    if k not in wd.adaptive_refs:
        plain = wd.ref(key, ov, "view", w, h, STEPS)[0]
        res = box_reference(wd.ref(key, ov, "view", ss * w, ss * h, STEPS)[0], ss)
        tiles = rule(plain, threshold, grow)
        px = pixel_mask(tiles, w, h)
        frame = np.where(px[..., None], res, plain)
        changed = (res != plain).any(-1)
        frame.setflags(write=False)
        mask = tiles.astype(np.uint8)
        mask.setflags(write=False)
        wd.adaptive_refs[k] = (frame, mask, changed, px)
    frame, mask, changed, px = wd.adaptive_refs[k]
    if checked:
        n = int(mask.sum())
        assert 2 <= n <= mask.size - 2, f"{k}: {n} of {mask.size} tiles flagged"
        inside, outside = float(changed[px].mean()), float(changed[~px].mean())
        assert inside >= MIN_SHARE, f"{k}: R differs from P on {inside:.0%} of the flagged pixels"
        if min_unflagged is None:
            assert changed[~px].any(), f"{k}: R equals P on every unflagged pixel"
        else:
            assert outside >= min_unflagged, f"{k}: R differs from P on {outside:.0%} of the unflagged pixels"
    return frame, mask


def check(got, want, label):
    frame, mask = host(*got)
    same(frame, want[0], label)
    assert np.array_equal(mask, want[1]), f"{label}: tile mask {mask.tolist()}, reference {want[1].tolist()}"


# ---- the cells
@pytest.mark.parametrize("ss", [2, 3, 4])
@pytest.mark.parametrize("key,overlay,threshold,flagged", CELLS, ids=CELL_IDS)
def test_cells(gpu, wd, key, overlay, threshold, flagged, ss):
    """Twice in a row (the second launch runs the learned order of P), once
    in latency mode, once with culling off."""
    label = f"{key}, overlay {'on' if overlay else 'off'}, ss {ss}, threshold {threshold}"
    want = reference_of(wd, key, overlay, ss, threshold,
                        min_unflagged=MIN_SHARE if key in ("small", "large") and not overlay else None)
    assert int(want[1].sum()) == flagged, (label, want[1].tolist())
    prm, cam = wd.params(STEPS), wd.cams["view"]
    try:
        setup(gpu, wd, key, overlay)
        for i in range(2):
            check(gpu.render_adaptive(cam, prm, W, H, ss, threshold), want, f"{label}, launch {i}")
        gpu.set_latency_mode(True)
        check(gpu.render_adaptive(cam, prm, W, H, ss, threshold), want, f"{label}, latency mode")
        gpu.set_latency_mode(False)
        gpu.set_culling(False)
        check(gpu.render_adaptive(cam, prm, W, H, ss, threshold), want, f"{label}, culling off")
    finally:
        reset(gpu, wd)


@pytest.mark.parametrize("ss", [2, 3, 4])
def test_grow_1_on_the_large_cell(gpu, wd, ss):
    """12 of the 15 tiles; R differs from P on 42 - 49 % of the flagged and
    53 - 63 % of the unflagged pixels."""
    want = reference_of(wd, "large", False, ss, 128, grow=1, min_unflagged=MIN_SHARE)
    assert int(want[1].sum()) == 12
    try:
        setup(gpu, wd, "large", False)
        check(gpu.render_adaptive(wd.cams["view"], wd.params(STEPS), W, H, ss, 128, grow=1), want, f"grow 1, ss {ss}")
    finally:
        reset(gpu, wd)


@pytest.mark.parametrize("ss", [2, 4])
def test_grow_2_on_stacked(gpu, wd, ss):
    """The 5x5 neighbourhoods of stacked's four seeds, clipped to the 5x3
    grid: more tiles than grow 0, the reference says which."""
    want = reference_of(wd, "stacked", False, ss, 64, grow=2, checked=False)
    seeds = reference_of(wd, "stacked", False, ss, 64)[1]
    assert int(want[1].sum()) > int(seeds.sum()) and (want[1] >= seeds).all()
    try:
        setup(gpu, wd, "stacked", False)
        check(gpu.render_adaptive(wd.cams["view"], wd.params(STEPS), W, H, ss, 64, grow=2), want, f"grow 2, ss {ss}")
    finally:
        reset(gpu, wd)


@pytest.mark.parametrize("ss", [2, 3, 4])
def test_threshold_limits(gpu, wd, ss):
    """threshold -1: sr_render_ss's frame with an all-ones mask (through the
    sparse launch with every tile listed); threshold 255: sr_render's with an
    all-zero mask."""
    prm, cam = wd.params(STEPS), wd.cams["view"]
    try:
        setup(gpu, wd, "small", False)
        full, plain = host(gpu.render_ss(cam, prm, W, H, ss), gpu.render(cam, prm, W, H))
        same(plain, wd.ref("small", False)[0], "sr_render")
        same(full, box_reference(wd.ref("small", False, "view", ss * W, ss * H)[0], ss), "sr_render_ss")
        assert (full != plain).any(-1).mean() >= MIN_SHARE
        for grow in (0, 2):
            check(gpu.render_adaptive(cam, prm, W, H, ss, -1, grow), (full, np.ones((GY, GX), np.uint8)),
                  f"ss {ss}, threshold -1, grow {grow}")
            check(gpu.render_adaptive(cam, prm, W, H, ss, 255, grow), (plain, np.zeros((GY, GX), np.uint8)),
                  f"ss {ss}, threshold 255, grow {grow}")
        check(gpu.render_adaptive(cam, prm, W, H, ss, 1000), (plain, np.zeros((GY, GX), np.uint8)), "threshold 1000")
    finally:
        reset(gpu, wd)


@pytest.mark.parametrize("threshold", [-1, 192])
@pytest.mark.parametrize("w,h", [(1, 1), (16, 16), (17, 11)], ids=["1x1", "16x16", "17x11"])
def test_small_frames(gpu, wd, w, h, threshold):
    """One pixel (no neighbour: flagged only by threshold -1), exactly one
    tile, and two tiles with the second one pixel wide (flagged and
    unflagged at threshold 192), at ss 3."""
    want = reference_of(wd, "small", False, 3, threshold, w=w, h=h, checked=False)
    if threshold < 0:
        assert want[1].all()
    else:
        assert want[1].tolist() == {(1, 1): [[0]], (16, 16): [[1]], (17, 11): [[1, 0]]}[(w, h)]
    try:
        setup(gpu, wd, "small", False)
        for i in range(2):
            check(gpu.render_adaptive(wd.cams["view"], wd.params(STEPS), w, h, 3, threshold), want,
                  f"{w}x{h}, threshold {threshold}, launch {i}")
    finally:
        reset(gpu, wd)


@pytest.mark.parametrize("ss,extra", [(2, 32), (3, 32), (2, 5)], ids=["ss2", "ss3", "ss2-unaligned"])
def test_padded_pitch_and_null_mask(gpu, wd, ss, extra):
    """pitch 4 W + extra into the middle of a sentinel-filled buffer, the
    tile mask NULL: the payload equals the reference, every other byte still
    holds the sentinel. extra 5 with the buffer 1 byte off: the selection's
    and the resolve's byte paths."""
    import torch

    abi, lib = wd.pkg.abi, gpu.lib
    prm, cam = wd.params(STEPS), wd.cams["view"]
    frame, _ = reference_of(wd, "small", False, ss, 192, min_unflagged=MIN_SHARE)
    pitch, guard = 4 * W + extra, 4096 + (extra & 3)
    size = 2 * guard + pitch * H
    want = np.full(size, SENTINEL, dtype=np.uint8)
    for y in range(H):
        want[guard + y * pitch: guard + y * pitch + 4 * W] = frame[y].reshape(-1)
    try:
        setup(gpu, wd, "small", False)
        for i in range(2):
            buf = torch.full((size,), SENTINEL, dtype=torch.uint8, device="cuda")
            rc = lib.sr_render_adaptive(gpu.ctx, C.byref(cam), C.byref(prm), W, H, ss, 192, 0,
                                        C.c_void_p(buf.data_ptr() + guard), pitch, None, gpu._stream(None))
            assert rc == abi.SR_OK
            got, = host(buf)
            payload = want != SENTINEL
            bad = got != want
            assert not bad.any(), (f"launch {i}: {int((bad & payload).sum())} payload bytes differ, "
                                   f"{int((bad & ~payload).sum())} bytes outside the payload changed")
    finally:
        reset(gpu, wd)


def test_other_launches_after_an_adaptive_one(gpu, wd):
    """sr_render, sr_render_ss and sr_render_blocks_batch on the context after
    adaptive calls give their usual frames, with split tiles on: the learned
    order (the sparse launch must not touch it), the sample scratch and the
    pixel state are not disturbed, and adaptive calls between them still give
    theirs."""
    prm, cam = wd.params(STEPS), wd.cams["view"]
    plain = wd.ref("small", False)[0]
    res2 = box_reference(wd.ref("small", False, "view", 2 * W, 2 * H)[0], 2)
    want = reference_of(wd, "small", False, 4, 192, min_unflagged=MIN_SHARE)
    try:
        setup(gpu, wd, "small", False)
        gpu.set_split(4, 4, 1)
        for i in range(2):
            check(gpu.render_adaptive(cam, prm, W, H, 4, 192), want, f"adaptive {i}")
        codes = gpu.last_order()  # P's learned order: every tile once, four of them split
        assert sorted(set(int(c) >> 8 for c in codes if c >= 0)) == list(range(GX * GY))
        assert int(((codes >= 0) & ((codes & 0x80) != 0)).sum()) == 4 * 16
        same(host(gpu.render(cam, prm, W, H))[0], plain, "sr_render after adaptive")
        check(gpu.render_adaptive(cam, prm, W, H, 4, 192), want, "adaptive after sr_render")
        same(host(gpu.render_ss(cam, prm, W, H, 2))[0], res2, "sr_render_ss after adaptive")
        check(gpu.render_adaptive(cam, prm, W, H, 4, 192), want, "adaptive after sr_render_ss")
        cams = wd.cam_array(wd.batch)
        for _ in range(2):
            out, rows = gpu.render_blocks_batch(cams, prm, W, H, 8, 0, 1)
        got, = host(out)
        assert rows == H
        for f, name in enumerate(wd.batch):
            same(got[f, :H], wd.ref("small", False, name)[0], f"render_blocks_batch after adaptive, frame {name}")
        check(gpu.render_adaptive(cam, prm, W, H, 4, 192), want, "adaptive after the batch")
    finally:
        reset(gpu, wd)


def test_one_context_on_two_streams(pkg, textures, wd):
    """Adaptive calls at two sizes and ss alternating with plain and fully
    supersampled renders on two streams of one context (the scratch, the mask
    and the code list regrow; every stream change waits on the event recorded
    after the masked resolve)."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    bg, arr = textures
    prm, cam = wd.params(STEPS), wd.cams["view"]
    small = (17, 11)
    refs = {
        ("a", 2): reference_of(wd, "small", False, 2, 192, min_unflagged=MIN_SHARE),
        ("a", 4): reference_of(wd, "small", False, 4, 192, min_unflagged=MIN_SHARE),
        ("s", 3): reference_of(wd, "small", False, 3, 192, w=small[0], h=small[1], checked=False),
    }
    ops = [("s", 3, 0), ("a", 2, 1), ("plain", 1, 0), ("a", 4, 1), ("a", 2, 0), ("ss", 2, 1), ("s", 3, 1), ("a", 4, 0)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    with pkg.Renderer(0) as r:
        r.set_background(bg)
        r.set_texture_array(arr)
        r.set_scene(wd.scene("small"))
        outs = []
        for kind, ss, k in ops:
            if kind == "plain":
                outs.append((r.render(cam, prm, W, H, stream=streams[k]),))
            elif kind == "ss":
                outs.append((r.render_ss(cam, prm, W, H, ss, stream=streams[k]),))
            elif kind == "s":
                outs.append(r.render_adaptive(cam, prm, small[0], small[1], ss, 192, stream=streams[k]))
            else:
                outs.append(r.render_adaptive(cam, prm, W, H, ss, 192, stream=streams[k]))
        torch.cuda.synchronize()
        for (kind, ss, k), o in zip(ops, outs):
            label = f"{kind}, ss {ss}, stream {k}"
            if kind == "plain":
                same(host(*o)[0], wd.ref("small", False)[0], label)
            elif kind == "ss":
                same(host(*o)[0], box_reference(wd.ref("small", False, "view", ss * W, ss * H)[0], ss), label)
            else:
                check(o, refs[(kind, ss)], label)
        assert r.diag_counters() == {"hit_not_opaque": 0, "free_errors": 0}


@pytest.mark.parametrize("key,overlay,threshold,flagged", CELLS, ids=CELL_IDS)
def test_device_edge_tiles_equals_host(gpu, wd, key, overlay, threshold, flagged):
    """sr_edge_tiles on the device against its host form and the rule on the
    oracle's P, dense and (1 byte off, pitch 4 W + 5) through the byte path."""
    import torch

    abi, lib = wd.pkg.abi, gpu.lib
    plain = wd.ref(key, overlay)[0]
    d_plain = torch.from_numpy(np.array(plain)).cuda()
    pitch = 4 * W + 5
    packed = np.full(1 + pitch * H, SENTINEL, dtype=np.uint8)
    for y in range(H):
        packed[1 + y * pitch: 1 + y * pitch + 4 * W] = plain[y].reshape(-1)
    d_packed = torch.from_numpy(packed).cuda()
    for thr, grow in [(threshold, 0), (threshold, 1), (threshold, 2), (-1, 0), (0, 0), (16, 1), (254, 0), (255, 2)]:
        want = abi.edge_tiles(plain, thr, grow)
        assert np.array_equal(want.astype(bool), rule(plain, thr, grow))
        if (thr, grow) == (threshold, 0):
            assert int(want.sum()) == flagged
        got, = host(gpu.edge_tiles(d_plain, thr, grow))
        assert np.array_equal(got, want), (key, overlay, thr, grow, got.tolist(), want.tolist())
        odd = torch.full((GY, GX), 9, dtype=torch.uint8, device="cuda")
        rc = lib.sr_edge_tiles(C.c_void_p(d_packed.data_ptr() + 1), pitch, W, H, thr, grow, C.c_void_p(odd.data_ptr()), 1,
                               gpu._stream(None))
        assert rc == abi.SR_OK
        assert np.array_equal(host(odd)[0], want), (key, overlay, thr, grow, "byte path")


def test_rejections_on_a_live_context(pkg, gpu, wd):
    """Each bad call returns its status before anything is launched or
    written; the good call after them still gives the reference."""
    import torch

    abi, lib = wd.pkg.abi, gpu.lib
    want = reference_of(wd, "small", False, 2, 192, min_unflagged=MIN_SHARE)
    try:
        setup(gpu, wd, "small", False)
        prm, cam = wd.params(STEPS), wd.cams["view"]
        st = gpu._stream(None)
        buf = torch.full((H, W, 4), SENTINEL, dtype=torch.uint8, device="cuda")
        mask = torch.full((GY, GX), SENTINEL, dtype=torch.uint8, device="cuda")
        p, m = C.c_void_p(buf.data_ptr()), C.c_void_p(mask.data_ptr())

        def call(ctx=gpu.ctx, params=prm, w=W, h=H, ss=2, thr=192, grow=0, out=p, pitch=4 * W):
            return lib.sr_render_adaptive(ctx, C.byref(cam), C.byref(params), w, h, ss, thr, grow, out, pitch, m, st)

        for ss in (1, 0, -2, 5):
            assert call(ss=ss) == abi.SR_E_INVALID, ss
        assert call(grow=-1) == abi.SR_E_INVALID and call(grow=3) == abi.SR_E_INVALID
        assert call(out=None) == abi.SR_E_INVALID
        assert call(pitch=4 * W - 4) == abi.SR_E_INVALID
        assert call(h=(1 << 23) + 1) == abi.SR_E_INVALID  # 2 x h sample rows > 2^24
        assert call(ss=4, h=(1 << 22) + 1) == abi.SR_E_INVALID
        assert call(w=0) == abi.SR_E_INVALID and call(h=0) == abi.SR_E_INVALID
        assert call(params=wd.params(raytrace_type=4)) == abi.SR_E_INVALID
        assert call(ctx=None) == abi.SR_E_INVALID
        assert call(thr=255, ss=5) == abi.SR_E_INVALID and call(thr=-1, grow=3) == abi.SR_E_INVALID
        with pkg.Renderer(0) as empty:  # a context without a scene
            assert call(ctx=empty.ctx) == abi.SR_E_NOT_READY
            assert call(ctx=empty.ctx, thr=255) == abi.SR_E_NOT_READY
        frame, tiles = host(buf, mask)
        assert (frame == SENTINEL).all() and (tiles == SENTINEL).all()
        dm = torch.full((GY, GX), SENTINEL, dtype=torch.uint8, device="cuda")
        img = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
        ip, mp = C.c_void_p(img.data_ptr()), C.c_void_p(dm.data_ptr())
        for args in [(None, 4 * W, W, H, 0, 0, mp), (ip, 4 * W, W, H, 0, 0, None), (ip, 4 * W - 1, W, H, 0, 0, mp),
                     (ip, 4 * W, 0, H, 0, 0, mp), (ip, 4 * W, W, -1, 0, 0, mp), (ip, 4 * W, W, H, 0, 3, mp),
                     (ip, 4 * W, W, H, 0, -1, mp)]:
            assert lib.sr_edge_tiles(*args, 1, st) == abi.SR_E_INVALID, args
        assert (host(dm)[0] == SENTINEL).all()
        check(gpu.render_adaptive(cam, prm, W, H, 2, 192), want, "the good call after the refused ones")
    finally:
        reset(gpu, wd)


def test_zz_diag_counters_zero(gpu):
    assert gpu.diag_counters() == {"hit_not_opaque": 0, "free_errors": 0}
