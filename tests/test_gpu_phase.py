"""Sample phases (sr_render_phase), the accumulator (sr_render_accumulate,
sr_accum_add, sr_accum_resolve) and progressive supersampling on the GPU.

The reference of every frame comparison is numpy slicing or summing the CPU
oracle's (ss W) x (ss H) RGBA8 frame S of the same scene, camera, params and
test ray:

    phase (i, j)          = S[j::ss, i::ss]
    all ss ss phases      = box_reference(S)   (sr.h's box rule, as sr_render_ss)
    the first k phases    = (their sum + k // 2) // k

Nothing has a tolerance. tests/test_phase_cases.py shows on the oracle alone
that any two phases of every cell differ on at least half of the pixels, so a
launch that ignored or swapped (i, j) cannot pass.

Cells: the five of tests/test_gpu_supersample.py at output 17x11, 300 steps
(one full and one partial tile column, every wave partial somewhere), and
one at 68x44, ss 2, 400 steps.
"""
import ctypes as C
import random

import numpy as np
import pytest

from test_gpu_launch_matrix import World, host, reset, same, setup, split_count
from test_gpu_supersample import CELL_IDS, CELLS, H, ROWS, SENTINEL, STEPS, W, box_reference

pytestmark = pytest.mark.gpu

CLEAN = {"hit_not_opaque": 0, "free_errors": 0}


@pytest.fixture(scope="module")
def wd(pkg, oracle, textures):
    w = World(pkg, oracle, textures)
    w.custom = {}
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


def need_gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch


def grid(ss):
    return [(i, j) for j in range(ss) for i in range(ss)]


def sample_frame(wd, key, ov, ss, w=W, h=H, steps=STEPS):
    return wd.ref(key, ov, "view", ss * w, ss * h, steps)[0]


def phase_of(S, ss, ph):
    return S[ph[1]::ss, ph[0]::ss]


def prefix_reference(S, ss, phases):
    k = len(phases)
    total = sum(phase_of(S, ss, ph).astype(np.int64) for ph in phases)
    return ((total + k // 2) // k).astype(np.uint8)


def as_u16(t):
    """A device accumulator (int16 tensor) as the ABI's uint16 on the host."""
    return host(t)[0].view(np.uint16)


# ---- 1. every phase of every cell
def check_every_phase(gpu, wd, S, ss, prm, label, w=W, h=H, rows=ROWS):
    import torch

    cam = wd.cams["view"]
    pitch, guard = 4 * w + 32, 1024
    y0, y1 = rows
    whole, band, padded = [], [], []
    for ph in grid(ss):
        for _ in range(2):  # the second launch runs the learned order
            out = gpu.render_phase(cam, prm, w, h, ss, *ph)
        whole.append(out)
        band.append(gpu.render_phase(cam, prm, w, h, ss, *ph, row_begin=y0, row_end=y1))
        buf = torch.full((2 * guard + pitch * (y1 - y0),), SENTINEL, dtype=torch.uint8, device="cuda")
        rc = gpu.lib.sr_render_phase(gpu.ctx, C.byref(cam), C.byref(prm), w, h, y0, y1, ss, ph[0], ph[1],
                                     C.c_void_p(buf.data_ptr() + guard), pitch, gpu._stream(None))
        assert rc == wd.pkg.abi.SR_OK
        padded.append(buf)
    got = host(*whole, *band, *padded)
    n = ss * ss
    for k, ph in enumerate(grid(ss)):
        ref = phase_of(S, ss, ph)
        same(got[k], ref, f"{label}, phase {ph}")
        same(got[n + k], ref[y0:y1], f"{label}, phase {ph}, rows {rows}")
        want = np.full(2 * guard + pitch * (y1 - y0), SENTINEL, dtype=np.uint8)
        for r in range(y1 - y0):
            want[guard + r * pitch:guard + r * pitch + 4 * w] = ref[y0 + r].reshape(-1)
        bad = got[2 * n + k] != want
        payload = want != SENTINEL
        assert not bad.any(), (f"{label}, phase {ph}, padded pitch: {int((bad & payload).sum())} payload bytes differ, "
                               f"{int((bad & ~payload).sum())} bytes outside the payload changed")


@pytest.mark.parametrize("ss", [2, 3, 4])
@pytest.mark.parametrize("key,overlay", CELLS, ids=CELL_IDS)
def test_every_phase(gpu, wd, key, overlay, ss):
    try:
        setup(gpu, wd, key, overlay)
        check_every_phase(gpu, wd, sample_frame(wd, key, overlay, ss), ss, wd.params(STEPS),
                          f"{key}, overlay {overlay}, ss {ss}")
    finally:
        reset(gpu, wd)


def test_every_phase_larger_cell(gpu, wd):
    try:
        setup(gpu, wd, "small", False)
        check_every_phase(gpu, wd, sample_frame(wd, "small", False, 2, 68, 44, 400), 2, wd.params(400),
                          "small, 68x44, ss 2", 68, 44, (7, 25))
    finally:
        reset(gpu, wd)


# ---- 2.
def test_ss1_phase_is_the_plain_frame(gpu, wd):
    try:
        setup(gpu, wd, "small", False)
        prm, cam = wd.params(STEPS), wd.cams["view"]
        plain, ph, band = host(gpu.render(cam, prm, W, H), gpu.render_phase(cam, prm, W, H, 1, 0, 0),
                               gpu.render_phase(cam, prm, W, H, 1, 0, 0, *ROWS))
        same(plain, wd.ref("small", False, "view", W, H, STEPS)[0], "sr_render")
        assert np.array_equal(ph, plain) and np.array_equal(band, plain[ROWS[0]:ROWS[1]])
        acc = gpu.render_accumulate(cam, prm, W, H, 1, [(0, 0)])
        assert np.array_equal(as_u16(acc), plain.astype(np.uint16))
        assert np.array_equal(host(gpu.accum_resolve(acc, 1))[0], plain)
    finally:
        reset(gpu, wd)


# ---- 3. the crosshair, the noise mask and the split modes are the sample's own
PER_SAMPLE = {
    "crosshair": ("small", dict(crosshair=1)),
    "percent_black": ("large", dict(percent_black=0.5)),
    "half_width": ("stacked", dict(raytrace_type=2)),  # SR_RAYTRACE_HALF_WIDTH
}


@pytest.mark.parametrize("ss", [2, 3])
@pytest.mark.parametrize("what", list(PER_SAMPLE))
def test_per_sample_evaluation(gpu, wd, what, ss):
    key, kw = PER_SAMPLE[what]
    assert wd.pkg.abi.RAYTRACE_HALF_WIDTH == 2
    prm = wd.params(STEPS)
    for name, v in kw.items():
        setattr(prm, name, v)
    if (what, ss) not in wd.custom:
        S = wd.oracle.render(wd.scene(key), wd.cams["view"], prm, ss * W, ss * H, wd.tex, wd.test_rays[False])[0]
        S.setflags(write=False)
        wd.custom[(what, ss)] = S
    S = wd.custom[(what, ss)]
    changed = int((S != sample_frame(wd, key, False, ss)).any(-1).sum())
    assert changed > 0, f"{what} leaves the oracle's sample frame unchanged"
    try:
        setup(gpu, wd, key, False)
        check_every_phase(gpu, wd, S, ss, prm, f"{what} ({changed} samples changed), ss {ss}")
        acc = gpu.render_accumulate(wd.cams["view"], prm, W, H, ss, grid(ss))
        same(host(gpu.accum_resolve(acc, ss * ss))[0], box_reference(S, ss), f"{what}, ss {ss}, accumulated")
    finally:
        reset(gpu, wd)


# ---- 4. all phases accumulated and resolved: the box rule, in any order and grouping
def groupings(ss):
    g = grid(ss)
    shuffled = list(g)
    random.Random(7).shuffle(shuffled)
    if shuffled == g:
        shuffled.reverse()
    return {
        "one launch": [g],
        "one phase per launch": [[ph] for ph in g],
        "3 then the rest": [g[:3], g[3:]],
        "shuffled, 2 per launch": [shuffled[k:k + 2] for k in range(0, len(g), 2)],
    }


@pytest.mark.parametrize("ss", [2, 3, 4])
@pytest.mark.parametrize("key,overlay", CELLS, ids=CELL_IDS)
def test_accumulate_resolves_to_the_box_rule(gpu, wd, key, overlay, ss):
    import torch

    abi = wd.pkg.abi
    S = sample_frame(wd, key, overlay, ss)
    ref = box_reference(S, ss)
    total = sum(phase_of(S, ss, ph).astype(np.int64) for ph in grid(ss)).astype(np.uint16)
    prm, cam, n = wd.params(STEPS), wd.cams["view"], ss * ss
    label = f"{key}, overlay {overlay}, ss {ss}"
    y0, y1 = ROWS
    try:
        setup(gpu, wd, key, overlay)
        frames, sums = [], []
        for name, groups in groupings(ss).items():
            acc = gpu.new_accum(W, H)
            acc.fill_(0x5A5A)  # the first launch resets: the old contents do not matter
            for k, group in enumerate(groups):
                gpu.render_accumulate(cam, prm, W, H, ss, group, accum=acc, reset=k == 0)
            sums.append(acc)
            frames.append(gpu.accum_resolve(acc, n))
        band = gpu.new_accum(W, y1 - y0)
        for k, group in enumerate(groupings(ss)["3 then the rest"]):
            gpu.render_accumulate(cam, prm, W, H, ss, group, accum=band, reset=k == 0, row_begin=y0, row_end=y1)
        band_frame = gpu.accum_resolve(band, n)
        # a padded accumulator pitch into a sentinel-filled buffer
        ap, guard = 8 * W + 24, 512
        buf = torch.full((2 * guard + ap * H,), SENTINEL, dtype=torch.uint8, device="cuda")
        flat = [v for ph in grid(ss) for v in ph]
        rc = gpu.lib.sr_render_accumulate(gpu.ctx, C.byref(cam), C.byref(prm), W, H, 0, H, ss,
                                          (C.c_uint8 * len(flat))(*flat), n, 1, C.c_void_p(buf.data_ptr() + guard), ap,
                                          gpu._stream(None))
        assert rc == abi.SR_OK
        padded_frame = torch.full((H, W + 2, 4), SENTINEL, dtype=torch.uint8, device="cuda")
        rc = gpu.lib.sr_accum_resolve(C.c_void_p(buf.data_ptr() + guard), ap, W, H, n,
                                      C.c_void_p(padded_frame.data_ptr()), 4 * (W + 2), 1, gpu._stream(None))
        assert rc == abi.SR_OK
        whole = gpu.render_ss(cam, prm, W, H, ss)
        for name, acc, frame in zip(groupings(ss), sums, frames):
            assert np.array_equal(as_u16(acc), total), f"{label}, {name}: the sums differ"
            same(host(frame)[0], ref, f"{label}, {name}")
        same(host(band_frame)[0], ref[y0:y1], f"{label}, rows {ROWS}")
        raw, pf, whole = host(buf, padded_frame, whole)
        want = np.full(raw.size, SENTINEL, dtype=np.uint8)
        for y in range(H):
            want[guard + y * ap:guard + y * ap + 8 * W] = total[y].reshape(-1).view(np.uint8)
        assert np.array_equal(raw, want), f"{label}: padded accumulator (payload or padding)"
        same(pf[:, :W], ref, f"{label}, padded accumulator resolved")
        assert (pf[:, W:] == SENTINEL).all()
        same(whole, ref, f"{label}, sr_render_ss")
    finally:
        reset(gpu, wd)


def test_accumulate_larger_cell(gpu, wd):
    S = sample_frame(wd, "small", False, 2, 68, 44, 400)
    prm, cam = wd.params(400), wd.cams["view"]
    try:
        setup(gpu, wd, "small", False)
        for groups in groupings(2).values():
            acc = None
            for group in groups:
                acc = gpu.render_accumulate(cam, prm, 68, 44, 2, group, accum=acc)
            same(host(gpu.accum_resolve(acc, 4))[0], box_reference(S, 2), f"68x44, ss 2, {groups}")
    finally:
        reset(gpu, wd)


# ---- 5. progressive prefixes
@pytest.mark.parametrize("ss", [1, 2, 3, 4])
@pytest.mark.parametrize("key,overlay", CELLS, ids=CELL_IDS)
def test_progressive_prefixes(gpu, wd, key, overlay, ss):
    order = wd.pkg.abi.phase_order(ss)
    S = sample_frame(wd, key, overlay, ss)
    prm, cam = wd.params(STEPS), wd.cams["view"]
    try:
        setup(gpu, wd, key, overlay)
        passes = list(gpu.progressive(cam, prm, W, H, ss))
        assert [k for k, _ in passes] == list(range(1, ss * ss + 1))
        threes = list(gpu.progressive(cam, prm, W, H, ss, phases_per_launch=3))
        assert [k for k, _ in threes] == [min(k + 3, ss * ss) for k in range(0, ss * ss, 3)]
        got = host(*[f for _, f in passes], *[f for _, f in threes])
        for (k, _), frame in zip(passes + threes, got):
            same(frame, prefix_reference(S, ss, order[:k]), f"{key}, overlay {overlay}, ss {ss}, after {k} passes")
        same(got[len(passes) - 1], box_reference(S, ss), "the last pass is the box rule")
    finally:
        reset(gpu, wd)


# ---- 6. the device add and resolve against the host forms
@pytest.mark.parametrize("n", [1, 3, 32, 256])
@pytest.mark.parametrize("width", [1, 67, 300])
def test_device_accum_equals_host(pkg, gpu, width, n):
    import torch

    abi = pkg.abi
    rows = 5
    rng = np.random.default_rng(width * 1000 + n)
    images = rng.integers(0, 256, (n, rows, width, 4), dtype=np.uint8)
    images[:, 0, 0] = 255  # n x 255 (255 x 256 = 65280 at n 256)
    start = rng.integers(0, 65536, (rows, width, 4), dtype=np.uint16)
    d_img = torch.from_numpy(images).cuda()
    stored = gpu.accum_add(d_img, gpu.new_accum(width, rows).fill_(0x1234), reset=True)
    added = gpu.accum_add(d_img, torch.from_numpy(start.view(np.int16)).cuda())
    one = gpu.accum_add(d_img[0], reset=True)
    frames = [gpu.accum_resolve(stored, n), gpu.accum_resolve(added, n), gpu.accum_resolve(added, 256 - n + 1)]
    h_stored = abi.accum_add(images, reset=True)
    h_added = abi.accum_add(images, start.copy())
    assert np.array_equal(as_u16(stored), h_stored) and h_stored[0, 0, 0] == n * 255
    assert np.array_equal(as_u16(added), h_added)
    assert np.array_equal(as_u16(one), images[0].astype(np.uint16))
    got = host(*frames)
    assert np.array_equal(got[0], abi.accum_resolve(h_stored, n))
    assert np.array_equal(got[1], abi.accum_resolve(h_added, n))
    assert np.array_equal(got[2], abi.accum_resolve(h_added, 256 - n + 1))
    assert np.array_equal(host(d_img)[0], images)


def test_device_resolve_is_exact_for_every_value_and_count(gpu):
    """Every acc in 0 .. 65535 with every n in 1 .. 256 against numpy."""
    import torch

    acc = np.arange(65536, dtype=np.uint16).reshape(64, 256, 4)
    d_acc = torch.from_numpy(acc.view(np.int16)).cuda()
    out = torch.empty((256, 64, 256, 4), dtype=torch.uint8, device="cuda")
    for n in range(1, 257):
        gpu.accum_resolve(d_acc, n, out=out[n - 1])
    got, = host(out)
    n = np.arange(1, 257, dtype=np.int64).reshape(256, 1, 1, 1)
    want = np.minimum(255, (acc.astype(np.int64)[None] + n // 2) // n).astype(np.uint8)
    assert np.array_equal(got, want)


# ---- 7. launch options leave the pixels unchanged
@pytest.mark.parametrize("option", ["split16", "split4", "split1", "latency", "cull_off"])
def test_launch_options(gpu, wd, option):
    ss = 3
    key, overlay = ("large", True) if option == "cull_off" else ("small", False)
    S = sample_frame(wd, key, overlay, ss)
    prm, cam = wd.params(STEPS), wd.cams["view"]
    try:
        setup(gpu, wd, key, overlay)
        if option.startswith("split"):
            gpu.set_split(4, int(option[5:]), 1)
        elif option == "latency":
            gpu.set_latency_mode(True)
        else:
            gpu.set_culling(False)
        outs = []
        for ph in grid(ss):
            for _ in range(2):  # the second launch runs the split tiles the first one chose
                out = gpu.render_phase(cam, prm, W, H, ss, *ph)
            outs.append(out)
        if option.startswith("split"):
            assert split_count(gpu) > 0
        acc = gpu.render_accumulate(cam, prm, W, H, ss, grid(ss))
        frame = gpu.accum_resolve(acc, ss * ss)
        for ph, img in zip(grid(ss), host(*outs)):
            same(img, phase_of(S, ss, ph), f"{option}, phase {ph}")
        same(host(frame)[0], box_reference(S, ss), f"{option}, accumulated")
    finally:
        reset(gpu, wd)


# ---- 8. other launches between phases on one context
def test_interleaved_with_other_launches(gpu, wd):
    ss = 2
    S = sample_frame(wd, "small", False, ss)
    plain_ref = wd.ref("small", False, "view", W, H, STEPS)[0]
    prm, cam = wd.params(STEPS), wd.cams["view"]
    g = grid(ss)
    try:
        setup(gpu, wd, "small", False)
        acc = gpu.render_accumulate(cam, prm, W, H, ss, g[:1])
        p0 = gpu.render_phase(cam, prm, W, H, ss, *g[0])
        plain = gpu.render(cam, prm, W, H)
        gpu.render_accumulate(cam, prm, W, H, ss, g[1:2], accum=acc)
        p1 = gpu.render_phase(cam, prm, W, H, ss, *g[1])
        whole = gpu.render_ss(cam, prm, W, H, ss)  # overwrites the sample scratch the accumulate launches use
        gpu.render_accumulate(cam, prm, W, H, ss, g[2:3], accum=acc)
        p2 = gpu.render_phase(cam, prm, W, H, ss, *g[2])
        adaptive, mask = gpu.render_adaptive(cam, prm, W, H, ss, -1)  # threshold < 0: every tile, sr_render_ss's frame
        gpu.render_accumulate(cam, prm, W, H, ss, g[3:], accum=acc)
        p3 = gpu.render_phase(cam, prm, W, H, ss, *g[3])
        plain2 = gpu.render(cam, prm, W, H)
        frame = gpu.accum_resolve(acc, 4)
        p0, p1, p2, p3, plain, plain2, whole, adaptive, mask, frame = host(p0, p1, p2, p3, plain, plain2, whole,
                                                                          adaptive, mask, frame)
        for ph, img in zip(g, (p0, p1, p2, p3)):
            same(img, phase_of(S, ss, ph), f"phase {ph} between other launches")
        same(plain, plain_ref, "sr_render between phases")
        same(plain2, plain_ref, "sr_render after the phases")
        same(whole, box_reference(S, ss), "sr_render_ss between phases")
        assert mask.all()
        same(adaptive, box_reference(S, ss), "sr_render_adaptive between phases")
        same(frame, box_reference(S, ss), "the accumulated frame")
    finally:
        reset(gpu, wd)


# ---- 9. two streams on one context
def test_one_context_on_two_streams(pkg, textures, wd):
    torch = need_gpu()
    bg, arr = textures
    ss = 3
    S = sample_frame(wd, "small", False, ss)
    prm, cam = wd.params(STEPS), wd.cams["view"]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    with pkg.Renderer(0) as r:
        r.set_background(bg)
        r.set_texture_array(arr)
        r.set_scene(wd.scene("small"))
        outs = [r.render_phase(cam, prm, W, H, ss, *ph, stream=streams[k % 2]) for k, ph in enumerate(grid(ss))]
        acc = r.new_accum(W, H)
        torch.cuda.synchronize()  # the accumulator's zero fill ran on the current stream
        # the context orders its launches: launch k + 1 on the other stream waits for the add of
        # launch k, which read the sample scratch and wrote the accumulator
        order = pkg.abi.phase_order(ss)
        for k, ph in enumerate(order):
            r.render_accumulate(cam, prm, W, H, ss, [ph], accum=acc, reset=k == 0, stream=streams[k % 2])
        frame = r.accum_resolve(acc, ss * ss, stream=streams[(len(order) - 1) % 2])
        got = host(*outs, frame)
        for ph, img in zip(grid(ss), got):
            same(img, phase_of(S, ss, ph), f"phase {ph} on alternating streams")
        same(got[-1], box_reference(S, ss), "one phase per launch on alternating streams")
        assert r.diag_counters() == CLEAN


# ---- 10. small frames
@pytest.mark.parametrize("ss", [2, 3, 4])
@pytest.mark.parametrize("w,h", [(1, 1), (8, 8), (65, 1)])
def test_small_frames(gpu, wd, w, h, ss):
    S = sample_frame(wd, "small", False, ss, w, h)
    prm, cam = wd.params(STEPS), wd.cams["view"]
    try:
        setup(gpu, wd, "small", False)
        outs = [gpu.render_phase(cam, prm, w, h, ss, *ph) for ph in grid(ss)]
        acc = gpu.render_accumulate(cam, prm, w, h, ss, grid(ss))
        frame = gpu.accum_resolve(acc, ss * ss)
        for ph, img in zip(grid(ss), host(*outs)):
            same(img, phase_of(S, ss, ph), f"{w}x{h}, ss {ss}, phase {ph}")
        same(host(frame)[0], box_reference(S, ss), f"{w}x{h}, ss {ss}, accumulated")
    finally:
        reset(gpu, wd)


# ---- 11. rejections
def test_rejections_on_a_live_context(pkg, gpu, wd):
    """Each bad call returns its status before anything is launched or
    written; the good calls after them still give the reference."""
    import torch

    abi, lib = pkg.abi, gpu.lib
    ss = 2
    S = sample_frame(wd, "small", False, ss)
    try:
        setup(gpu, wd, "small", False)
        prm, cam = wd.params(STEPS), wd.cams["view"]
        st = gpu._stream(None)
        img = torch.full((H, W, 4), SENTINEL, dtype=torch.uint8, device="cuda")
        acc = torch.full((H, W, 4), 0x2D2D, dtype=torch.int16, device="cuda")
        I, A = img.data_ptr(), acc.data_ptr()
        assert A % 8 == 0
        ph33 = (C.c_uint8 * 66)(*([0, 1] * 33))

        def phase(ctx=gpu.ctx, s=ss, x=0, y=0, y0=0, y1=H, out=I, pitch=4 * W):
            return lib.sr_render_phase(ctx, C.byref(cam), C.byref(prm), W, H, y0, y1, s, x, y, out, pitch, st)

        def accumulate(ctx=gpu.ctx, s=ss, phases=ph33, n=4, y0=0, y1=H, accum=A, ap=8 * W):
            return lib.sr_render_accumulate(ctx, C.byref(cam), C.byref(prm), W, H, y0, y1, s, phases, n, 0, accum, ap, st)

        for kw in [dict(s=0), dict(s=5), dict(s=-1), dict(x=2), dict(y=2), dict(x=-1), dict(y=-1), dict(s=1, x=1),
                   dict(out=None), dict(pitch=4 * W - 4), dict(y1=H + 1), dict(y0=5, y1=4), dict(y0=-1), dict(ctx=None)]:
            assert phase(**kw) == abi.SR_E_INVALID, kw
        for kw in [dict(s=0), dict(s=5), dict(phases=None), dict(accum=None), dict(n=0), dict(n=-1),
                   dict(phases=(C.c_uint8 * 4)(0, 0, 2, 0), n=2), dict(phases=(C.c_uint8 * 4)(0, 0, 1, 2), n=2), dict(s=1),
                   dict(ap=8 * W - 8), dict(ap=8 * W + 4), dict(accum=A + 4), dict(accum=A + 2), dict(y1=H + 1),
                   dict(y0=5, y1=4), dict(ctx=None)]:
            assert accumulate(**kw) == abi.SR_E_INVALID, kw
        assert accumulate(n=33) == abi.SR_E_CAPACITY
        with pkg.Renderer(0) as empty:  # a context without a scene
            assert phase(ctx=empty.ctx) == abi.SR_E_NOT_READY and accumulate(ctx=empty.ctx) == abi.SR_E_NOT_READY
        for kw in [dict(n=0), dict(n=257), dict(accum=A + 4), dict(out=I + 2), dict(pitch=4 * W - 4), dict(out=None)]:
            a = dict(accum=A, n=4, out=I, pitch=4 * W)
            a.update(kw)
            assert lib.sr_accum_resolve(a["accum"], 8 * W, W, H, a["n"], a["out"], a["pitch"], 1, st) == abi.SR_E_INVALID, kw
        for kw in [dict(n=0), dict(n=257), dict(accum=A + 4), dict(images=I + 1), dict(images=None)]:
            a = dict(accum=A, n=1, images=I)
            a.update(kw)
            assert lib.sr_accum_add(a["images"], 4 * W, 4 * W * H, a["n"], W, H, 0, a["accum"], 8 * W, 1, st) == abi.SR_E_INVALID, kw
        assert phase(y0=4, y1=4) == abi.SR_OK and accumulate(y0=4, y1=4) == abi.SR_OK  # no rows: nothing is written
        got_img, got_acc = host(img, acc)
        assert (got_img == SENTINEL).all() and (got_acc == 0x2D2D).all()
        same(host(gpu.render_phase(cam, prm, W, H, ss, 1, 0))[0], phase_of(S, ss, (1, 0)), "the good phase after the refusals")
    finally:
        reset(gpu, wd)


def test_a_full_batch_of_phases(gpu, wd):
    """SR_MAX_BATCH phases in one launch: the 16 of ss 4, each twice."""
    ss = 4
    S = sample_frame(wd, "small", False, ss)
    prm, cam = wd.params(STEPS), wd.cams["view"]
    try:
        setup(gpu, wd, "small", False)
        acc = gpu.render_accumulate(cam, prm, W, H, ss, grid(ss) + grid(ss)[::-1])
        assert len(grid(ss)) * 2 == wd.pkg.abi.MAX_BATCH
        same(host(gpu.accum_resolve(acc, 32))[0], box_reference(S, ss), "32 phases in one launch")
    finally:
        reset(gpu, wd)


# ---- 13. a phase launch has the pixel state of a plain frame of the output's size
def test_pixel_state_is_the_output_frames(pkg, textures, wd):
    need_gpu()
    bg, arr = textures
    prm, cam = wd.params(STEPS), wd.cams["view"]
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    fields = pkg.abi.PS_FIELDS
    with pkg.Renderer(0) as r:
        r.set_background(bg)
        r.set_texture_array(arr)
        r.set_scene(wd.scene("small"))
        r.render_phase(cam, prm, W, H, 4, 3, 2)
        assert r.pixel_state().size == tiles * 256 * fields
        r.render_accumulate(cam, prm, W, H, 4, [(0, 0)])
        assert r.pixel_state().size == tiles * 256 * fields
        r.render_accumulate(cam, prm, W, H, 4, grid(4)[:5])
        assert r.pixel_state().size == 5 * tiles * 256 * fields
        stiles = ((4 * W + 15) // 16) * ((4 * H + 15) // 16)
        assert 5 * tiles < stiles  # still below the sample frame's
        assert r.diag_counters() == CLEAN


# ---- 12.
def test_zz_diag_counters_zero(gpu):
    assert gpu.diag_counters() == CLEAN
