"""Supersampled launches (sr_render_ss, sr_render_block_list_ss) and the
device resolve (sr_resolve_box) on the GPU.

The reference of every frame comparison is numpy applying sr.h's rule

    out[y][x][c] = (sum of the ss x ss samples' bytes + (ss ss) / 2) div (ss ss)

to the CPU oracle's (ss W) x (ss H) RGBA8 frame of the same scene, camera,
params and test ray. Nothing has a tolerance. Every case first asserts, on
the reference alone, that the resolved frame differs from the oracle's plain
W x H frame on at least 25 % of the pixels: an implementation that returned
the plain frame cannot pass.

A. The matrix: output 17x11 at 300 steps (sample frames 34x22, 51x33, 68x44:
   every wave shape is partial somewhere), ss 2 / 3 / 4, the small, large and
   stacked scenes and the first two with the test-ray overlay, through the
   whole frame, a row band and a three-camera block list with padding and a
   partial last block; one larger cell (68x44, ss 2, 400 steps).
B. ss 1, padded buffers, two ranks' priced lists reassembled on the device,
   two streams on one context, the device resolve against the host's,
   rejections, the diagnostic counters.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_launch_matrix import FILL, World, host, reset, same, setup

pytestmark = pytest.mark.gpu

W, H, STEPS = 17, 11, 300
ROWS = (3, 9)
BR, LIST = 4, [2, -1, 0]  # block 2 holds the frame's last 3 rows
CELLS = [("small", False), ("large", False), ("stacked", False), ("small", True), ("large", True)]
CELL_IDS = ["small", "large", "stacked", "small-overlay", "large-overlay"]
MIN_CHANGED = 0.25
SENTINEL = 0xA5


def box_reference(samples, ss):
    s = np.asarray(samples)
    rows, w = s.shape[-3] // ss, s.shape[-2] // ss
    v = s.reshape(s.shape[:-3] + (rows, ss, w, ss, 4)).astype(np.int64)
    return ((v.sum(axis=(-4, -2)) + (ss * ss) // 2) // (ss * ss)).astype(np.uint8)


@pytest.fixture(scope="module")
def wd(pkg, oracle, textures):
    w = World(pkg, oracle, textures)
    w.ss_refs = {}
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


def ss_ref(wd, key, ov, cam, ss, w=W, h=H, steps=STEPS):
    """The resolved oracle frame of a cell (read-only), after the check that
    it is not the plain frame."""
    k = (key, ov, cam, ss, w, h, steps)
    if k not in wd.ss_refs:
        ref = box_reference(wd.ref(key, ov, cam, ss * w, ss * h, steps)[0], ss)
        plain = wd.ref(key, ov, cam, w, h, steps)[0]
        changed = float((ref != plain).any(-1).mean())
        assert changed >= MIN_CHANGED, f"{k}: the reference differs from the plain frame on {changed:.0%} of the pixels"
        ref.setflags(write=False)
        wd.ss_refs[k] = ref
    return wd.ss_refs[k]


def list_want(refs, blocks, br, h, w):
    """[frames, len(blocks) * br, w, 4]: FILL where the call writes nothing."""
    want = np.full((len(refs), len(blocks) * br, w, 4), FILL, dtype=np.uint8)
    for f, rb in enumerate(refs):
        for s, b in enumerate(blocks):
            if b >= 0:
                n = min(br, h - b * br)
                want[f, s * br:s * br + n] = rb[b * br:b * br + n]
    return want


def run_paths(gpu, wd, key, ov, ss, path, w, h, steps, rows, br, blocks):
    import torch

    label = f"{key}, overlay {'on' if ov else 'off'}, ss {ss}, {w}x{h}, {path}"
    prm = wd.params(steps)
    if path == "frame":
        ref = ss_ref(wd, key, ov, "view", ss, w, h, steps)
        for _ in range(2):  # the second launch runs the learned order
            got, = host(gpu.render_ss(wd.cams["view"], prm, w, h, ss))
        same(got, ref, label)
    elif path == "rows":
        ref = ss_ref(wd, key, ov, "view", ss, w, h, steps)
        y0, y1 = rows
        got, = host(gpu.render_ss(wd.cams["view"], prm, w, h, ss, y0, y1))
        same(got, ref[y0:y1], label)
    else:
        refs = [ss_ref(wd, key, ov, c, ss, w, h, steps) for c in wd.batch]
        out = torch.full((len(refs), len(blocks) * br, w, 4), FILL, dtype=torch.uint8, device="cuda")
        for _ in range(2):
            gpu.render_block_list_ss(wd.cam_array(wd.batch), prm, w, h, br, blocks, ss, out=out)
        got, = host(out)
        want = list_want(refs, blocks, br, h, w)
        for f, name in enumerate(wd.batch):
            same(got[f], want[f], f"{label}, frame {name}")


# ---- A. the matrix
@pytest.mark.parametrize("path", ["frame", "rows", "list"])
@pytest.mark.parametrize("ss", [2, 3, 4])
@pytest.mark.parametrize("key,overlay", CELLS, ids=CELL_IDS)
def test_matrix(gpu, wd, key, overlay, ss, path):
    try:
        setup(gpu, wd, key, overlay)
        run_paths(gpu, wd, key, overlay, ss, path, W, H, STEPS, ROWS, BR, LIST)
    finally:
        reset(gpu, wd)


@pytest.mark.parametrize("path", ["frame", "rows", "list"])
def test_larger_cell(gpu, wd, path):
    """Output 68x44 (sample frame 136x88: 9x6 workgroup tiles), ss 2, 400
    steps, the default scene; the list has padding and the partial block 5."""
    try:
        setup(gpu, wd, "small", False)
        run_paths(gpu, wd, "small", False, 2, path, 68, 44, 400, (7, 25), 8, [5, 0, -1, 3])
    finally:
        reset(gpu, wd)


# ---- B.
def test_ss1_is_the_plain_frame(gpu, wd):
    import torch

    try:
        setup(gpu, wd, "small", False)
        prm, cam = wd.params(STEPS), wd.cams["view"]
        plain, = host(gpu.render(cam, prm, W, H))
        same(plain, wd.ref("small", False, "view", W, H, STEPS)[0], "sr_render")
        got, = host(gpu.render_ss(cam, prm, W, H, 1))
        assert np.array_equal(got, plain)
        got, = host(gpu.render_ss(cam, prm, W, H, 1, *ROWS))
        assert np.array_equal(got, plain[ROWS[0]:ROWS[1]])
        cams = wd.cam_array(wd.batch)
        a = torch.full((3, len(LIST) * BR, W, 4), FILL, dtype=torch.uint8, device="cuda")
        b = a.clone()
        gpu.render_block_list(cams, prm, W, H, BR, LIST, out=a)
        gpu.render_block_list_ss(cams, prm, W, H, BR, LIST, 1, out=b)
        a, b = host(a, b)
        assert np.array_equal(a, b)
        assert np.array_equal(a[0, 2 * BR:3 * BR], plain[:BR]) and (a[:, BR:2 * BR] == FILL).all()
    finally:
        reset(gpu, wd)


@pytest.mark.parametrize("ss", [2, 3])
def test_padded_pitch_and_frame_stride(gpu, wd, ss):
    """The row band and the block list with pitch 4 W + 32 and a padded frame
    stride into the middle of a sentinel-filled buffer: the payload equals
    the reference; row padding, the -1 slot, the rows past the height, the
    gaps between frames and the guard bands still hold the sentinel."""
    import torch

    abi, lib = wd.pkg.abi, gpu.lib
    prm = wd.params(STEPS)
    cams = wd.cam_array(wd.batch)
    arr = (abi.Camera * 3)(*cams)
    refs = [ss_ref(wd, "small", False, c, ss) for c in wd.batch]
    pitch, guard = 4 * W + 32, 4096

    def run(label, n_frames, source_rows, call):
        rows = len(source_rows)
        stride = pitch * rows + 256
        size = 2 * guard + n_frames * stride
        buf = torch.full((size,), SENTINEL, dtype=torch.uint8, device="cuda")
        want = np.full(size, SENTINEL, dtype=np.uint8)
        for f in range(n_frames):
            for k, y in enumerate(source_rows):
                if y is not None:
                    o = guard + f * stride + k * pitch
                    want[o:o + 4 * W] = refs[f][y].reshape(-1)
        rc = call(C.c_void_p(buf.data_ptr() + guard), stride)
        assert rc == abi.SR_OK, (label, rc)
        got, = host(buf)
        payload = want != SENTINEL
        bad = got != want
        assert not bad.any(), (f"{label}: {int((bad & payload).sum())} payload bytes differ, "
                               f"{int((bad & ~payload).sum())} bytes outside the payload changed")

    try:
        setup(gpu, wd, "small", False)
        st = gpu._stream(None)
        y0, y1 = ROWS
        run(f"ss {ss}, sr_render_ss rows [{y0}, {y1})", 1, list(range(y0, y1)),
            lambda p, stride: lib.sr_render_ss(gpu.ctx, C.byref(cams[0]), C.byref(prm), W, H, y0, y1, ss, p, pitch, st))
        lst = (C.c_int * len(LIST))(*LIST)
        src = [b * BR + j if 0 <= b and b * BR + j < H else None for b in LIST for j in range(BR)]
        assert src.count(None) == BR + 1
        for _ in range(2):
            run(f"ss {ss}, sr_render_block_list_ss", 3, src,
                lambda p, stride: lib.sr_render_block_list_ss(gpu.ctx, arr, 3, C.byref(prm), W, H, BR, lst, len(LIST),
                                                              ss, p, pitch, stride, st))
    finally:
        reset(gpu, wd)


@pytest.mark.parametrize("ss", [2, 3])
def test_two_ranks_priced_lists_assemble_to_the_frame(gpu, wd, ss):
    """Output 20x28 in 8-row blocks: the sample frame's sr_wave_costs map ->
    block_costs -> supersample_block_costs -> balanced_blocks for two ranks;
    each list rendered with sr_render_block_list_ss, the tiles put together
    by sr_assemble_blocks on the device: the whole sr_render_ss frame."""
    import torch

    D = wd.pkg.dist
    w, h = 20, 28
    prm, cam = wd.params(STEPS), wd.cams["view"]
    ref = ss_ref(wd, "small", False, "view", ss, w, h, STEPS)
    try:
        setup(gpu, wd, "small", False)
        waves, = host(gpu.wave_costs(cam, prm, ss * w, ss * h))
        assert waves.shape == ((ss * h + 7) // 8, (ss * w + 7) // 8, 2)
        costs = D.supersample_block_costs(D.block_costs(waves), ss, h)
        assert costs.shape == (4,) and (costs > 0).all()
        lists = D.balanced_blocks(costs, 2)
        assert sorted(b for l in lists for b in l if b >= 0) == [0, 1, 2, 3] and len(lists[0]) == len(lists[1]) == 2
        tiles = torch.stack([gpu.render_block_list_ss([cam], prm, w, h, 8, l, ss) for l in lists])  # [2, 1, 16, w, 4]
        frame = D.assemble_blocks_abi(tiles, lists, h, 8)
        whole = gpu.render_ss(cam, prm, w, h, ss)
        frame, whole = host(frame, whole)
        same(whole, ref, f"ss {ss}, sr_render_ss {w}x{h}")
        same(frame[0], whole, f"ss {ss}, two ranks' tiles reassembled")
    finally:
        reset(gpu, wd)


def test_one_context_on_two_streams(pkg, textures, wd):
    """Plain renders alternating with ss 2, 4, 1, 3 at two output sizes on
    two streams of one context (the sample scratch regrows twice after its
    first allocation, the order cache holds plain and sample shapes, every
    stream change waits on the event recorded after the resolve): each
    result equals a fresh context's render of the same call."""
    import torch

    bg, arr = textures
    prm, cam = wd.params(STEPS), wd.cams["view"]
    A, B = (W, H), (40, 23)
    ops = [(1, A, 0), (2, B, 1), (1, B, 0), (4, A, 1), (1, A, 0), (1, B, 1), (3, B, 0), (2, A, 0), (4, B, 1),
           (1, A, 1), (2, B, 0)]

    def make():
        r = pkg.Renderer(0)
        r.set_background(bg)
        r.set_texture_array(arr)
        r.set_scene(wd.scene("small"))
        return r

    fresh = {}
    for ss, size, _ in ops:
        if (ss, size) not in fresh:
            with make() as r:
                fresh[(ss, size)], = host(r.render_ss(cam, prm, size[0], size[1], ss))
    for (ss, size), img in fresh.items():
        want = ss_ref(wd, "small", False, "view", ss, *size) if ss > 1 else wd.ref("small", False, "view", *size, STEPS)[0]
        same(img, want, f"fresh context, ss {ss}, {size}")
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    with make() as r:
        outs = []
        for i, (ss, size, k) in enumerate(ops):
            if i % 2 == 0:  # the plain entry point and the ss one with ss 1 alternate for the plain frames
                outs.append(r.render_ss(cam, prm, size[0], size[1], ss, stream=streams[k]))
            elif ss == 1:
                outs.append(r.render(cam, prm, size[0], size[1], stream=streams[k]))
            else:
                outs.append(r.render_ss(cam, prm, size[0], size[1], ss, stream=streams[k]))
        got = host(*outs)
        for (ss, size, k), img in zip(ops, got):
            same(img, fresh[(ss, size)], f"ss {ss}, {size}, stream {k}")
        assert r.diag_counters() == {"hit_not_opaque": 0, "free_errors": 0}


@pytest.mark.parametrize("offset", [0, 4, 1], ids=["aligned", "off4", "off1"])
@pytest.mark.parametrize("ss", [2, 3, 4])
@pytest.mark.parametrize("width", [1, 67, 130, 300])
def test_device_resolve_equals_host(pkg, width, ss, offset):
    """sr_resolve_box on the device against its host form on random bytes:
    vector and byte paths (sample pointers offset by 4 bytes, and by 1), two
    frames with padded pitches and strides, nothing outside the payload
    written. 300 pixels: more than one workgroup along the row."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    abi, lib = pkg.abi, pkg.abi.load()
    rows, frames = 5, 2
    rng = np.random.default_rng(width * 100 + ss * 10 + offset)
    samples = rng.integers(0, 256, (frames, ss * rows, ss * width, 4), dtype=np.uint8)
    want_px = abi.resolve_box(samples, ss)
    align = 16 * 3  # keeps every ss's vector alignment when the offset is 0
    sp = (4 * ss * width + align - 1) // align * align + align
    sstride = sp * ss * rows + align
    op, ostride, guard = 4 * width + 8, (4 * width + 8) * rows + 16, 256
    src = np.full(guard + frames * sstride + guard, 0x3C, dtype=np.uint8)
    for f in range(frames):
        for r in range(ss * rows):
            o = guard + offset + f * sstride + r * sp
            src[o:o + 4 * ss * width] = samples[f, r].reshape(-1)
    want = np.full(2 * guard + frames * ostride, SENTINEL, dtype=np.uint8)
    for f in range(frames):
        for r in range(rows):
            o = guard + f * ostride + r * op
            want[o:o + 4 * width] = want_px[f, r].reshape(-1)
    d_src = torch.from_numpy(src).cuda()
    d_out = torch.full((want.size,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert d_src.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.sr_resolve_box(C.c_void_p(d_src.data_ptr() + guard + offset), sp, sstride, width, rows, ss,
                            C.c_void_p(d_out.data_ptr() + guard), op, ostride, frames, 1, st)
    assert rc == abi.SR_OK
    got, back = host(d_out, d_src)
    assert np.array_equal(back, src)
    bad = got != want
    assert not bad.any(), f"{int(bad.sum())} bytes differ from the host form (payload or padding)"


def test_rejections_on_a_live_context(pkg, gpu, wd):
    """Each bad call returns its status before anything is launched or
    written; the good call after them still gives the reference."""
    import torch

    abi, lib = wd.pkg.abi, gpu.lib
    try:
        setup(gpu, wd, "small", False)
        prm, cam = wd.params(STEPS), wd.cams["view"]
        st = gpu._stream(None)
        buf = torch.full((33, len(LIST) * BR, W, 4), SENTINEL, dtype=torch.uint8, device="cuda")
        p, pitch = C.c_void_p(buf.data_ptr()), 4 * W
        stride = pitch * len(LIST) * BR
        cams33 = (abi.Camera * 33)(*[abi.camera_flyby((f + 0.5) / 33.0, 30.0, 10.0) for f in range(33)])
        lst = (C.c_int * len(LIST))(*LIST)

        def frame(ss=2, ctx=gpu.ctx, y0=0, y1=H, pitch_=pitch, out=p):
            return lib.sr_render_ss(ctx, C.byref(cam), C.byref(prm), W, H, y0, y1, ss, out, pitch_, st)

        def blist(ss=2, ctx=gpu.ctx, n=3, l=lst, stride_=stride, br=BR):
            return lib.sr_render_block_list_ss(ctx, cams33, n, C.byref(prm), W, H, br, l, len(LIST), ss, p, pitch,
                                               stride_, st)

        for ss in (0, 5, -1):
            assert frame(ss=ss) == abi.SR_E_INVALID and blist(ss=ss) == abi.SR_E_INVALID, ss
        assert blist(n=33) == abi.SR_E_CAPACITY
        assert blist(n=0) == abi.SR_E_INVALID
        assert frame(y1=H + 1) == abi.SR_E_INVALID and frame(y0=5, y1=4) == abi.SR_E_INVALID
        assert frame(pitch_=pitch - 4) == abi.SR_E_INVALID and frame(out=None) == abi.SR_E_INVALID
        assert blist(stride_=stride - 4) == abi.SR_E_INVALID
        assert blist(l=(C.c_int * 3)(0, 3, 1)) == abi.SR_E_INVALID  # an entry equal to the block count
        assert blist(ss=4, br=(1 << 22) + 1) == abi.SR_E_INVALID  # 4 x 3 x block_rows sample rows > 2^24
        assert frame(ctx=None) == abi.SR_E_INVALID and blist(ctx=None) == abi.SR_E_INVALID
        with pkg.Renderer(0) as empty:  # a context without a scene
            assert frame(ctx=empty.ctx) == abi.SR_E_NOT_READY and blist(ctx=empty.ctx) == abi.SR_E_NOT_READY
            assert frame(ss=1, ctx=empty.ctx) == abi.SR_E_NOT_READY
        assert frame(y0=4, y1=4) == abi.SR_OK  # no rows: nothing is written
        assert (host(buf)[0] == SENTINEL).all()
        got, = host(gpu.render_ss(cam, prm, W, H, 2))
        same(got, ss_ref(wd, "small", False, "view", 2), "the good render after the refused calls")
    finally:
        reset(gpu, wd)


def test_zz_diag_counters_zero(gpu):
    assert gpu.diag_counters() == {"hit_not_opaque": 0, "free_errors": 0}
