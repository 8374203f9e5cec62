"""Shutter frames (sr.h): motion blur and anti-aliasing from one batched launch.

Every written frame equals, byte for byte, shutter_cases' reference: the
rounded mean, in numpy, of the CPU oracle's sub-frames, each a phase image of
the oracle's sample frame of its own scene and camera (the reference's wrong
neighbours differ on at least 10 % of the pixels: tests/test_shutter_cases.py).
The buffers are test_gpu_sequence's Out: filled with a sentinel, with a padded
pitch and frame stride (multiples of 4 only: the resolve kernel's dword path);
the padding, the rows a launch leaves unwritten and everything after a
rejection keep the sentinel. The same launch through Renderer.render_shutter
writes a dense tensor (at widths that are multiples of 4: the vector path).

The cells of (M, K, ss) run at 68x44, 33x17 and 1x1; the sample frames of the
ss 3 and ss 4 cells at 68x44 are the oracle's costliest (27 of 204x132, 32 of
272x176), the GPU's part of every cell is a single launch.
"""
import ctypes as C

import numpy as np
import pytest

import projection_cases as PC
from shutter_cases import OWN, Case, Shutter
from test_gpu_launch_matrix import FILL, LIST, H, W, host, overlay_pixels, same, split_count
from test_gpu_sequence import PAD, Out

pytestmark = pytest.mark.gpu

OK, INV, CAP, NOMEM, NOT_READY = 0, -1, -2, -4, -5
CLEAN = {"hit_not_opaque": 0, "free_errors": 0}
TURNS = ("view", "fly1", "fly5")
SIZES = ((W, H), (33, 17), (1, 1))


@pytest.fixture(scope="module")
def sh(pkg, oracle, textures):
    return Shutter(pkg, oracle, textures)


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


@pytest.fixture(autouse=True)
def settings(gpu, sh):
    """The context state every test starts from and leaves behind."""
    def reset():
        gpu.set_split(0)
        gpu.set_latency_mode(False)
        gpu.set_culling(True)
        gpu.set_projection("rectilinear")
        gpu.set_test_ray(sh.wd.test_rays[False])
    reset()
    yield
    reset()


def phase_bytes(sh, case):
    """The case's explicit pairs as the ABI's bytes, or None for the default ones"""
    if case.phases is None:
        return None
    flat = [int(v) for v in np.asarray(case.phases, dtype=np.uint8).reshape(-1)]
    return (C.c_uint8 * len(flat))(*flat)


def cams_of(gpu, sh, case, n=None):
    n = case.n if n is None else n
    camera = gpu.lib.sr_render_shutter.argtypes[2]._type_  # abi.Camera
    return (camera * max(1, n))(*[sh.cam(c) for c in case.cams[:n]])


def load(gpu, sh, case, overlay=False):
    """The case's scenes on the context (its sequence, or its own scene) and the test ray"""
    gpu.set_test_ray(sh.wd.test_rays[overlay])
    if case.seq is not None:
        gpu.set_scene_sequence(sh.sq.scenes(case.seq))
    else:
        gpu.set_scene(sh.wd.scene(case.own))


def render(gpu, sh, case, prm, w, h, y0=0, y1=None, stream=None, out=None):
    """sr_render_shutter into an Out -> (status, Out)"""
    y1 = h if y1 is None else y1
    out = out or Out(case.M, y1 - y0, w)
    rc = gpu.lib.sr_render_shutter(gpu.ctx, case.first_scene, cams_of(gpu, sh, case), phase_bytes(sh, case), case.K, case.M,
                                   C.byref(prm), w, h, y0, y1, case.ss, out.ptr(), out.pitch, out.stride,
                                   gpu._stream(stream))
    return rc, out


def render_list(gpu, sh, case, prm, w, h, block_rows, blocks):
    out = Out(case.M, len(blocks) * block_rows, w)
    lst = (C.c_int * len(blocks))(*blocks)
    rc = gpu.lib.sr_render_shutter_block_list(gpu.ctx, case.first_scene, cams_of(gpu, sh, case), phase_bytes(sh, case),
                                              case.K, case.M, C.byref(prm), w, h, block_rows, lst, len(blocks), case.ss,
                                              out.ptr(), out.pitch, out.stride, gpu._stream(None))
    return rc, out


def dense(gpu, sh, case, prm, w, h, y0=0, y1=None):
    """The same launch through the Renderer: a dense [M, rows, w, 4] tensor on the host"""
    t = gpu.render_shutter(case.first_scene, [sh.cam(c) for c in case.cams[:case.n]], case.K, prm, w, h, case.ss,
                           None if case.phases is None else [tuple(p) for p in case.phases], y0, h if y1 is None else y1)
    return host(t)[0]


def check(gpu, sh, case, w=W, h=H, overlay=False, y0=0, y1=None, label="", launches=1, prm=None, tag=None, want=None):
    """One shutter call (the last of `launches`) against the reference, padded and dense"""
    y1 = h if y1 is None else y1
    p = prm if prm is not None else sh.sq.params()
    for _ in range(launches):
        rc, out = render(gpu, sh, case, p, w, h, y0, y1)
        assert rc == OK, (label, rc)
    got = out.frames(label)
    if want is None:
        want = sh.reference(case, w, h, overlay, params=prm, tag=tag)
    for m in range(case.M):
        same(got[m], want[m][y0:y1], f"{label} {case.name} frame {m} rows [{y0}, {y1})")
    d = dense(gpu, sh, case, p, w, h, y0, y1)
    for m in range(case.M):
        same(d[m], want[m][y0:y1], f"{label} {case.name} frame {m}, dense")
    return got


# ---- the cells ----------------------------------------------------------------------------

def explicit_32(ss):
    return [((3 * j + 1) % ss, (j // 2 + j // 7) % ss) for j in range(32)]


def non_default_8x4():
    """Per group another order of the 2x2 grid, one group with a phase twice and one with a single phase"""
    groups = [[(0, 1), (1, 0), (1, 1), (0, 0)], [(1, 1), (0, 0), (0, 1), (1, 0)], [(1, 0), (1, 0), (0, 1), (0, 0)],
              [(1, 1), (1, 1), (1, 1), (1, 1)]]
    return [p for g in range(8) for p in groups[g % 4]]


CELLS = {
    "4x4_ss2": lambda: Case("4x4_ss2", 4, 4, 2, ["view"] * 16, seq="ORBIT40"),
    "5x3_ss1": lambda: Case("5x3_ss1", 5, 3, 1, ["view"] * 15, seq="ORBIT40"),
    "3x9_ss3": lambda: Case("3x9_ss3", 3, 9, 3, ["view"] * 27, seq="ORBIT40", first=2),
    "2x16_ss4": lambda: Case("2x16_ss4", 2, 16, 4, ["view"] * 32, seq="ORBIT40", first=8),
    "1x32_ss2_explicit": lambda: Case("1x32_ss2_explicit", 1, 32, 2, ["view"] * 32, seq="ORBIT40", phases=explicit_32(2)),
    "32x1_ss1": lambda: Case("32x1_ss1", 32, 1, 1, ["view"] * 32, seq="ORBIT40", first=5),
    "8x4_ss2_explicit": lambda: Case("8x4_ss2_explicit", 8, 4, 2, ["view"] * 32, seq="ORBIT40",
                                     phases=non_default_8x4()),
}


@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("cell", list(CELLS))
def test_cells(gpu, sh, cell, size):
    w, h = size
    case = CELLS[cell]()
    load(gpu, sh, case)
    check(gpu, sh, case, w, h, label=f"{w}x{h}", launches=2)  # the second launch runs the learned order


# ---- ORBIT40, MIX and the own scene, the overlay off and on ------------------------------------

def scene_case(name):
    """Cameras in turn, "view" (which sees the test ray) among them"""
    if name == "MIX":  # slot counts change per sub-frame: 6, 21, 8, ...
        return Case("mix_2x3_ss2", 2, 3, 2, [TURNS[j % 3] for j in range(6)], seq="MIX")
    if name == "ORBIT40":
        return Case("orbit_3x4_ss2", 3, 4, 2, [TURNS[j % 3] for j in range(12)], seq="ORBIT40", first=11)
    return Case("own_2x4_ss2", 2, 4, 2, [TURNS[j % 3] for j in range(8)], own="general")


@pytest.mark.parametrize("overlay", [False, True], ids=["plain", "overlay"])
@pytest.mark.parametrize("name", ["ORBIT40", "MIX", "own"])
def test_scenes(gpu, sh, name, overlay):
    case = scene_case(name)
    w, h = (W, H) if name != "MIX" and not overlay else (33, 17)  # the oracle's overlay is its slowest part
    load(gpu, sh, case, overlay)
    if overlay:
        seen = sum(overlay_pixels(sh.sample_frame(case, j, case.cams[j], w, h, True)) for j in range(case.n))
        assert seen > 0, "the test ray shows in no sub-frame"
    check(gpu, sh, case, w, h, overlay, label=f"{name} overlay {overlay}")


@pytest.mark.parametrize("name", ["flyby_k4_ss2", "own_k4_ss2"])
def test_moving_camera(gpu, sh, name):
    """The flyby camera at the sub-frames' times, over the sequence and over the own scene."""
    case = sh.case(name)
    load(gpu, sh, case)
    check(gpu, sh, case, label="flyby", launches=2)


# ---- launch paths ---------------------------------------------------------------------------

def test_row_bands(gpu, sh):
    case = sh.case("view_k4_ss2")
    load(gpu, sh, case)
    for y0, y1 in ((5, 6), (7, 25), (40, H)):
        check(gpu, sh, case, y0=y0, y1=y1, label="band")
    rc, out = render(gpu, sh, case, sh.sq.params(), W, H, 9, 9, out=Out(case.M, 1, W))
    assert rc == OK and out.untouched(), "no rows: nothing is written"


def want_list(frame, blocks, w, h):
    want = np.full((len(blocks) * 8, w, 4), FILL, dtype=np.uint8)  # padding and rows past the frame keep the sentinel
    for s, b in enumerate(blocks):
        if b >= 0:
            n = min(8, h - b * 8)
            want[s * 8:s * 8 + n] = frame[b * 8:b * 8 + n]
    return want


def test_padded_block_list(gpu, sh):
    case = sh.case("view_k4_ss2")
    load(gpu, sh, case)
    ref = sh.reference(case)
    for _ in range(2):  # the second launch runs the list's learned order
        rc, out = render_list(gpu, sh, case, sh.sq.params(), W, H, 8, LIST)
        assert rc == OK
    got = out.frames("block list")
    for m in range(case.M):
        same(got[m], want_list(ref[m], LIST, W, H), f"block list frame {m}")
    # dense (the vector path skips the same rows)
    t = gpu.torch.full((case.M, len(LIST) * 8, W, 4), FILL, dtype=gpu.torch.uint8, device="cuda")
    gpu.render_shutter_block_list(case.first_scene, [sh.cam(c) for c in case.cams[:case.n]], case.K, sh.sq.params(), W, H,
                                  8, LIST, case.ss, out=t)
    (d,) = host(t)
    for m in range(case.M):
        same(d[m], want_list(ref[m], LIST, W, H), f"block list frame {m}, dense")


def test_two_ranks_assembled(gpu, sh, pkg):
    """Two ranks' lists of a shutter call, put together by sr_assemble_blocks on the device."""
    import torch

    case = sh.case("view_k3_ss1")
    load(gpu, sh, case)
    lists = [[5, 2, 0, -1], [1, 3, -1, 4]]
    cams = [sh.cam(c) for c in case.cams[:case.n]]
    tiles = [gpu.render_shutter_block_list(case.first_scene, cams, case.K, sh.sq.params(), W, H, 8, lst, case.ss).clone()
             for lst in lists]
    (frames,) = host(pkg.dist.assemble_blocks_abi(torch.stack(tiles), lists, H, 8))
    ref = sh.reference(case)
    for m in range(case.M):
        same(frames[m], ref[m], f"assembled frame {m}")


# ---- launch options -------------------------------------------------------------------------

@pytest.mark.parametrize("option", ["culling_off", "latency_mode", "split_tiles"])
@pytest.mark.parametrize("name", ["view_k4_ss2", "own_k4_ss2"])
def test_launch_options(gpu, sh, name, option):
    case = sh.case(name)
    load(gpu, sh, case)
    if option == "culling_off":
        gpu.set_culling(False)
        check(gpu, sh, case, label=option)
    elif option == "latency_mode":
        gpu.set_latency_mode(True)
        check(gpu, sh, case, label=option)
    else:
        gpu.set_split(4, 16, 1)
        p = sh.sq.params()
        for _ in range(3):
            rc, out = render(gpu, sh, case, p, W, H)
            assert rc == OK
        assert split_count(gpu) == 4 * 4, "the learned order of the shutter launch holds no split tiles"
        got, ref = out.frames(option), sh.reference(case)
        for m in range(case.M):
            same(got[m], ref[m], f"{option} frame {m}")


_PROJ = {}


@pytest.mark.parametrize("projection", [PC.EQUIRECT, PC.FISHEYE], ids=["equirect", "fisheye"])
def test_projections(gpu, sh, pkg, oracle, projection):
    """17x11 at ss 2 against projection_cases' 1x1 method: each sub-frame its own scene, camera and phase."""
    w, h = 17, 11
    case = Case("proj_2x2_ss2", 2, 2, 2, [TURNS[j % 3] for j in range(4)], seq="MIX", first=1)
    load(gpu, sh, case)
    gpu.set_projection(projection)
    ph = sh.phases(case)
    frames = []
    for m in range(case.M):
        subs = []
        for k in range(case.K):
            j = m * case.K + k
            key = (projection, j)
            if key not in _PROJ:
                _PROJ[key] = PC.pixel_frame(pkg, oracle, sh.sq.scenes("MIX")[case.first + j], sh.cam(case.cams[j]),
                                            sh.sq.params(), 2 * w, 2 * h, projection, sh.wd.tex)[0]
            subs.append(_PROJ[key][int(ph[j][1])::2, int(ph[j][0])::2])
        frames.append(sh.resolve(subs))
    check(gpu, sh, case, w, h, label=PC.NAMES[projection], want=np.stack(frames))


PER_SAMPLE = {
    "crosshair": dict(crosshair=1),
    "percent_black": dict(percent_black=0.5),
    "half_width": dict(raytrace_type=2),  # SR_RAYTRACE_HALF_WIDTH
}


@pytest.mark.parametrize("what", list(PER_SAMPLE))
def test_per_sample_evaluation(gpu, sh, what):
    """The crosshair, the noise mask and a split mode are those of each sub-frame's sample frame."""
    w, h = 33, 17
    case = Case("per_sample_2x4_ss2", 2, 4, 2, ["view"] * 8, seq="ORBIT40", first=3)
    prm = sh.sq.params()
    for name, v in PER_SAMPLE[what].items():
        setattr(prm, name, v)
    load(gpu, sh, case)
    want = sh.reference(case, w, h, params=prm, tag=what)
    changed = int((want != sh.reference(case, w, h)).any(-1).sum())
    assert changed > 0, f"{what} leaves the reference unchanged"
    check(gpu, sh, case, w, h, label=f"{what} ({changed} pixels changed)", prm=prm, tag=what)


# ---- the definition's identities, byte for byte -------------------------------------------------

def test_k1_ss1_is_render_sequence(gpu, sh):
    case = Case("seq_6x1", 6, 1, 1, [TURNS[j % 3] for j in range(6)], seq="MIX")
    load(gpu, sh, case)
    prm = sh.sq.params()
    cams = [sh.cam(c) for c in case.cams]
    (seq,) = host(gpu.render_sequence(0, cams, prm, W, H))
    (got,) = host(gpu.render_shutter(0, cams, 1, prm, W, H))
    assert np.array_equal(got, seq)
    gpu.set_scene(sh.wd.scene("general"))
    (batch,) = host(gpu.render_blocks_batch(cams, prm, W, H, H, 0, 1)[0])
    (got,) = host(gpu.render_shutter(OWN, cams, 1, prm, W, H))
    assert np.array_equal(got, batch)


@pytest.mark.parametrize("ss", [2, 3, 4])
def test_one_scene_one_camera_is_render_ss(gpu, sh, ss):
    w, h = 33, 17
    gpu.set_scene(sh.wd.scene("small"))
    prm, cam = sh.sq.params(), sh.cam("view")
    (want,) = host(gpu.render_ss(cam, prm, w, h, ss))
    (got,) = host(gpu.render_shutter(OWN, [cam] * (ss * ss), ss * ss, prm, w, h, ss))
    assert np.array_equal(got[0], want)
    same(want, PC.box_average(sh.wd.ref("small", False, "view", ss * w, ss * h)[0], ss), "sr_render_ss itself")


def test_one_scene_one_camera_is_accumulate_and_resolve(gpu, sh):
    w, h, ss = 33, 17, 3
    gpu.set_scene(sh.wd.scene("general"))
    prm, cam = sh.sq.params(), sh.cam("fly1")
    phases = [(2, 0), (0, 0), (1, 2), (1, 2), (2, 2)]
    acc = gpu.render_accumulate(cam, prm, w, h, ss, phases)
    (want,) = host(gpu.accum_resolve(acc, len(phases)))
    (got,) = host(gpu.render_shutter(OWN, [cam] * 5, 5, prm, w, h, ss, phases))
    assert np.array_equal(got[0], want)


# ---- sr_render_accumulate_shutter ---------------------------------------------------------------

def test_any_grouping_resolves_to_the_shutter_frame(gpu, sh):
    case = sh.case("flyby_k4_ss2")
    load(gpu, sh, case)
    prm = sh.sq.params()
    ref = sh.reference(case)
    order = [tuple(int(v) for v in p) for p in sh.phases(case)]
    m = 2
    j0 = m * case.K
    for groups in ((4,), (1, 3), (2, 2), (1, 1, 1, 1)):
        acc, j = None, j0
        for g in groups:
            cams = [sh.cam(c) for c in case.cams[j:j + g]]
            acc = gpu.accumulate_shutter(case.first + j, cams, prm, W, H, case.ss, order[j:j + g], accum=acc)
            j += g
        (got,) = host(gpu.accum_resolve(acc, case.K))
        same(got, ref[m], f"grouping {groups}")
    # a band, with the default phases of a group's first sub-frames
    cams = [sh.cam(c) for c in case.cams[j0:j0 + case.K]]
    acc = gpu.accumulate_shutter(case.first + j0, cams, prm, W, H, case.ss, None, row_begin=7, row_end=25)
    same(host(gpu.accum_resolve(acc, case.K))[0], ref[m][7:25], "a band")


def test_a_shutter_of_40_sub_frames_over_two_calls(gpu, sh):
    """Longer than one launch holds: 32 + 8 sub-frames, ORBIT40's every scene, against numpy."""
    w, h, ss = 33, 17, 2
    case = Case("long_1x40_ss2", 1, 40, ss, ["view"] * 40, seq="ORBIT40")
    load(gpu, sh, case)
    prm = sh.sq.params()
    ph = [tuple(int(v) for v in p) for p in sh.phases(case)]
    cams = [sh.cam("view")] * 40
    acc = gpu.accumulate_shutter(0, cams[:32], prm, w, h, ss, ph[:32])
    acc = gpu.accumulate_shutter(32, cams[32:], prm, w, h, ss, ph[32:], accum=acc)
    subs = [sh.sub_frame(case, j, w, h) for j in range(40)]
    total = sum(s.astype(np.uint16) for s in subs)
    assert np.array_equal(host(acc)[0].view(np.uint16), total)
    same(host(gpu.accum_resolve(acc, 40))[0], sh.resolve(subs), "40 sub-frames")


# ---- the resolve alone --------------------------------------------------------------------------

@pytest.mark.parametrize("aligned", [True, False], ids=["aligned16", "aligned4"])
def test_device_resolve_equals_host(gpu, pkg, aligned):
    """Widths 1, 3, 4, 5, 17, 68 and K 1, 2, 3, 32 on buffers whose base, pitch
    and strides are multiples of 16 (the vector path and its row tails), and
    of 4 only (the dword path); the padding keeps the sentinel."""
    import torch

    rng = np.random.default_rng(5)
    rows, M = 5, 3
    for w in (1, 3, 4, 5, 17, 68):
        for k in (1, 2, 3, 32):
            img = rng.integers(0, 256, size=(M * k, rows, w, 4), dtype=np.uint8)
            if k == 32:
                img[:k] = 255  # the largest sum
            want = pkg.shutter_resolve(img, k)
            if aligned:
                pitch, opitch = (4 * w + 15) // 16 * 16 + 16, (4 * w + 15) // 16 * 16
                stride, ostride, off = pitch * rows + 32, opitch * rows + 16, 0
            else:
                pitch, opitch = 4 * w + 12, 4 * w + 4
                stride, ostride, off = pitch * rows + 8, opitch * rows + 20, 4
            src = np.full(M * k * stride, FILL, dtype=np.uint8)
            v = src.reshape(M * k, stride)[:, :pitch * rows].reshape(M * k, rows, pitch)
            v[:, :, :4 * w] = img.reshape(M * k, rows, 4 * w)
            d_src = torch.full((src.size + 16,), FILL, dtype=torch.uint8, device="cuda")
            d_src[off:off + src.size] = torch.from_numpy(src).cuda()
            d_out = torch.full((M * ostride + 16,), FILL, dtype=torch.uint8, device="cuda")
            assert d_src.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
            rc = gpu.lib.sr_shutter_resolve(C.c_void_p(d_src.data_ptr() + off), pitch, stride, k, M, w, rows,
                                            C.c_void_p(d_out.data_ptr() + off), opitch, ostride, 1, gpu._stream(None))
            assert rc == OK, (w, k, rc)
            (o,) = host(d_out)
            assert (o[:off] == FILL).all() and (o[off + M * ostride:] == FILL).all(), (w, k, "wrote outside the frames")
            o = o[off:off + M * ostride].reshape(M, ostride)
            assert (o[:, opitch * rows:] == FILL).all(), (w, k, "wrote between the frames")
            o = o[:, :opitch * rows].reshape(M, rows, opitch)
            assert (o[:, :, 4 * w:] == FILL).all(), (w, k, "wrote behind a row")
            got = np.ascontiguousarray(o[:, :, :4 * w]).reshape(M, rows, w, 4)
            assert np.array_equal(got, want), f"width {w}, K {k}: {int((got != want).any(-1).sum())} pixels differ"
    t = torch.from_numpy(img).cuda()
    assert np.array_equal(host(gpu.shutter_resolve(t, 32))[0], want)  # the Renderer's form


# ---- context state ------------------------------------------------------------------------------

def test_context_state_afterwards(gpu, sh, pkg, textures):
    import torch

    case = sh.case("view_k3_ss1")
    load(gpu, sh, case)
    gpu.set_scene(sh.wd.scene("small"))
    prm, cam = sh.sq.params(), sh.cam("view")
    own = Case("own_2x2_ss2", 2, 2, 2, ["view", "fly1", "fly5", "view"], own="small")
    s = gpu._stream(None)
    for c in (case, own):
        gpu.render(cam, prm, W, H)
        assert gpu.can_reshade()
        rc, _ = render(gpu, sh, c, prm, 33, 17)
        assert rc == OK and not gpu.can_reshade()
        buf = torch.full((H, W, 4), FILL, dtype=torch.uint8, device="cuda")
        ids = torch.full((H, W), FILL, dtype=torch.int32, device="cuda")
        assert gpu.lib.sr_reshade(gpu.ctx, C.c_void_p(buf.data_ptr()), 4 * W, 0, s) == NOT_READY
        assert gpu.lib.sr_reshade_debug(gpu.ctx, None, C.c_void_p(buf.data_ptr()), None, s) == NOT_READY
        assert gpu.lib.sr_pick_map(gpu.ctx, C.c_void_p(ids.data_ptr()), 4 * W, 0, s) == NOT_READY
        b, i = host(buf, ids)
        assert (b == FILL).all() and (i == FILL).all()
    gpu.render(cam, prm, W, H)
    acc = gpu.accumulate_shutter(0, [cam] * 3, prm, 33, 17)
    assert not gpu.can_reshade() and acc.shape == (17, 33, 4)
    # the sequence and the own scene survive
    assert gpu.scene_sequence_length() == 40
    (seq,) = host(gpu.render_sequence(7, [cam], prm, W, H))
    same(seq[0], sh.sq.ref("ORBIT40", 7)[0], "the sequence after the shutter calls")
    (plain,) = host(gpu.render(cam, prm, W, H))
    same(plain, sh.wd.ref("small", False)[0], "the own scene after the shutter calls")
    assert gpu.can_reshade()
    bg, arr = textures
    with pkg.Renderer(0) as fresh:
        fresh.set_background(bg)
        fresh.set_texture_array(arr)
        fresh.set_scene(sh.wd.scene("small"))
        assert np.array_equal(host(fresh.render(cam, prm, W, H))[0], plain), "a fresh context's frame"


@pytest.mark.parametrize("streams", [1, 2])
def test_queued_with_a_plain_render(gpu, sh, streams):
    """Two shutter calls and a plain sr_render, queued with no host wait, on one stream and on two."""
    import torch

    a, b = sh.case("view_k4_ss2"), sh.case("view_k3_ss1")
    load(gpu, sh, a)
    gpu.set_scene(sh.wd.scene("general"))
    ss = [torch.cuda.Stream() for _ in range(streams)]
    prm = sh.sq.params()
    plain = torch.full((H, W, 4), FILL, dtype=torch.uint8, device="cuda")
    o1, o2 = Out(a.M, H, W), Out(b.M, H, W)
    torch.cuda.synchronize()  # the buffers are filled: the launches below run on streams of their own
    rc1, _ = render(gpu, sh, a, prm, W, H, stream=ss[0], out=o1)
    gpu.render(sh.cam("fly1"), prm, W, H, out=plain, stream=ss[-1])
    rc2, _ = render(gpu, sh, b, prm, W, H, stream=ss[0], out=o2)
    assert (rc1, rc2) == (OK, OK)
    g1, g2 = o1.frames("first"), o2.frames("second")
    for m in range(a.M):
        same(g1[m], sh.reference(a)[m], f"first call frame {m}")
    for m in range(b.M):
        same(g2[m], sh.reference(b)[m], f"second call frame {m}")
    same(host(plain)[0], sh.wd.ref("general", False, "fly1")[0], "the plain render between them")


def test_interleaved_with_the_other_launch_kinds(gpu, sh):
    """A shutter call between the other kinds on one context: each finds its own scratch and order."""
    case = sh.case("view_k4_ss2")
    load(gpu, sh, case)
    gpu.set_scene(sh.wd.scene("small"))
    prm, cam = sh.sq.params(), sh.cam("view")
    ref = sh.reference(case, 33, 17)
    small2 = PC.box_average(sh.wd.ref("small", False, "view", 66, 34)[0], 2)

    def shutter():
        got = dense(gpu, sh, case, prm, 33, 17)
        for m in range(case.M):
            same(got[m], ref[m], f"shutter frame {m}")

    (adaptive,) = host(gpu.render_adaptive(cam, prm, 33, 17, 2, 16)[0])
    shutter()
    same(host(gpu.render_ss(cam, prm, 33, 17, 2))[0], small2, "sr_render_ss")
    shutter()
    acc = gpu.render_accumulate(cam, prm, 33, 17, 2, [(0, 0), (1, 1), (1, 0), (0, 1)])
    shutter()
    same(host(gpu.accum_resolve(acc, 4))[0], small2, "sr_render_accumulate around a shutter call")
    same(host(gpu.render_sequence(3, [cam], prm, 33, 17, ss=2))[0][0],
         PC.box_average(sh.sq.ref("ORBIT40", 3, False, "view", 66, 34)[0], 2), "sr_render_sequence ss 2")
    shutter()
    out, _ = gpu.render_adaptive(cam, prm, 33, 17, 2, 16)
    shutter()
    same(host(out)[0], adaptive, "sr_render_adaptive before and after the shutter calls")
    same(host(gpu.render(cam, prm, 33, 17))[0], sh.wd.ref("small", False, "view", 33, 17)[0], "sr_render")


# ---- rejections -----------------------------------------------------------------------------------

def live_context(gpu, sh):
    """A sequence of 40 scenes and an own scene on the context -> (case, params, camera)"""
    case = sh.case("view_k3_ss1")
    load(gpu, sh, case)
    gpu.set_scene(sh.wd.scene("small"))
    return case, sh.sq.params(), sh.cam("view")


def test_rejections_write_nothing(gpu, sh, pkg):
    case, prm, cam = live_context(gpu, sh)

    def call(first=1, n_cams=6, K=3, M=2, prm=prm, w=W, h=H, y0=0, y1=H, ss=2, phases=None, pitch=None, stride=None,
             null_out=False, null_cams=False, ctx=None, off=0):
        out = Out(min(max(M, 1), 33), max(y1 - y0, 1), w)
        camera = gpu.lib.sr_render_shutter.argtypes[2]._type_
        arr = (camera * max(1, n_cams))(*([cam] * n_cams))
        ph = None if phases is None else (C.c_uint8 * len(phases))(*phases)
        rc = gpu.lib.sr_render_shutter(gpu.ctx if ctx is None else ctx, first, None if null_cams else arr, ph, K, M,
                                       C.byref(prm), w, h, y0, y1, ss,
                                       None if null_out else C.c_void_p(out.t.data_ptr() + off),
                                       out.pitch if pitch is None else pitch, out.stride if stride is None else stride,
                                       gpu._stream(None))
        assert out.untouched(), "a rejected call wrote pixels"
        return rc

    bad_prm = sh.sq.params()
    bad_prm.max_steps = -1
    assert call(K=0) == INV
    assert call(M=0) == INV
    assert call(K=-1) == INV
    assert call(null_cams=True) == INV
    assert call(null_out=True) == INV
    assert call(first=-2) == INV
    assert call(first=35) == INV  # 35 + 6 > 40
    assert call(first=40) == INV
    assert call(K=11, M=3, n_cams=33) == CAP
    assert call(K=33, M=1, n_cams=33) == CAP
    assert call(K=1, M=33, n_cams=33) == CAP
    assert call(K=1 << 20, M=1 << 20) == CAP  # the product does not wrap
    assert call(ss=0) == INV
    assert call(ss=5) == INV
    assert call(phases=[0, 0, 1, 1, 2, 0, 0, 1, 1, 0, 0, 0]) == INV  # a phase >= ss
    assert call(ss=1, phases=[0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0]) == INV
    assert call(prm=bad_prm) == INV
    assert call(w=0) == INV
    assert call(y0=3, y1=2) == INV
    assert call(y1=H + 1) == INV
    assert call(pitch=4 * W - 4) == INV
    assert call(pitch=4 * W + 2) == INV
    assert call(stride=(4 * W + PAD) * H - 4) == INV
    assert call(off=1) == INV

    # not ready: a context without a sequence, or (own scene) without sr_set_scene
    with pkg.Renderer(0) as r:  # (no textures: nothing is launched on it)
        assert call(ctx=r.ctx) == NOT_READY
        assert call(ctx=r.ctx, first=OWN) == NOT_READY
        r.set_scene(sh.wd.scene("small"))
        assert call(ctx=r.ctx) == NOT_READY
        r.set_scene_sequence(sh.sq.scenes("ORBIT40")[:8])
        assert call(ctx=r.ctx, first=3) == INV  # 3 + 6 > 8
        assert r.diag_counters() == CLEAN
    check(gpu, sh, case, 33, 17, label="after the rejections")


def test_block_list_and_accumulate_rejections_write_nothing(gpu, sh):
    case, prm, cam = live_context(gpu, sh)

    def lst(first=1, blocks=(0, 1), block_rows=8, ss=2, n_blocks=None, K=3, M=2):
        out = Out(max(M, 1), len(blocks) * max(block_rows, 1), W)
        camera = gpu.lib.sr_render_shutter.argtypes[2]._type_
        arr = (camera * 32)(*([cam] * 32))
        bl = (C.c_int * len(blocks))(*blocks)
        rc = gpu.lib.sr_render_shutter_block_list(gpu.ctx, first, arr, None, K, M, C.byref(prm), W, H, block_rows, bl,
                                                  len(blocks) if n_blocks is None else n_blocks, ss, out.ptr(), out.pitch,
                                                  out.stride, gpu._stream(None))
        assert out.untouched(), "a rejected call wrote pixels"
        return rc

    assert lst(first=35) == INV
    assert lst(first=-2) == INV
    assert lst(blocks=(0, 6)) == INV  # the frame has six 8-row blocks: 0 .. 5
    assert lst(blocks=(0, -2)) == INV
    assert lst(block_rows=0) == INV
    assert lst(n_blocks=0) == INV
    assert lst(ss=5) == INV
    assert lst(K=0) == INV
    assert lst(K=8, M=5) == CAP

    import torch

    def accum(first=1, n_sub=3, ss=2, y0=0, y1=H, apitch=8 * W, off=0, null=False, phases=None):
        acc = torch.full((H * 8 * W + 16,), FILL, dtype=torch.uint8, device="cuda")
        camera = gpu.lib.sr_render_shutter.argtypes[2]._type_
        arr = (camera * 40)(*([cam] * 40))
        ph = None if phases is None else (C.c_uint8 * len(phases))(*phases)
        rc = gpu.lib.sr_render_accumulate_shutter(gpu.ctx, first, arr, ph, n_sub, C.byref(prm), W, H, y0, y1, ss, 1,
                                                  None if null else C.c_void_p(acc.data_ptr() + off), apitch,
                                                  gpu._stream(None))
        assert (host(acc)[0] == FILL).all(), "a rejected call wrote to the accumulator"
        return rc

    assert accum(n_sub=0) == INV
    assert accum(n_sub=33) == CAP
    assert accum(first=38) == INV
    assert accum(first=-2) == INV
    assert accum(ss=0) == INV
    assert accum(null=True) == INV
    assert accum(apitch=8 * W - 8) == INV
    assert accum(apitch=8 * W + 4) == INV
    assert accum(off=4) == INV
    assert accum(y1=H + 1) == INV
    assert accum(phases=[0, 0, 2, 0, 0, 0]) == INV
    check(gpu, sh, case, 33, 17, label="after the rejections")


def test_zz_diag_counters_stay_zero(gpu):
    assert gpu.diag_counters() == CLEAN
