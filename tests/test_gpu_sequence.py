"""Scene sequences (sr.h): one launch renders frames of different scenes.

Every written frame equals, bit for bit, the CPU oracle's frame of its own
scene and camera (tests/sequence_cases.py; its frames differ pairwise, so a
kernel that read a neighbour's scene fails). The buffers are filled with a
sentinel and have a padded pitch and frame stride: the padding, the rows a
launch leaves unwritten and everything after a rejection keep the sentinel.
"""
import ctypes as C

import numpy as np
import pytest

import projection_cases as PC
from sequence_cases import MIX, Sequences
from test_gpu_launch_matrix import FILL, LIST, H, W, compare, host, overlay_pixels, same, split_count

pytestmark = pytest.mark.gpu

OK, INV, CAP, NOT_READY = 0, -1, -2, -5
PAD, TAIL = 12, 40  # bytes behind each row and each frame
TURNS = ("view", "fly1", "fly5")
WINDOWS = ((0, 6), (1, 3), (0, 1), (5, 1))


@pytest.fixture(scope="module")
def sq(pkg, oracle, textures):
    return Sequences(pkg, oracle, textures)


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
def settings(gpu, sq):
    """The context state every test starts from and leaves behind."""
    def reset():
        gpu.set_split(0)
        gpu.set_latency_mode(False)
        gpu.set_culling(True)
        gpu.set_projection("rectilinear")
        gpu.set_test_ray(sq.wd.test_rays[False])
    reset()
    yield
    reset()


def cams_of(sq, names, n):
    return [sq.wd.cams[names[f % len(names)]] for f in range(n)]


class Out:
    """A sentinel-filled device buffer of n frames of `rows` rows with padded pitch and stride."""

    def __init__(self, n, rows, w):
        import torch

        self.n, self.rows, self.w = n, rows, w
        self.pitch = 4 * w + PAD
        self.stride = self.pitch * rows + TAIL
        self.t = torch.full((max(1, n) * self.stride,), FILL, dtype=torch.uint8, device="cuda")

    def ptr(self):
        return C.c_void_p(self.t.data_ptr())

    def frames(self, label):
        """[n, rows, w, 4] on the host, once every padding byte is seen to hold the sentinel."""
        (a,) = host(self.t)
        a = a.reshape(max(1, self.n), self.stride)[:self.n]
        assert (a[:, self.pitch * self.rows:] == FILL).all(), f"{label}: wrote between the frames"
        a = a[:, :self.pitch * self.rows].reshape(self.n, self.rows, self.pitch)
        assert (a[:, :, 4 * self.w:] == FILL).all(), f"{label}: wrote behind a row"
        return np.ascontiguousarray(a[:, :, :4 * self.w]).reshape(self.n, self.rows, self.w, 4)

    def untouched(self):
        (a,) = host(self.t)
        return bool((a == FILL).all())


def stream_ptr(gpu, stream=None):
    return gpu._stream(stream)


def cam_array(gpu, cams):
    camera = gpu.lib.sr_render_sequence.argtypes[2]._type_  # abi.Camera
    return (camera * max(1, len(cams)))(*cams)


def render(gpu, first, cams, prm, w, h, y0=0, y1=None, ss=1, stream=None, out=None):
    """sr_render_sequence into an Out -> (status, Out)"""
    y1 = h if y1 is None else y1
    n = len(cams)
    out = out or Out(n, y1 - y0, w)
    arr = cam_array(gpu, cams)
    rc = gpu.lib.sr_render_sequence(gpu.ctx, first, arr, n, C.byref(prm), w, h, y0, y1, ss, out.ptr(), out.pitch,
                                    out.stride, stream_ptr(gpu, stream))
    return rc, out


def render_list(gpu, first, cams, prm, w, h, block_rows, blocks, ss=1):
    n = len(cams)
    out = Out(n, len(blocks) * block_rows, w)
    arr = cam_array(gpu, cams)
    lst = (C.c_int * len(blocks))(*blocks)
    rc = gpu.lib.sr_render_sequence_block_list(gpu.ctx, first, arr, n, C.byref(prm), w, h, block_rows, lst, len(blocks),
                                               ss, out.ptr(), out.pitch, out.stride, stream_ptr(gpu))
    return rc, out


def check_window(gpu, sq, name, first, n, turns, overlay=False, w=W, h=H, y0=0, y1=None, label="", launches=1):
    y1 = h if y1 is None else y1
    names = [turns[f % len(turns)] for f in range(n)]
    for _ in range(launches):
        rc, out = render(gpu, first, cams_of(sq, turns, n), sq.params(), w, h, y0, y1)
        assert rc == OK, (label, rc)
    got = out.frames(label)
    for f in range(n):
        want = sq.ref(name, first + f, overlay, names[f], w, h)[0][y0:y1]
        same(got[f], want, f"{label} {name}[{first}+{f}] cam {names[f]} rows [{y0}, {y1})")
    return got


# ---- windows and sizes ------------------------------------------------------------------

@pytest.mark.parametrize("overlay", [False, True], ids=["plain", "overlay"])
def test_mix_windows(gpu, sq, overlay):
    """MIX: slot, cylinder and object counts change from frame to frame; one
    frame has every ray resumed, one no objects. One camera for all frames,
    then three in turn. The window of the small scene alone runs the small
    layout, the one that also holds the large scene all slots: the frame they
    share is the same."""
    gpu.set_test_ray(sq.wd.test_rays[overlay])
    gpu.set_scene_sequence(sq.scenes("MIX"))
    assert gpu.scene_sequence_length() == len(MIX)
    if overlay:
        assert overlay_pixels(sq.ref("MIX", 5, True)[0]) > 0
    got = {}
    for turns in (("view",), TURNS):
        for first, n in WINDOWS:
            got[turns, first, n] = check_window(gpu, sq, "MIX", first, n, turns, overlay, label=f"window ({first}, {n})")
    for turns in (("view",), TURNS):
        same(got[turns, 0, 1][0], got[turns, 0, 6][0], "the small scene alone against the window with the large one")


@pytest.mark.parametrize("name,first", [("GEO8", 0), ("SHADE8", 0), ("ORBIT40", 17)])
def test_moving_scenes(gpu, sq, name, first):
    gpu.set_scene_sequence(sq.scenes(name))
    check_window(gpu, sq, name, first, 8, ("view",), label=name, launches=2)  # the second runs the learned order
    check_window(gpu, sq, name, first, 8, TURNS, label=name + " cameras in turn")


def test_full_batch_and_one_more(gpu, sq):
    """32 frames of ORBIT40 in one launch at 17x11; 33 are refused."""
    gpu.set_scene_sequence(sq.scenes("ORBIT40"))
    check_window(gpu, sq, "ORBIT40", 5, 32, ("view",), w=17, h=11, label="32 frames")
    rc, out = render(gpu, 5, cams_of(sq, ("view",), 33), sq.params(), 17, 11)
    assert rc == CAP and out.untouched()


# ---- launch paths and settings ----------------------------------------------------------

def test_row_bands(gpu, sq):
    gpu.set_scene_sequence(sq.scenes("MIX"))
    for y0, y1 in ((5, 6), (7, 25), (40, H)):
        check_window(gpu, sq, "MIX", 0, 6, TURNS, y0=y0, y1=y1, label="band")


def want_list(sq, name, k, cam, blocks, w=W, h=H):
    want = np.full((len(blocks) * 8, w, 4), FILL, dtype=np.uint8)  # padding and rows past the frame keep the sentinel
    rb = sq.ref(name, k, False, cam, w, h)[0]
    for s, b in enumerate(blocks):
        if b >= 0:
            n = min(8, h - b * 8)
            want[s * 8:s * 8 + n] = rb[b * 8:b * 8 + n]
    return want


def test_padded_block_list(gpu, sq):
    gpu.set_scene_sequence(sq.scenes("MIX"))
    for _ in range(2):  # the second launch runs the list's learned order
        rc, out = render_list(gpu, 0, cams_of(sq, TURNS, 6), sq.params(), W, H, 8, LIST)
        assert rc == OK
    got = out.frames("block list")
    for f in range(6):
        same(got[f], want_list(sq, "MIX", f, TURNS[f % 3], LIST), f"block list frame {f}")


def test_two_ranks_assembled(gpu, sq, pkg):
    """Two ranks' lists of a sequence launch, put together by sr_assemble_blocks."""
    import torch

    gpu.set_scene_sequence(sq.scenes("ORBIT40"))
    lists = [[5, 2, 0, -1], [1, 3, -1, 4]]
    cams = cams_of(sq, TURNS, 4)
    tiles = []
    for lst in lists:
        t = gpu.render_sequence_block_list(20, cams, sq.params(), W, H, 8, lst)
        tiles.append(t.clone())
    frames = pkg.dist.assemble_blocks_abi(torch.stack(tiles), lists, H, 8)
    (frames,) = host(frames)
    for f in range(4):
        same(frames[f], sq.ref("ORBIT40", 20 + f, False, TURNS[f % 3])[0], f"assembled frame {f}")


@pytest.mark.parametrize("ss", [2, 3])
def test_supersample(gpu, sq, ss):
    """ss through launch_ss: the sample frame is a sequence launch, the resolve numpy's box average."""
    w, h = 17, 11
    gpu.set_scene_sequence(sq.scenes("MIX"))
    want = [PC.box_average(sq.ref("MIX", k, False, TURNS[k % 3], ss * w, ss * h)[0], ss) for k in range(6)]
    rc, out = render(gpu, 0, cams_of(sq, TURNS, 6), sq.params(), w, h, ss=ss)
    assert rc == OK
    got = out.frames(f"ss {ss}")
    for k in range(6):
        same(got[k], want[k], f"ss {ss} frame {k}")
    rc, out = render(gpu, 1, cams_of(sq, TURNS, 4)[1:], sq.params(), w, h, 3, 9, ss=ss)  # frame k's camera, k = 1 .. 3
    assert rc == OK
    got = out.frames(f"ss {ss} band")
    for f in range(3):
        same(got[f], want[1 + f][3:9], f"ss {ss} band frame {f}")
    blocks = [1, -1, 0]
    rc, out = render_list(gpu, 0, cams_of(sq, TURNS, 6), sq.params(), w, h, 8, blocks, ss=ss)
    assert rc == OK
    got = out.frames(f"ss {ss} block list")
    for k in range(6):
        exp = np.full((24, w, 4), FILL, dtype=np.uint8)
        exp[0:3] = want[k][8:11]
        exp[16:24] = want[k][0:8]
        same(got[k], exp, f"ss {ss} block list frame {k}")


def test_culling_off(gpu, sq):
    gpu.set_scene_sequence(sq.scenes("MIX"))
    gpu.set_culling(False)
    check_window(gpu, sq, "MIX", 0, 6, TURNS, label="culling off")


def test_latency_mode(gpu, sq):
    """The default unroll under sequences: the same pixels."""
    gpu.set_scene_sequence(sq.scenes("MIX"))
    gpu.set_latency_mode(True)
    check_window(gpu, sq, "MIX", 0, 1, ("view",), label="latency mode, small")
    check_window(gpu, sq, "MIX", 0, 6, TURNS, label="latency mode")


def test_split_tiles(gpu, sq):
    gpu.set_scene_sequence(sq.scenes("MIX"))
    gpu.set_split(4, 16, 1)
    check_window(gpu, sq, "MIX", 0, 6, TURNS, label="split tiles", launches=3)
    assert split_count(gpu) == 4 * 4, "the learned order of the sequence launch holds no split tiles"


_PROJ = {}


@pytest.mark.parametrize("projection", [PC.EQUIRECT, PC.FISHEYE], ids=["equirect", "fisheye"])
def test_projections(gpu, sq, pkg, oracle, projection):
    """33x17 against projection_cases' 1x1 method, each frame with its own scene."""
    w, h = 33, 17
    gpu.set_scene_sequence(sq.scenes("MIX"))
    gpu.set_projection(projection)
    rc, out = render(gpu, 0, cams_of(sq, TURNS, 6), sq.params(), w, h)
    assert rc == OK
    got = out.frames("projected")
    for k in range(6):
        key = (projection, k)
        if key not in _PROJ:
            _PROJ[key] = PC.pixel_frame(pkg, oracle, sq.scenes("MIX")[k], sq.wd.cams[TURNS[k % 3]], sq.params(), w, h,
                                        projection, sq.wd.tex)[0]
        same(got[k], _PROJ[key], f"{PC.NAMES[projection]} frame {k}")


@pytest.mark.parametrize("overlay", [False, True], ids=["plain", "overlay"])
def test_debug_of_every_mix_scene(gpu, sq, overlay):
    gpu.set_test_ray(sq.wd.test_rays[overlay])
    gpu.set_scene_sequence(sq.scenes("MIX"))
    for k in range(len(MIX)):
        f, b, s = host(*gpu.render_sequence_debug(k, sq.wd.cams["view"], sq.params(), W, H))
        compare((b, f, s), sq.ref("MIX", k, overlay), f"render_sequence_debug of MIX[{k}]")
    f, b, s = host(*gpu.render_sequence_debug(3, sq.wd.cams["fly1"], sq.params(), W, H, 7, 25))
    compare((b, f, s), tuple(a[7:25] for a in sq.ref("MIX", 3, overlay, "fly1")), "render_sequence_debug rows [7, 25)")


# ---- ordering and context state -----------------------------------------------------------

@pytest.mark.parametrize("streams", [1, 2])
def test_queued_with_a_plain_render(gpu, sq, streams):
    """Two sequence launches and a plain sr_render of the context's own scene
    (another one), queued with no host wait, on one stream and on two."""
    import torch

    gpu.set_scene_sequence(sq.scenes("ORBIT40"))
    gpu.set_scene(sq.wd.scene("general"))
    ss = [torch.cuda.Stream() for _ in range(streams)]
    prm = sq.params()
    plain = torch.full((H, W, 4), FILL, dtype=torch.uint8, device="cuda")
    o1, o2, o3 = Out(5, H, W), Out(7, H, W), Out(2, 11, 17)
    torch.cuda.synchronize()  # the buffers are filled: the launches below run on streams of their own
    rc1, _ = render(gpu, 3, cams_of(sq, TURNS, 5), prm, W, H, stream=ss[0], out=o1)
    rc2, _ = render(gpu, 30, cams_of(sq, ("fly5", "view"), 7), prm, W, H, stream=ss[-1], out=o2)
    gpu.render(sq.wd.cams["fly1"], prm, W, H, out=plain, stream=ss[0])
    rc3, _ = render(gpu, 0, cams_of(sq, ("view",), 2), prm, 17, 11, stream=ss[-1], out=o3)
    assert (rc1, rc2, rc3) == (OK, OK, OK)
    g1, g2, g3 = o1.frames("first"), o2.frames("second"), o3.frames("third")
    for f in range(5):
        same(g1[f], sq.ref("ORBIT40", 3 + f, False, TURNS[f % 3])[0], f"first launch frame {f}")
    for f in range(7):
        same(g2[f], sq.ref("ORBIT40", 30 + f, False, ("fly5", "view")[f % 2])[0], f"second launch frame {f}")
    for f in range(2):
        same(g3[f], sq.ref("ORBIT40", f, False, "view", 17, 11)[0], f"third launch frame {f}")
    same(host(plain)[0], sq.wd.ref("general", False, "fly1")[0], "the plain render between them")


def test_test_ray_after_the_sequence(gpu, sq):
    """sr_set_test_ray packs the sequence's test-ray part again."""
    gpu.set_scene_sequence(sq.scenes("MIX"))
    check_window(gpu, sq, "MIX", 0, 6, ("view",), False, label="before")
    gpu.set_test_ray(sq.wd.test_rays[True])
    assert overlay_pixels(sq.ref("MIX", 0, True)[0]) > 0
    check_window(gpu, sq, "MIX", 0, 6, ("view",), True, label="after sr_set_test_ray")
    gpu.set_test_ray(sq.wd.test_rays[False])
    check_window(gpu, sq, "MIX", 0, 6, ("view",), False, label="and back")


def test_replace_clear_and_independence(gpu, sq):
    """A new sequence replaces the old one, n == 0 clears it; the sequence and
    the context's own scene do not touch each other."""
    gpu.set_scene(sq.wd.scene("stacked"))
    gpu.set_scene_sequence(sq.scenes("GEO8"))
    check_window(gpu, sq, "GEO8", 2, 4, ("view",), label="GEO8")
    gpu.set_scene_sequence(sq.scenes("SHADE8"))
    assert gpu.scene_sequence_length() == 8
    check_window(gpu, sq, "SHADE8", 2, 4, ("view",), label="SHADE8 in GEO8's place")
    gpu.set_scene(sq.wd.scene("general"))  # leaves the sequence alone
    check_window(gpu, sq, "SHADE8", 0, 8, ("view",), label="after sr_set_scene")
    (plain,) = host(gpu.render(sq.wd.cams["view"], sq.params(), W, H))
    same(plain, sq.wd.ref("general", False)[0], "the context's own scene")
    gpu.set_scene_sequence([])
    assert gpu.scene_sequence_length() == 0
    rc, out = render(gpu, 0, cams_of(sq, ("view",), 1), sq.params(), W, H)
    assert rc == NOT_READY and out.untouched()
    (plain,) = host(gpu.render(sq.wd.cams["view"], sq.params(), W, H))
    same(plain, sq.wd.ref("general", False)[0], "the context's own scene after the sequence went")


def test_sequence_without_set_scene(pkg, sq, textures):
    """sr_set_scene is not required; a context without a sequence is not ready."""
    bg, arr = textures
    with pkg.Renderer(0) as r:
        r.set_background(bg)
        r.set_texture_array(arr)
        rc, out = render(r, 0, cams_of(sq, ("view",), 1), sq.params(), 17, 11)
        assert rc == NOT_READY and out.untouched()
        r.set_scene_sequence(sq.scenes("GEO8"))
        check_window(r, sq, "GEO8", 0, 8, ("view",), w=17, h=11, label="no sr_set_scene")
        assert r.diag_counters() == {"hit_not_opaque": 0, "free_errors": 0}


# ---- rejections and diagnostics -----------------------------------------------------------

def test_rejected_scene_keeps_the_old_sequence(gpu, sq, pkg):
    abi = pkg.abi
    gpu.set_scene_sequence(sq.scenes("SHADE8"))
    bad = [PC.copy_struct(pkg, abi.Scene, s) for s in sq.scenes("GEO8")[:4]]
    bad[2].num_objects = abi.MAX_OBJECTS + 1
    arr = (abi.Scene * 4)(*bad)
    rc = gpu.lib.sr_set_scene_sequence(gpu.ctx, arr, 4)
    assert rc in (INV, CAP) and rc == gpu.lib.sr_set_scene(gpu.ctx, C.byref(bad[2]))
    many = (abi.Scene * (abi.MAX_SEQUENCE + 1))()
    assert gpu.lib.sr_set_scene_sequence(gpu.ctx, many, abi.MAX_SEQUENCE + 1) == CAP
    assert gpu.lib.sr_set_scene_sequence(gpu.ctx, None, 3) == INV
    assert gpu.lib.sr_set_scene_sequence(gpu.ctx, arr, -1) == INV
    assert gpu.scene_sequence_length() == 8
    check_window(gpu, sq, "SHADE8", 0, 8, ("view",), label="the old sequence")


def test_rejections_write_nothing(gpu, sq):
    gpu.set_scene_sequence(sq.scenes("MIX"))
    prm, cams = sq.params(), cams_of(sq, TURNS, 3)

    def seq(first=1, cams=cams, prm=prm, w=W, h=H, y0=0, y1=H, ss=1, pitch=None, stride=None, null_out=False):
        out = Out(len(cams), max(y1 - y0, 1), w)
        arr = cam_array(gpu, cams)
        rc = gpu.lib.sr_render_sequence(gpu.ctx, first, arr if cams else None, len(cams), C.byref(prm), w, h, y0, y1, ss,
                                        None if null_out else out.ptr(), out.pitch if pitch is None else pitch,
                                        out.stride if stride is None else stride, stream_ptr(gpu))
        assert out.untouched(), "a rejected launch wrote pixels"
        return rc

    bad_prm = sq.params()
    bad_prm.max_steps = -1
    assert seq(first=-1) == INV
    assert seq(first=4) == INV  # 4 + 3 > 6
    assert seq(first=6) == INV
    assert seq(first=0, cams=cams_of(sq, TURNS, 33)) == INV  # leaves the sequence (and is above 32 frames)
    assert seq(cams=[]) == INV
    assert seq(prm=bad_prm) == INV
    assert seq(y0=3, y1=2) == INV
    assert seq(y1=H + 1) == INV
    assert seq(ss=0) == INV
    assert seq(ss=5) == INV
    assert seq(pitch=4 * W - 4) == INV
    assert seq(stride=(4 * W + PAD) * H - 4) == INV
    assert seq(ss=2, pitch=4 * W - 4) == INV
    assert seq(ss=2, stride=(4 * W + PAD) * H - 4) == INV
    assert seq(null_out=True) == INV
    assert seq(w=0) == INV

    def lst(first=1, blocks=(0, 1), block_rows=8, ss=1, n_blocks=None):
        out = Out(3, len(blocks) * max(block_rows, 1), W)
        arr = cam_array(gpu, cams)
        bl = (C.c_int * len(blocks))(*blocks)
        rc = gpu.lib.sr_render_sequence_block_list(gpu.ctx, first, arr, 3, C.byref(prm), W, H, block_rows, bl,
                                                   len(blocks) if n_blocks is None else n_blocks, ss, out.ptr(),
                                                   out.pitch, out.stride, stream_ptr(gpu))
        assert out.untouched(), "a rejected launch wrote pixels"
        return rc

    assert lst(first=4) == INV
    assert lst(first=-2) == INV
    assert lst(blocks=(0, 6)) == INV  # the frame has six 8-row blocks: 0 .. 5
    assert lst(blocks=(0, -2)) == INV
    assert lst(block_rows=0) == INV
    assert lst(n_blocks=0) == INV
    assert lst(ss=5) == INV
    assert lst(ss=2, first=5) == INV
    # the debug call
    cam = sq.wd.cams["view"]
    assert gpu.lib.sr_render_sequence_debug(gpu.ctx, 6, C.byref(cam), C.byref(prm), W, H, 0, H, None, Out(1, H, W).ptr(),
                                            None, stream_ptr(gpu)) == INV
    assert gpu.lib.sr_render_sequence_debug(gpu.ctx, 0, C.byref(cam), C.byref(prm), W, H, 0, H, None, None, None,
                                            stream_ptr(gpu)) == INV
    check_window(gpu, sq, "MIX", 1, 3, TURNS, label="after the rejections")


def test_no_retained_frame(gpu, sq):
    import torch

    gpu.set_scene(sq.wd.scene("small"))
    gpu.set_scene_sequence(sq.scenes("MIX"))
    prm, cam = sq.params(), sq.wd.cams["view"]
    gpu.render(cam, prm, W, H)
    assert gpu.can_reshade()
    gpu.set_scene_sequence(sq.scenes("MIX"))  # does not drop the plain launch's retained frame
    assert gpu.can_reshade()
    rc, out = render(gpu, 6, [cam], prm, W, H)  # nor does a rejected sequence launch
    assert rc == INV and gpu.can_reshade()
    for launch in (lambda: render(gpu, 0, cams_of(sq, TURNS, 6), prm, W, H)[0],
                   lambda: render(gpu, 0, cams_of(sq, TURNS, 2), prm, 17, 11, ss=2)[0],
                   lambda: render_list(gpu, 0, cams_of(sq, TURNS, 2), prm, W, H, 8, LIST)[0]):
        gpu.render(cam, prm, W, H)
        assert gpu.can_reshade()
        assert launch() == OK
        assert not gpu.can_reshade()
        buf = torch.full((H, W, 4), FILL, dtype=torch.uint8, device="cuda")
        ids = torch.full((H, W), FILL, dtype=torch.int32, device="cuda")
        s = stream_ptr(gpu)
        assert gpu.lib.sr_reshade(gpu.ctx, C.c_void_p(buf.data_ptr()), 4 * W, 0, s) == NOT_READY
        assert gpu.lib.sr_reshade_debug(gpu.ctx, None, C.c_void_p(buf.data_ptr()), None, s) == NOT_READY
        assert gpu.lib.sr_pick_map(gpu.ctx, C.c_void_p(ids.data_ptr()), 4 * W, 0, s) == NOT_READY
        b, i = host(buf, ids)
        assert (b == FILL).all() and (i == FILL).all()
    gpu.render(cam, prm, W, H)  # a plain launch brings the retained frame back
    assert gpu.can_reshade()
    (again,) = host(gpu.reshade())
    same(again, sq.wd.ref("small", False)[0], "sr_reshade after the plain launch")


def test_zz_diag_counters_stay_zero(gpu):
    assert gpu.diag_counters() == {"hit_not_opaque": 0, "free_errors": 0}
