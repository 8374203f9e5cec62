"""A rejected block-list call touches no cache of the context.

tests/test_gpu_rejections.py promises that "a rejected call launches nothing
and drops nothing", but never fills a cache. Here the retained frame is a
block-list launch, and each block-list entry point is then rejected nine
times (more than the block-list cache's 8 entries hold), every time with a
valid list the context has never seen and for a reason found late (the
params, or the frame stride of a batch). An entry point that uploaded its
list before it had finished rejecting would evict the retained frame's list
on the way, and with it the retained frame.

68x44 frame, the small scene: one frame and two reshades are launched.
"""
import ctypes as C
import itertools

import pytest

pytestmark = pytest.mark.gpu

W, H = 68, 44
BR, NBK = 8, 3
ROWS = NBK * BR
FILL = 77
REJECTED = 9  # more than a cache holds


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


def test_rejected_block_list_calls_keep_the_retained_frame(pkg, gpu):
    import numpy as np
    import torch

    r = gpu
    abi, sc, lib = pkg.abi, pkg.scenes, r.lib
    INV = abi.SR_E_INVALID
    cam = sc.camera_look((0.0, 2.0, 15.0), (0.0, -2.0, -15.0))
    cams = (abi.Camera * 4)(cam, cam, cam, cam)
    prm = abi.default_params(max_steps=400, percent_black=-1.0, crosshair=0)
    st = r._stream(None)
    r.set_scene(sc.scene_default(True))
    r.set_test_ray(abi.default_test_ray())
    r.set_scene_sequence([sc.scene_default(True), sc.scene_default(False)])
    r.render_block_list([cam], prm, W, H, BR, [0, 2, 4])
    assert r.can_reshade()
    r0 = r.reshade().cpu().numpy()

    fresh = (l for l in itertools.permutations(range((H + BR - 1) // BR), NBK) if l != (0, 2, 4))
    buf = torch.full((2, ROWS, W, 4), FILL, dtype=torch.uint8, device="cuda")
    out, pitch, short = C.c_void_p(buf.data_ptr()), 4 * W, 4 * W * ROWS - 4
    keep, failures = [], []
    entries = {
        # (params, n_frames, frame_stride) -> the call
        "sr_render_block_list": lambda p, n, fs, lst: lib.sr_render_block_list(
            r.ctx, cams, n, p, W, H, BR, lst, NBK, out, pitch, fs, st),
        "sr_render_block_list_ss": lambda p, n, fs, lst: lib.sr_render_block_list_ss(
            r.ctx, cams, n, p, W, H, BR, lst, NBK, 2, out, pitch, fs, st),
        "sr_render_sequence_block_list": lambda p, n, fs, lst: lib.sr_render_sequence_block_list(
            r.ctx, 0, cams, n, p, W, H, BR, lst, NBK, 1, out, pitch, fs, st),
        "sr_render_shutter_block_list": lambda p, n, fs, lst: lib.sr_render_shutter_block_list(
            r.ctx, 0, cams, None, 2, n, p, W, H, BR, lst, NBK, 2, out, pitch, fs, st),
    }
    for entry, fn in entries.items():
        for k in range(REJECTED):
            blocks = next(fresh)
            lst = (C.c_int * NBK)(*blocks)
            keep.append(lst)
            if k % 2 == 0:
                got, why = fn(None, 1, 4 * W * ROWS, lst), "params = NULL"
            else:
                got, why = fn(C.byref(prm), 2, short, lst), "n_frames = 2, frame_stride 4 bytes short"
            torch.cuda.synchronize()
            what = f"{entry} {list(blocks)} ({why})"
            print(f"{what}: {got}, sr_can_reshade {lib.sr_can_reshade(r.ctx)}")
            if got != INV:
                failures.append(f"{what}: status {got}, expected {INV}")
            if not bool((buf == FILL).all()):
                failures.append(f"{what}: the buffer was written")
                buf.fill_(FILL)
            if lib.sr_can_reshade(r.ctx) != 1:
                failures.append(f"{what}: the retained frame is gone")
    assert not failures, "\n".join(failures)
    assert np.array_equal(r.reshade().cpu().numpy(), r0), "the retained frame no longer reshades to the same bytes"
    assert r.diag_counters() == {"hit_not_opaque": 0, "free_errors": 0}
