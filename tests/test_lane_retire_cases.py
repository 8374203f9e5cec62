"""The frames of tests/test_gpu_lane_retire.py exercise what it claims.

The coasting loop of sr_integrate_kernel retires, inside the loop, the lanes
whose ray ends when it crosses u_f; a wave whose escaping lanes end at many
different steps runs that handler many times, next to lanes that are still
integrating, fall into the hole or hit an object. This module shows on the
CPU oracle alone that the GPU module's frames (default scene and camera)
hold such waves.

A lane "escapes" when its colour and step count equal those of the frame of
scene_black_hole_only (nothing but the hole and the skybox) and its colour
is not black; it is "captured" when both frames agree and it is black; any
other lane met an object. The counts below are lower bounds of what
oracle.render gave when this module was written.
"""
import numpy as np
import pytest

SIZES = [(68, 44), (16, 16)]
# (width, height) -> max_steps -> the most distinct end steps of one wave's escaping lanes
DISTINCT = {(68, 44): {100: 10, 500: 26, 2000: 49}, (16, 16): {100: 12, 500: 27, 2000: 31}}
# waves that hold escaping, captured and object-hit lanes together, of how many waves
MIXED = {(68, 44): (4, 54), (16, 16): (2, 4)}


def classify(pkg, oracle, textures, w, h, steps):
    """(escaping, captured, object-hit masks, step map) of the default frame."""
    abi, sc = pkg.abi, pkg.scenes
    bg, arr = textures
    tex = oracle.TextureSet(bg, arr)
    cam = abi.default_camera()
    prm = abi.default_params(max_steps=steps, percent_black=-1.0, crosshair=0)
    b, _, s = oracle.render(sc.scene_default(True), cam, prm, w, h, tex)
    b0, _, s0 = oracle.render(sc.scene_black_hole_only(), cam, prm, w, h, tex)
    agree = (b == b0).all(-1) & (s == s0)
    black = (b[..., :3] == 0).all(-1)
    return agree & ~black, agree & black, ~agree, s


def waves(w, h):
    for y in range(0, h, 8):
        for x in range(0, w, 8):
            yield slice(y, min(h, y + 8)), slice(x, min(w, x + 8))


@pytest.fixture(scope="module")
def frames(pkg, oracle, textures):
    return {(w, h, n): classify(pkg, oracle, textures, w, h, n) for w, h in SIZES for n in (100, 500, 2000)}


@pytest.mark.parametrize("steps", [100, 500, 2000])
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_escaping_lanes_end_at_many_steps(frames, w, h, steps):
    esc, _, _, s = frames[(w, h, steps)]
    most = max(len(np.unique(s[ys, xs][esc[ys, xs]])) for ys, xs in waves(w, h))
    print(f"{w}x{h}, {steps} steps: {most} distinct end steps in one wave")
    assert most >= DISTINCT[(w, h)][steps]


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_waves_hold_all_three_kinds(frames, w, h):
    need, total = MIXED[(w, h)]
    assert len(list(waves(w, h))) == total
    for steps in (100, 500, 2000):
        esc, cap, obj, _ = frames[(w, h, steps)]
        n = sum(bool(esc[ys, xs].any() and cap[ys, xs].any() and obj[ys, xs].any()) for ys, xs in waves(w, h))
        print(f"{w}x{h}, {steps} steps: {n} of {total} waves hold all three kinds")
        assert n >= need, (steps, n)
