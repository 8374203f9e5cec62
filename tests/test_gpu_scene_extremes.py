"""The culling shortcuts on scenes no generator draws (tests/extreme_cases.py).

The kernel's budgets, reach tests, exclusions and black-hole windows
 are exact by margin: each rests on premises about the scene
(a radius is a magnitude, a frame is orthonormal, an object lies outside the
hole and inside 1 / u_f, ...). Every case here breaks one premise or sits at
a bound's edge: signed and zero sizes, primitives at and inside the horizon,
around the camera and the hole, thin, beyond r = 1 / u_f, non-unit and
sheared normals, non-finite fields. Each cell (case, host scene, step
schedule) renders a 64x40 frame (4 x 3 tiles, partial waves on two edges) and
asserts:

- sr_set_scene accepts the scene;
- the frame equals the CPU oracle's: RGBA8, float bits (NaN = NaN) and step
  counts, no pixel differing (test_gpu_parity.compare);
- the culled frame equals the frame with culling off on all three arrays.

Which of the two fails names the cause: culled != unculled is a margin bug;
both GPU frames agreeing with each other and not with the oracle is the base
arithmetic. tests/test_scene_extremes_cases.py shows on the oracle alone
that each primitive is on screen.

Found with this table, on the library of this module's parent commit with
culling on (pixels of 2560 that differ from the oracle and from the frame
with culling off, which equalled the oracle everywhere): disk_radius_neg4
607 at 400 steps and 592 at 100, alone and embedded (every pixel that shows
the disk); annulus_neg_neg and annulus_pos_neg 147 alone, 139 and 138
embedded; annulus_neg_pos and every other case 0. The distance-to-primitive
clearance took rho - radius with the signed radius (precompute.cpp pack_slot now
stores magnitudes).
"""
import ctypes as C

import numpy as np
import pytest

import extreme_cases as X
from test_gpu_parity import compare

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(pkg, textures):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    bg, arr = textures
    r = pkg.Renderer(0)
    r.set_background(bg)
    r.set_texture_array(arr)
    r.set_test_ray(pkg.abi.default_test_ray())
    yield r
    r.close()


@pytest.fixture(scope="module")
def oracle_tex(oracle, textures):
    bg, arr = textures
    return oracle.TextureSet(bg, arr)


def frames(gpu, cam, params):
    """(rgba8, float, steps) with culling on and off."""
    import torch

    outs = []
    for cull in (True, False):
        gpu.set_culling(cull)
        f, b, s = gpu.render_debug(cam, params, X.W, X.H)
        torch.cuda.synchronize()
        outs.append((b.cpu().numpy(), f.cpu().numpy(), s.cpu().numpy()))
    gpu.set_culling(True)
    return outs


@pytest.mark.parametrize("cell", X.cells(), ids=X.cell_id)
def test_extreme_scene(pkg, gpu, oracle, oracle_tex, cell):
    case, host, schedule = cell
    scene = X.build(pkg, case, host)
    cam = X.camera_of(pkg, case)
    params = X.params_of(pkg, case, schedule)
    assert gpu.lib.sr_set_scene(gpu.ctx, C.byref(scene)) == pkg.abi.SR_OK
    culled, unculled = frames(gpu, cam, params)
    o = oracle.render(scene, cam, params, X.W, X.H, oracle_tex)
    label = X.cell_id(cell)
    same = [np.array_equal(culled[0], unculled[0]),
            np.array_equal(culled[1].view(np.uint32), unculled[1].view(np.uint32)),
            np.array_equal(culled[2], unculled[2])]
    px = int(((culled[0] != unculled[0]).any(-1) | (culled[2] != unculled[2])).sum())
    vs_oracle = [int(((g[0] != o[0]).any(-1) | (g[2] != o[2])).sum()) for g in (culled, unculled)]
    print(f"MEASURED {label}: culled vs unculled {px} pixels, culled vs oracle {vs_oracle[0]}, "
          f"unculled vs oracle {vs_oracle[1]}")
    compare(unculled, o, label + " (culling off: the base arithmetic)")
    assert all(same), f"{label}: culling changes {px} pixels (rgba8, float bits, steps equal: {same})"
    compare(culled, o, label + " (culling on)")


def test_zz_diag_counters_zero(gpu):
    """After every frame of this module on the shared context: no pixel
    stopped at an opaque-classified hit whose shaded alpha was not 1, and no
    stream-ordered free failed."""
    assert gpu.diag_counters() == {"hit_not_opaque": 0, "free_errors": 0}
