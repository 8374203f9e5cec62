"""The shading half of geodesic.hip at the edges of its inputs
(tests/shading_cases.py).

The other extreme tables keep plain_material and one_light; the generators
of scenes.py draw shininess from {4, 8, 32, 100}, positive attenuations,
intensities of 2 to 10 and colours in [0, 1]. Here shade_hit,
surface_of_t<false>, surface_frame, bilinear, tex_array, get_bg, the material
branch of hit_opacity_uniform, the shade kernel's hit log and write_pixel's
unorm8 see what no other module gives them: shininess 0, negative, infinite
and NaN; negative, infinite and NaN material and light terms; no light and
four; attenuations of zero and of either sign; a light on the surface, behind
it, at the origin, at 1e30 and at NaN; alphas around 1, negative, infinite
and NaN, alone and in front of an opaque rectangle; single-sided surfaces
from behind under the crosshair; a hit log filled with "maybe translucent"
hits of which one is exactly opaque; texture sizes and plane mappings of 0,
negative, NaN, infinite and 1e30; normal maps on every primitive type, on the
box's six faces, on tilted and sheared frames, with zero texels; uv seams on
the centre ray; skyboxes of 1x1 to 5x7 texels with 3 and 4 channels, looking
up, down and along the u wrap; contexts without a texture array and without a
background. This is also where host and device arithmetic differ most: a
binary64 pow / asin / atan2 rounded to binary32, 1 / sqrt(0), 0 * inf, a
waterfall over (object, face) keys.

Each cell (case, host, mode) renders a 65x41 frame (5 x 3 tiles, partial
waves on two edges, the centre pixel at uv = (0, 0)) at 100 steps and
asserts, in this order:

- sr_set_scene accepts the scene;
- the frame with culling off equals the oracle's (the base arithmetic);
- the frame with culling on equals the frame with culling off (the margins);
- the frame with culling on equals the oracle's.

"Equals" is compare_strict: RGBA8 bytes, step counts, and float bits per
channel, where NaN matches NaN and everything else matches bit for bit -
the finite channels of a pixel that also has a NaN channel included
(test_gpu_parity.compare excuses the whole pixel).

Every nonfinite case is also rendered through sr_render (== the debug
path's bytes) and sr_render_ss with ss = 2 (== numpy's box average of the
oracle's 130x82 frame), and every kernel frame stores NaN as 0, +inf as 255
and -inf as 0.

Measured with this table on the library of this module's parent commit
(pixels of 2665 that differ): every one of the 286 cells 0 with culling on
against culling off, 0 with culling on against the oracle and 0 with culling
off against the oracle, shininess 1/2, 1, 2 and 3 included (where a binary64
pow off by its last bit on one side could have flipped a binary32 rounding);
sr_render and sr_render_ss of the non-finite cases 0; diagnostic counters 0
on all three contexts. Nothing in the library changed.

tests/test_shading_cases.py shows on the oracle alone that each case is what
it says; tests/test_oracle_golden_shading.py pins the oracle to the reference
shader on the cases the shader's capacities hold.
"""
import ctypes as C

import numpy as np
import pytest

import shading_cases as S
from test_gpu_launch_matrix import host, same
from test_gpu_supersample import box_reference

pytestmark = pytest.mark.gpu

DIAG_ZERO = {"hit_not_opaque": 0, "free_errors": 0}


class Contexts:
    """The shared context (its uploads follow the cell's texture set) and one
    fresh context per texture set that lacks an upload."""

    def __init__(self, pkg):
        self.pkg = pkg
        self.ctx = {}
        self.bound = {}

    def get(self, key):
        bg, arr, _ = S.textures_of(self.pkg, key)
        name = "shared" if bg is not None and arr is not None else key
        if name not in self.ctx:
            self.ctx[name] = self.pkg.Renderer(0)
            self.ctx[name].set_test_ray(self.pkg.abi.default_test_ray())
        r = self.ctx[name]
        if self.bound.get(name) != key:
            if bg is not None:
                r.set_background(bg)
            if arr is not None:
                r.set_texture_array(arr)
            self.bound[name] = key
        return r

    def close(self):
        for r in self.ctx.values():
            r.close()


@pytest.fixture(scope="module")
def contexts(pkg):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    c = Contexts(pkg)
    yield c
    c.close()


@pytest.fixture(scope="module")
def refs(pkg, oracle):
    """(case, host, mode, ss=1) -> the oracle's read-only frame, rendered once."""
    texsets, frames = {}, {}

    def get(case, host_key, mode, ss=1):
        k = (case.name, host_key, mode, ss)
        if k not in frames:
            if case.textures not in texsets:
                bg, arr, _ = S.textures_of(pkg, case.textures)
                texsets[case.textures] = oracle.TextureSet(bg, arr)
            frames[k] = oracle.render(S.build(pkg, case, host_key), S.camera_of(pkg, case), S.params_of(pkg, case, mode),
                                      ss * S.W, ss * S.H, texsets[case.textures])
            for a in frames[k]:
                a.setflags(write=False)
        return frames[k]

    return get


def compare_strict(got, want, label):
    """(rgba8, float, steps) frames: bytes and step counts equal, floats
    equal bit for bit per channel with NaN = NaN."""
    b, f, s = got
    rb, rf, rs = want
    px = (b != rb).any(-1)
    chan = (f.view(np.uint32) != rf.view(np.uint32)) & ~(np.isnan(f) & np.isnan(rf))
    msg = (f"{label}: rgba8 differ {int(px.sum())}/{px.size}, float channels differ {int(chan.sum())} in "
           f"{int(chan.any(-1).sum())} pixels, steps differ {int((s != rs).sum())}, "
           f"max byte diff {int(np.abs(b.astype(int) - rb.astype(int)).max())}")
    assert not px.any(), msg
    assert not (s != rs).any(), msg
    assert not chan.any(), msg


def differing(a, b):
    chan = (a[1].view(np.uint32) != b[1].view(np.uint32)) & ~(np.isnan(a[1]) & np.isnan(b[1]))
    return int(((a[0] != b[0]).any(-1) | chan.any(-1) | (a[2] != b[2])).sum())


def check_stores(frame, label):
    """write_pixel's unorm8: NaN -> 0, +inf -> 255, -inf -> 0."""
    b, f, _ = frame
    assert (b[np.isnan(f)] == 0).all() and (b[f == np.inf] == 255).all() and (b[f == -np.inf] == 0).all(), label


def debug_frames(gpu, cam, params):
    """(rgba8, float, steps) with culling on and off."""
    outs = []
    for cull in (True, False):
        gpu.set_culling(cull)
        f, b, s = host(*gpu.render_debug(cam, params, S.W, S.H))
        outs.append((b, f, s))
    gpu.set_culling(True)
    return outs


@pytest.mark.parametrize("cell", S.cells(), ids=S.cell_id)
def test_shading_extreme(pkg, contexts, refs, cell):
    case, host_key, mode = cell
    label = S.cell_id(cell)
    scene, cam, params = S.build(pkg, case, host_key), S.camera_of(pkg, case), S.params_of(pkg, case, mode)
    o = refs(case, host_key, mode)
    try:
        gpu = contexts.get(case.textures)
        assert gpu.lib.sr_set_scene(gpu.ctx, C.byref(scene)) == pkg.abi.SR_OK
        culled, unculled = debug_frames(gpu, cam, params)
        plain = ss = None
        if case.nonfinite:
            plain, ss = host(gpu.render(cam, params, S.W, S.H), gpu.render_ss(cam, params, S.W, S.H, 2))
    except AssertionError:
        raise
    except Exception as e:  # noqa: BLE001 - a runtime error, not a failed comparison: nothing more is launched
        pytest.exit(f"device error in {label}, nothing more is launched: {e!r}", returncode=3)
    print(f"MEASURED {label}: culled vs unculled {differing(culled, unculled)} pixels, culled vs oracle "
          f"{differing(culled, o)}, unculled vs oracle {differing(unculled, o)}")
    compare_strict(unculled, o, label + " (culling off: the base arithmetic)")
    compare_strict(culled, unculled, label + " (culling on against off)")
    compare_strict(culled, o, label + " (culling on)")
    for frame in (culled, unculled):
        check_stores(frame, label)
    if case.nonfinite:
        same(plain, culled[0], label + ", sr_render against the debug path")
        same(ss, box_reference(refs(case, host_key, mode, ss=2)[0], 2), label + ", sr_render_ss against the oracle's box")


def test_zz_diag_counters_zero(contexts):
    """After every frame of this module, on every context: no pixel stopped
    at an opaque-classified hit whose shaded alpha was not 1, and no
    stream-ordered free failed."""
    assert contexts.ctx
    for name, gpu in contexts.ctx.items():
        assert gpu.diag_counters() == DIAG_ZERO, name
