"""The oracle's own arithmetic restated on top of the ray maps (a helper, not
a test module).

sr_ray_maps (sr.h "Ray maps") has no counterpart in the oracle, whose only
output is FragColor. Two numpy statements tie the maps to it bit for bit:

- sky_uv_np(dir): get_bg's (u, v) (frag:830-834). The oracle's float
  FragColor of a pure-sky pixel is oracle.sample_texture(sky, u, v, mode).
- deferred_np(scene, object, point, normal, view, base): calculate_lighting's
  light loop (frag:406-437, sr_oracle.c:393-425) in float32, in the oracle's
  operation order, pow / atan2 / asin as the binary64 function rounded to
  float32. The oracle's FragColor rgb of a pixel whose first surface is opaque.

tests/test_ray_map_cases.py shows on the oracle alone that both reproduce its
frames and that the frames are sensitive to one ulp of every input: under the
light rig below. A rig of distant lights and a high shininess is not (a light
12 away with shininess 20 hides an ulp of the point or of the view direction
on every pixel).
"""
from __future__ import annotations

import math

import numpy as np

import extreme_cases as X
import shading_cases as S

F = np.float32
PI = F(3.1415926535)  # frag:10
QNAN_BITS = 0x7FC00000
END_NONE, END_SKY, END_OPAQUE = 0, 1, 2  # sr.h SR_RAY_END_*
W, H = 68, 44
SKY_W, SKY_H = 2048, 1024
MIN_SKY_SHARE = MIN_HIT_SHARE = 0.05
MIN_UV_SENSITIVE = 0.90   # of the sky pixels, per ulp of u and of v
MIN_LIT_SENSITIVE = 0.03  # of a scene's opaque-hit pixels, per ulp of a component of point, normal, view
MIN_LIT_PIXELS = 5


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def same_bits(a, b):
    """Elementwise: equal as bits, a NaN matching a NaN."""
    a, b = np.asarray(a, dtype=F), np.asarray(b, dtype=F)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def ulp_up(a):
    """The next float32 above (finite, non-zero inputs: one ulp away from zero for negatives is down)."""
    return np.nextafter(np.asarray(a, dtype=F), F(np.inf))


def random_sky(seed=11):
    """The 2048 x 1024 random RGB skybox (generated, not committed)."""
    sky = np.random.default_rng(seed).integers(0, 256, size=(SKY_H, SKY_W, 3), dtype=np.uint8)
    sky.setflags(write=False)
    return sky


# ---- the numpy statements ------------------------------------------------------
def _f(fn, *cols):
    """A binary64 libm function of float32 columns, rounded once to float32 (a domain error is a NaN)."""
    out = np.empty(len(cols[0]), dtype=F)
    for i, xs in enumerate(zip(*cols)):
        try:
            out[i] = F(fn(*(float(x) for x in xs)))
        except ValueError:
            out[i] = F(np.nan)
    return out


def sky_uv_np(direction):
    """get_bg's (u, v) of directions [..., 3] (taken as they are) -> [..., 2] float32."""
    d = np.asarray(direction, dtype=F)
    flat = d.reshape(-1, 3)
    with np.errstate(all="ignore"):
        u = _f(math.atan2, flat[:, 2], flat[:, 0]) / PI
        u = np.where(u < F(0.0), u + F(2.0), u)
        u = u * F(0.5)
        v = _f(math.asin, flat[:, 1]) / PI + F(0.5)
    return np.stack([u, v], axis=-1).astype(F).reshape(d.shape[:-1] + (2,))


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def norm3(a):
    k = F(1.0) / np.sqrt(dot3(a, a))
    return a * k[..., None]


def _fmax0(x):
    return np.where(x < F(0.0), F(0.0), x)  # f_max(x, 0) = x < 0 ? 0 : x


def deferred_np(scene, obj, point, normal, view, base):
    """calculate_lighting's rgb of n pixels of object `obj` (an index into
    scene.objects[]): point, normal, view [n, 3] and base [n, 4] float32."""
    p, n, v, base = (np.asarray(a, dtype=F) for a in (point, normal, view, base))
    mi = int(scene.objects[obj].material_index)
    if mi < 0 or mi >= len(scene.materials):
        mi = 0
    m = scene.materials[mi]
    brgb = base[:, :3]
    with np.errstate(all="ignore"):
        col = brgb * F(m.ambient)
        for i in range(min(int(scene.num_lights), len(scene.lights))):
            L = scene.lights[i]
            lpos = np.array(list(L.transform.pos), dtype=F)
            lcol = np.array(list(L.color), dtype=F)
            d = lpos[None, :] - p
            ldir = norm3(d)
            dist = np.sqrt(dot3(d, d))
            att = F(1.0) / ((F(L.attenuation_constant) + F(L.attenuation_linear) * dist) +
                            (F(L.attenuation_quadratic) * dist) * dist)
            diff = _fmax0(dot3(n, ldir))
            diffuse = (lcol[None, :] * (F(m.diffuse) * diff)[:, None]) * brgb
            inc = -ldir
            refl = inc - n * (F(2.0) * dot3(n, inc))[:, None]
            s = _fmax0(dot3(v, refl))
            spec = _f(math.pow, s, np.full(len(s), F(m.shininess), dtype=F))
            specular = lcol[None, :] * (F(m.specular) * spec)[:, None]
            col = col + ((diffuse + specular) * att[:, None]) * F(L.intensity)
    return col.astype(F)


def deferred_frame(scene, ids, point, normal, view, base):
    """deferred_np over a frame: rgb [..., 3] where ids >= 0 (NaN elsewhere)."""
    out = np.full(ids.shape + (3,), np.nan, dtype=F)
    for obj in np.unique(ids[ids >= 0]):
        k = ids == obj
        out[k] = deferred_np(scene, int(obj), point[k], normal[k], view[k], base[k])
    return out


# ---- the light rig ---------------------------------------------------------------
# Four lights 1.5 to 5 from the lit surfaces, on different sides of them, of
# distinct colours, all three attenuation terms non-zero; every material
# shininess 1 or 2 and specular >= 0.5. Positions are relative to an anchor
# (a point on or near the lit surfaces).
RIG_OFFSETS = ((2.5, 1.0, 2.5), (-2.5, 1.5, 2.0), (0.5, -2.5, 2.5), (-0.5, 0.5, 3.5))
RIG_COLORS = ((1.0, 0.9, 0.8), (0.4, 0.7, 1.0), (0.9, 0.3, 0.5), (0.5, 1.0, 0.4))
RIG_ATT = ((0.25, 0.3, 0.5), (0.25, 0.6, 1.0), (0.25, 0.45, 0.75), (0.25, 0.9, 1.5))


def rig(pkg, scene, anchor):
    """A copy of the scene under the rig around `anchor`."""
    s = pkg.scenes.struct_from_bytes(pkg.abi.Scene, pkg.scenes.struct_bytes(scene))
    s.num_lights = 4
    for i in range(4):
        S._set_light(s.lights[i], {"pos": tuple(a + o for a, o in zip(anchor, RIG_OFFSETS[i])), "color": RIG_COLORS[i],
                                   "intensity": 1.5 + 0.5 * i, "att": RIG_ATT[i]})
    for k, m in enumerate(s.materials):
        m.shininess = 1.0 if k % 2 == 0 else 2.0
        m.specular = 0.9 if k % 2 == 0 else 0.6
        m.diffuse, m.ambient = 0.7, 0.2
    return s


# ---- the CPU cases: flat-mode frames of spheres and rectangles ------------------
CAM = S.CAM  # (0, 0, 12) looking at the origin, fov 60
SPHERE = {"type": "sphere", "pos": (0.0, 0.0, 6.0), "axes": S.FACING, "radius": 2.0}
SMALL_SPHERE = {"type": "sphere", "pos": (2.6, -0.8, 7.0), "axes": X.IDENT, "radius": 1.1}
RECT = {"type": "rectangle", "pos": (-3.2, 1.4, 6.0), "axes": S.FACING, "width": 3.6, "height": 2.8}


def _scene(pkg, specs, colors):
    s = X.empty_scene(pkg)
    for k, (spec, rgba) in enumerate(zip(specs, colors)):
        X.plain_material(s.materials[k], rgba)
        X.append_primitive(s, spec, k)
    return rig(pkg, s, (0.0, 0.0, 7.0))


def cpu_cases(pkg):
    """{name: rigged scene}: one sphere; a rectangle and a sphere."""
    return {
        "sphere": _scene(pkg, (SPHERE,), ((0.9, 0.5, 0.2, 1.0),)),
        "rect+sphere": _scene(pkg, (RECT, SMALL_SPHERE), ((0.3, 0.8, 0.6, 1.0), (0.8, 0.4, 0.9, 1.0))),
    }


def camera(pkg):
    pos, target, fov = CAM
    return pkg.scenes.camera_look(pos, tuple(float(t) - float(p) for p, t in zip(pos, target)), fov=fov)


def geometric_normal(scene, obj, point):
    """tangent_space[2] of a sphere (frag:209-232) or a rectangle (frag:320-333) hit, in numpy."""
    o = scene.objects[obj]
    if o.type == X.TYPE_OF["sphere"]:
        pos = np.array(list(scene.spheres[o.index].transform.pos), dtype=F)
        return norm3(np.asarray(point, dtype=F) - pos[None, :])
    assert o.type == X.TYPE_OF["rectangle"], o.type
    up = np.array(list(scene.rectangles[o.index].plane.transform.axes[3:6]), dtype=F)
    return np.broadcast_to(up, np.asarray(point).shape).astype(F)


# ---- the GPU scenes under the rig ------------------------------------------------
def rigged(pkg, scene):
    """A GPU test scene under the rig, anchored above the hole among its objects."""
    return rig(pkg, scene, (0.0, 1.0, 1.0))
