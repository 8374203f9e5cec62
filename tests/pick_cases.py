"""Picking scenes whose oracle frames can be read back as object codes (a
helper, not a test module).

sr_pick_map (sr.h "Retained frames") names the first surface on a pixel's ray
that is not a single-sided surface seen from behind. The oracle has no such
call; its frame says the same when the colours are codes:

- every object gets an untextured, ambient-1 material of its own and the
  scene no light, so a hit's colour is the material's, exactly;
- an object's colour is red only, a red value of its own, k / 32: opaque
  (alpha 1) or, marked translucent, alpha 0.25. Whatever lies behind a
  translucent surface adds no red (the scenes with a translucent object give
  the opaque ones a green of their own instead), so the red channel of the
  float frame is the first surface's;
- the hole is (0, 0, 0, 1); the skybox one texel (0, 0, 255), three channels;
  the overlay's rays (0, 0.75, 0.5, 1) and (0, 0.25, 0.75, 1); a pixel the noise
  mask blacked out has alpha 0.

A scene has ten materials. With more than nine objects the scene is rendered
in passes (pass k gives objects 9 k .. 9 k + 8 their own colours and the rest
the colour OTHER, all of them opaque and double-sided: the geometry of every
pass is the same) and a pixel's code is the object of the one pass that shows
one. tests/test_pick_cases.py shows on the oracle alone that every pixel of
every case decodes to exactly one code and that each code a case claims
appears on at least 1 % of its frame.
"""
from __future__ import annotations

import numpy as np

import extreme_cases as X
import shading_cases as S
from test_gpu_launch_matrix import World

SKY, HOLE, TR_FLAT, TR_CURVED, NONE = -1, -2, -3, -4, -5  # sr.h SR_PICK_*
UNKNOWN, OTHER_CODE = -100, -101
MIN_SHARE = 0.01
PER_PASS = 9

SKY_RGB = (0.0, 0.0, 1.0)
CURVED_RGBA = (0.0, 0.75, 0.5, 1.0)
FLAT_RGBA = (0.0, 0.25, 0.75, 1.0)
OTHER_RGB = (0.0, 0.125, 0.125)
TRANSLUCENT_ALPHA = 0.25


def red_of(i):
    return (i % PER_PASS + 1) / 32.0


def green_of(i):
    return (i % PER_PASS + 1) / 32.0 + 0.5  # apart from OTHER's, the overlay's and the sky's greens


def sky_texel():
    return np.array([[[0, 0, 255]]], dtype=np.uint8)


def _material(m, rgba, double_sided=1, flip=0):
    X.plain_material(m, rgba)
    m.ambient, m.diffuse, m.specular, m.shininess = 1.0, 0.0, 0.0, 1.0
    m.double_sided_normals, m.flip_normals = double_sided, flip


def recoloured(pkg, scene, flags=None):
    """The passes of a scene: [scene_0, scene_1, ...] with code colours.
    flags: {object index: {"translucent": bool, "double_sided": 0 / 1, "flip":
    0 / 1}} (at most nine objects then: every object keeps a material of its own)."""
    sc, abi = pkg.scenes, pkg.abi
    n = int(scene.num_objects)
    flags = flags or {}
    assert not flags or n <= PER_PASS
    any_translucent = any(f.get("translucent") for f in flags.values())
    passes = []
    for k in range((n + PER_PASS - 1) // PER_PASS or 1):
        s = sc.struct_from_bytes(abi.Scene, sc.struct_bytes(scene))
        s.num_lights = 0
        _material(s.materials[0], (*OTHER_RGB, 1.0))
        for i in range(n):
            if i // PER_PASS != k:
                s.objects[i].material_index = 0
                continue
            f = flags.get(i, {})
            if f.get("translucent"):
                rgba = (red_of(i), 0.0, 0.0, TRANSLUCENT_ALPHA)
            elif any_translucent:
                rgba = (0.0, green_of(i), 0.0, 1.0)
            else:
                rgba = (red_of(i), 0.0, 0.0, 1.0)
            s.objects[i].material_index = 1 + i % PER_PASS
            _material(s.materials[1 + i % PER_PASS], rgba, f.get("double_sided", 1), f.get("flip", 0))
        passes.append(s)
    return passes


def decode_pass(f32, n_objects, k, any_translucent):
    """One pass's float frame -> int32 codes (UNKNOWN where no rule matches,
    OTHER_CODE on an object of another pass)."""
    r, g, b, a = (f32[..., c] for c in range(4))
    out = np.full(f32.shape[:-1], UNKNOWN, dtype=np.int32)
    hits = np.zeros(f32.shape[:-1], dtype=np.int32)

    def put(mask, code):
        out[mask] = code
        hits[mask] += 1

    nored = r == 0.0
    put(nored & (g == 0.0) & (b == 0.0) & (a == 0.0), NONE)
    put(nored & (g == 0.0) & (b == 0.0) & (a == 1.0), HOLE)
    put(nored & (g == SKY_RGB[1]) & (b == SKY_RGB[2]) & (a == 1.0), SKY)
    put(nored & (g == np.float32(CURVED_RGBA[1])) & (b == np.float32(CURVED_RGBA[2])) & (a == 1.0), TR_CURVED)
    put(nored & (g == np.float32(FLAT_RGBA[1])) & (b == np.float32(FLAT_RGBA[2])) & (a == 1.0), TR_FLAT)
    put(nored & (g == np.float32(OTHER_RGB[1])) & (b == np.float32(OTHER_RGB[2])) & (a == 1.0), OTHER_CODE)
    for i in range(k * PER_PASS, min(n_objects, (k + 1) * PER_PASS)):
        # red is the first surface's alone: a translucent one (alpha 0.25 + what follows) or an opaque one
        put(r == np.float32(red_of(i)), i)
        if any_translucent:
            put(nored & (g == np.float32(green_of(i))) & (b == 0.0) & (a == 1.0), i)
    out[hits != 1] = UNKNOWN
    return out


def decode(frames, n_objects, any_translucent=False):
    """The passes' float frames -> (codes, every pixel decoded exactly once)."""
    per = [decode_pass(f, n_objects, k, any_translucent) for k, f in enumerate(frames)]
    codes = per[0].copy()
    ok = np.ones(codes.shape, dtype=bool)
    obj = np.stack([p >= 0 for p in per])
    ok &= ~np.stack([p == UNKNOWN for p in per]).any(0)
    ok &= obj.sum(0) <= 1
    for p in per:
        codes[p >= 0] = p[p >= 0]
    # a pixel without an object shows the same non-object code in every pass
    none = ~obj.any(0)
    for p in per[1:]:
        ok &= ~none | (p == per[0])
    ok &= codes != OTHER_CODE
    return codes, ok


# ---- the cases ---------------------------------------------------------------------
FRONT = {**S.RECT, "pos": (-2.0, 1.0, 6.0), "width": 4.0, "height": 2.0}  # a smaller RECT in front of BACK
FRONT_AWAY = {**S.RECT_AWAY, "pos": (-2.0, -1.0, 6.0), "width": 4.0, "height": 2.0}


def _two_rects(pkg, front):
    s = X.empty_scene(pkg)
    X.append_primitive(s, front, 0)
    X.append_primitive(s, S.BACK, 1)
    return s


def _case(name, scene, w=34, h=22, steps=300, cams=("view",), overlay=False, flags=None, covers=(), **prm):
    return {"id": name, "scene": scene, "w": w, "h": h, "steps": steps, "cams": cams, "overlay": overlay,
            "flags": flags or {}, "covers": covers, "prm": prm}


def cases(pkg):
    sc = pkg.scenes
    default, stress = sc.scene_default(True), sc.scene_stress()
    return [
        # (two of the stress scene's planes fill most of any view: three cameras for nine of its codes)
        _case("stress", stress, 68, 44, 400, cams=("view", "rnd2", "top"), covers=(SKY, HOLE, 2, 4, 5, 13, 14, 15, 20)),
        _case("default", default, 68, 44, 400, cams=("view", "top"), covers=(SKY, HOLE, 1, 2, 3, 4)),
        _case("flat", default, cams=("near",), covers=(SKY, HOLE, 2), raytrace_type=1),
        _case("half-width", default, cams=("near",), covers=(SKY, HOLE, 2), raytrace_type=2, curved_percentage=0.5),
        _case("overlay", default, cams=("rnd3",), overlay=True, covers=(TR_FLAT, TR_CURVED, SKY, HOLE)),
        _case("noise", default, covers=(NONE, SKY), percent_black=0.4),
        _case("translucent-front", _two_rects(pkg, FRONT), cams=("rect",), flags={0: {"translucent": True}},
              covers=(0, 1, SKY)),
        _case("single-sided-behind", _two_rects(pkg, FRONT_AWAY), cams=("rect",), flags={0: {"double_sided": 0}},
              covers=(1, SKY)),
        _case("single-sided-behind-flat", _two_rects(pkg, FRONT_AWAY), cams=("rect",),
              flags={0: {"double_sided": 0}}, covers=(1, SKY), raytrace_type=1),
        _case("kinds", default, 17, 11, cams=("view", "fly1", "fly5"), covers=(SKY, HOLE, 2, 4)),
    ]


class Picks:
    """The cases' recoloured scenes and the decoded oracle frames, made once."""

    def __init__(self, pkg, oracle, textures):
        self.pkg, self.oracle = pkg, oracle
        self.wd = World(pkg, oracle, textures)
        self.arr = textures[1]
        self.bg = sky_texel()
        self.tex = oracle.TextureSet(self.bg, self.arr)
        self.cams = dict(self.wd.cams)
        self.cams["rect"] = S.camera_of(pkg, S.BY_NAME["alpha_0p5"])  # shading_cases.CAM
        sc = pkg.scenes
        self.cams["near"] = sc.camera_look((0.0, 1.0, 6.0), (0.0, -1.0, -6.0), fov=90.0)
        self.cams["top"] = sc.camera_look((2.0, 14.0, 6.0), (-2.0, -14.0, -6.0), fov=100.0)
        self.cams["rnd2"], self.cams["rnd3"] = sc.random_camera(2), sc.random_camera(3)
        tr = pkg.scenes.struct_from_bytes(pkg.abi.TestRay, pkg.scenes.struct_bytes(self.wd.test_rays[True]))
        tr.radius = 0.3  # thick enough for the small frames
        for k in range(4):
            tr.curved_color[k], tr.flat_color[k] = CURVED_RGBA[k], FLAT_RGBA[k]
        self.test_rays = {False: self.wd.test_rays[False], True: tr}
        self.cases = {c["id"]: c for c in cases(pkg)}
        self._passes, self._codes = {}, {}

    def passes(self, case):
        if case["id"] not in self._passes:
            self._passes[case["id"]] = recoloured(self.pkg, case["scene"], case["flags"])
        return self._passes[case["id"]]

    def params(self, case):
        p = self.wd.params(case["steps"])
        for k, v in case["prm"].items():
            setattr(p, k, v)
        return p

    def codes(self, case, cam):
        """(codes [h, w] int32, decoded-once mask) from the oracle, read-only."""
        k = (case["id"], cam)
        if k not in self._codes:
            frames = [self.oracle.render(s, self.cams[cam], self.params(case), case["w"], case["h"], self.tex,
                                         self.test_rays[case["overlay"]])[1] for s in self.passes(case)]
            out = decode(frames, int(case["scene"].num_objects),
                         any(f.get("translucent") for f in case["flags"].values()))
            for a in out:
                a.setflags(write=False)
            self._codes[k] = out
        return self._codes[k]
