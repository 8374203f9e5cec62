"""The (A, B) pairs of the retained-frame tests (a helper, not a test module).

A pair is a launch of scene A with background A, then sr_set_scene(B) and
sr_set_background(SKY_B), then a reshade: B = relit(A) differs from A in
shading-only fields alone (sr.h "Retained frames") and in every one of them.
tests/test_reshade_cases.py shows on the oracle alone that every pair's two
frames differ on more than MIN_CHANGED of the pixels, so that a reshade that
did nothing cannot pass tests/test_gpu_reshade.py.

    PAIRS          key, overlay: a scene and test ray of test_gpu_launch_matrix.World
                   cams: the World's cameras the GPU test launches
                   w, h, steps, prm: the frame and overrides of World.params
                   ss: the sample grids whose frames the GPU test needs
                   (1: the plain frame; 2, 3: the (ss w) x (ss h) sample frame)
    SHADING_PAIRS  (A, B) names of tests/shading_cases.py cases whose scenes
                   differ in shading-only fields: rendered in a chain
"""
from __future__ import annotations

import numpy as np

import shading_cases as S
from test_gpu_launch_matrix import World
from test_gpu_supersample import CELL_IDS, CELLS, box_reference

MIN_CHANGED = 0.10
W, H, STEPS = 17, 11, 300
SKY_B = (5, 7, 3)  # (w, h, channels) of background B, after the World's 2:1 skybox
BATCH = ("view", "fly1", "fly5")


def _pair(name, key="small", overlay=False, cams=("view",), w=W, h=H, steps=STEPS, ss=(1,), **prm):
    return {"id": name, "key": key, "overlay": overlay, "cams": cams, "w": w, "h": h, "steps": steps, "ss": ss,
            "prm": prm}


CELL_PAIRS = [_pair("cell-" + i, k, ov) for (k, ov), i in zip(CELLS, CELL_IDS)] + [
    _pair("cell-small-68x44", w=68, h=44, steps=400)]
MODE_PAIRS = [
    _pair("flat", raytrace_type=1),
    _pair("half-width", raytrace_type=2, curved_percentage=0.5),
    _pair("half-height", raytrace_type=3, curved_percentage=0.5),
    _pair("noise", percent_black=0.4),
    _pair("crosshair", w=68, h=44, crosshair=1),
]
KIND_PAIR = _pair("kinds", cams=BATCH, ss=(1, 2, 3))
PAIRS = CELL_PAIRS + MODE_PAIRS + [KIND_PAIR]
BY_ID = {p["id"]: p for p in PAIRS}

_CHAIN = ("spec_shin_1p0", "spec_shin_0", "spec_shin_inf", "spec_shin_m2", "spec_shin_nan", "spec_ambient_nan",
          "spec_specular_minf", "light_none", "light_four", "light_att_000", "light_intensity_nan",
          "light_color_nan", "light_pos_nan", "light_at_hit", "spec_shin_10000p0")
SHADING_PAIRS = [(S.BY_NAME[a].name, S.BY_NAME[b].name) for a, b in zip(_CHAIN, _CHAIN[1:])]


def relit(pkg, scene):
    """B of a pair: the scene with every light moved and recoloured, a light
    removed (added when there was one at most), every shading-only material
    term changed and every normal_map_index toggled. Nothing else differs."""
    sc, abi = pkg.scenes, pkg.abi
    b = sc.struct_from_bytes(abi.Scene, sc.struct_bytes(scene))
    n = int(scene.num_lights)
    b.num_lights = n - 1 if n >= 2 else n + 1
    for i in range(abi.MAX_LIGHTS):
        L = b.lights[i]
        for k, v in enumerate((7.0 - 5.0 * i, 3.0 + 2.0 * i, 13.0 - i)):
            L.transform.pos[k] = v
        for k, v in enumerate((0.35 + 0.2 * i, 1.0 - 0.15 * i, 0.6)):
            L.color[k] = v
        for k in range(9):
            L.transform.axes[k] = float(k % 4 == 0)
        L.intensity = 9.0 - i
        L.attenuation_constant, L.attenuation_linear, L.attenuation_quadratic = 0.8, 0.05, 0.02
    for i in range(abi.MAX_MATERIALS):
        m = b.materials[i]
        c = [float(m.color[k]) for k in range(3)]
        m.color[0], m.color[1], m.color[2] = 1.0 - 0.5 * c[1], 0.25 + 0.5 * c[2], 0.9 - 0.6 * c[0]
        m.ambient = float(m.ambient) + 0.25
        m.diffuse = 0.5 * float(m.diffuse) + 0.1
        m.specular = float(m.specular) + 0.5
        m.shininess = 2.0 * float(m.shininess) + 3.0
        m.normal_map_index = 1 if m.normal_map_index < 0 else -1
    return b


class Pairs:
    """The World of test_gpu_launch_matrix plus the B side: relit scenes, the
    second background and the oracle's frames of both, rendered once."""

    def __init__(self, pkg, oracle, textures):
        self.pkg, self.oracle = pkg, oracle
        self.wd = World(pkg, oracle, textures)
        self.bg_a, self.arr = textures
        self.bg_b = S.skybox(*SKY_B)
        self.bg_b.setflags(write=False)
        self.tex = {"A": self.wd.tex, "B": oracle.TextureSet(self.bg_b, self.arr)}
        self._b, self._frames = {}, {}

    def scene(self, which, key):
        if which == "A":
            return self.wd.scene(key)
        if key not in self._b:
            self._b[key] = relit(self.pkg, self.wd.scene(key))
        return self._b[key]

    def params(self, pair):
        p = self.wd.params(pair["steps"])
        for k, v in pair["prm"].items():
            setattr(p, k, v)
        return p

    def frame(self, which, pair, cam="view", ss=1):
        """The oracle's read-only (rgba8, float rgba, steps) of side `which`
        of a pair: the (ss w) x (ss h) frame."""
        k = (which, pair["id"], cam, ss)
        if k not in self._frames:
            out = self.oracle.render(self.scene(which, pair["key"]), self.wd.cams[cam], self.params(pair),
                                     ss * pair["w"], ss * pair["h"], self.tex[which],
                                     self.wd.test_rays[pair["overlay"]])
            for a in out:
                a.setflags(write=False)
            self._frames[k] = out
        return self._frames[k]

    def resolved(self, which, pair, cam, ss):
        """RGBA8 of the output frame: the sample frame's box resolve for ss > 1."""
        s = self.frame(which, pair, cam, ss)[0]
        return s if ss == 1 else box_reference(s, ss)

    # ---- the chain of shading cases (65x41, 100 steps, the "std" textures, then SKY_B)
    def shading_tex(self, which):
        bg, arr, _ = S.textures_of(self.pkg, "std")
        return (bg if which == "A" else self.bg_b), arr

    def shading_frame(self, which, name):
        k = ("shading", which, name)
        if k not in self._frames:
            case = S.BY_NAME[name]
            bg, arr = self.shading_tex(which)
            out = self.oracle.render(S.build(self.pkg, case), S.camera_of(self.pkg, case), S.params_of(self.pkg, case),
                                     S.W, S.H, self.oracle.TextureSet(bg, arr))
            for a in out:
                a.setflags(write=False)
            self._frames[k] = out
        return self._frames[k]


def changed_share(a, b) -> float:
    """The share of pixels in which two RGBA8 frames differ."""
    return float((np.asarray(a) != np.asarray(b)).any(-1).mean())
