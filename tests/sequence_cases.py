"""Scene sequences for the sr_render_sequence tests (sr.h "Scene sequences").

A sequence launch renders frame f from scene first_scene + f; every test
compares a frame with the CPU oracle's frame of that one scene. The sequences
are chosen so that a launch which read a neighbouring frame's scene in any one
kernel cannot pass: for the camera "view" any two frames of a sequence differ
on at least 1 % of the pixels at every size the GPU tests use
(tests/test_sequence_cases.py asserts it with the oracle alone).

  MIX      small, large, general, stacked, large_translucent and the black
           hole alone: slot counts (6, 21, 8, ...), cylinder counts and object
           counts change from frame to frame, one frame has every ray resumed
           (stacked), one has no objects
  GEO8     the default scene with spheres[0] at eight positions, heights and
           radii on a circle of 10; nothing else changes
  SHADE8   the default scene with only lights[0] moved and recoloured
  ORBIT40  both kinds of change over 40 positions

Scenes, cameras, test rays, params and textures are World's
(tests/test_gpu_launch_matrix.py).
"""
import math

from test_gpu_launch_matrix import STEPS, H, W, World

MIX = ("small", "large", "general", "stacked", "large_translucent", "bh")
NAMES = ("MIX", "GEO8", "SHADE8", "ORBIT40")
# the sizes the GPU tests render each sequence at (tests/test_gpu_sequence.py)
SIZES = {
    "MIX": ((W, H), (33, 17), (17, 11)),
    "GEO8": ((W, H), (17, 11)),
    "SHADE8": ((W, H), (17, 11)),
    "ORBIT40": ((W, H), (17, 11)),
}

# the frames of every Sequences of the session (World's scenes, cameras and
# textures are the same in each): the CPU and the GPU modules share them
_REF = {}


def _default(sc):
    return sc.scene_default(True)


def _orbit_sphere(s, angle, height, radius):
    sp = s.spheres[0]
    sp.transform.pos[0] = 10.0 * math.cos(angle)
    sp.transform.pos[1] = height
    sp.transform.pos[2] = 10.0 * math.sin(angle)
    sp.radius = radius


def _orbit_light(s, angle, k):
    lt = s.lights[0]
    lt.transform.pos[0] = 14.0 * math.cos(angle)
    lt.transform.pos[1] = 10.0 - 0.4 * (k % 8)
    lt.transform.pos[2] = 14.0 * math.sin(angle)
    lt.color[0] = 0.35 + 0.65 * (0.5 + 0.5 * math.cos(angle))
    lt.color[1] = 0.35 + 0.65 * (0.5 + 0.5 * math.cos(angle + 2.1))
    lt.color[2] = 0.35 + 0.65 * (0.5 + 0.5 * math.cos(angle + 4.2))
    lt.intensity = 6.0 + (k % 5)


def geo8(sc):
    out = []
    for k in range(8):
        s = _default(sc)
        _orbit_sphere(s, 0.3 + 2.0 * math.pi * k / 8.0, -2.5 + 0.8 * k, 1.2 + 0.25 * k)
        out.append(s)
    return out


def shade8(sc):
    out = []
    for k in range(8):
        s = _default(sc)
        _orbit_light(s, 0.5 + 2.0 * math.pi * k / 8.0, k)
        out.append(s)
    return out


def orbit40(sc):
    out = []
    for k in range(40):
        s = _default(sc)
        a = 2.0 * math.pi * k / 40.0
        _orbit_sphere(s, a, 3.0 * math.sin(3.0 * a), 1.5 + 0.5 * math.cos(2.0 * a))
        _orbit_light(s, 0.5 + 2.0 * a, k)
        out.append(s)
    return out


class Sequences:
    """World with the sequences' scenes and their oracle frames, made once."""

    def __init__(self, pkg, oracle, textures):
        self.pkg, self.oracle = pkg, oracle
        self.wd = World(pkg, oracle, textures)
        self._scenes = {}
        self._ref = _REF

    def scenes(self, name):
        if name not in self._scenes:
            sc = self.pkg.scenes
            self._scenes[name] = {
                "MIX": lambda: [sc.scene_black_hole_only() if k == "bh" else self.wd.scene(k) for k in MIX],
                "GEO8": lambda: geo8(sc),
                "SHADE8": lambda: shade8(sc),
                "ORBIT40": lambda: orbit40(sc),
            }[name]()
        return self._scenes[name]

    def params(self, steps=STEPS, **kw):
        return self.wd.params(steps, **kw)

    def ref(self, name, k, overlay=False, cam="view", w=W, h=H, steps=STEPS):
        """The oracle's (rgba8, float rgba, steps) of scene k of a sequence, read-only."""
        key = (name, k, overlay, cam, w, h, steps)
        if key not in self._ref:
            out = self.oracle.render(self.scenes(name)[k], self.wd.cams[cam], self.params(steps), w, h, self.wd.tex,
                                     self.wd.test_rays[overlay])
            for a in out:
                a.setflags(write=False)
            self._ref[key] = out
        return self._ref[key]


def differing_pixels(a, b):
    return int((a != b).any(-1).sum())


def min_pair_difference(sq, name, w, h):
    """(fewest differing pixels over all pairs of the sequence's frames, the pair)"""
    frames = [sq.ref(name, k, False, "view", w, h)[0] for k in range(len(sq.scenes(name)))]
    best = None
    for i in range(len(frames)):
        for j in range(i + 1, len(frames)):
            d = differing_pixels(frames[i], frames[j])
            if best is None or d < best[0]:
                best = (d, (i, j))
    return best
