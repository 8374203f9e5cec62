"""Ray sets and oracle references for sr_trace_ray_maps (a helper, not a test
module).

sr.h "Ray maps of ray queries" defines the maps of a traced ray as what "Ray
maps" gives pixel (0, 0) of the 1x1 frame by which "Ray queries" defines the
ray. Both halves are already tied to the unchanged oracle: a ray is a 1x1
oracle frame (tests/trace_cases.py ray_frames), and the maps are whatever makes
the oracle's own arithmetic, restated in numpy (tests/ray_map_cases.py
sky_uv_np and deferred_np), reproduce that frame's FragColor. Nothing new is
needed of the oracle.

probe_rays: the CPU cases' rays, which start at origins of their own (the
frames of tests/test_ray_map_cases.py all start at one camera position).

TraceMaps: the scattered sets of tests/trace_cases.py under the light rig of
tests/ray_map_cases.py, with the 1x1 oracle frames under the random sky and
under the 1x1 black and white skies of check_end's rule, made once per
session.
"""
from __future__ import annotations

import numpy as np

import extreme_cases as X
import ray_map_cases as R
import trace_cases as T

F = np.float32
N_ORIGINS, N_DIRS = 24, 20
MIN_END_SKY_SHARE = 0.05  # of a scattered set's finite rays: those whose black- and white-sky frames differ


def targets(scene):
    """(centre, extent) of a CPU case's objects: a sphere's radius, half a rectangle's larger side."""
    out = []
    for i in range(int(scene.num_objects)):
        t, rec = T.transform_of(scene, i)
        o = scene.objects[i]
        if int(o.type) == X.TYPE_OF["sphere"]:
            ext = float(rec.radius)
        else:
            assert int(o.type) == X.TYPE_OF["rectangle"], o.type
            ext = 0.5 * max(float(rec.width), float(rec.height))
        out.append((np.array(list(t.pos), dtype=np.float64), ext))
    return out


def probe_rays(scene, seed=5):
    """(origins [480, 3], dirs [480, 3]) float32: N_ORIGINS origins in front of
    the case's objects, N_DIRS directions from each, aimed at an object's
    centre jittered by +-1 extent (every fourth by +-2.5: past its edge) and
    scaled by a factor in [0.2, 5], so no V is normalised."""
    rng = np.random.default_rng(seed)
    tg = targets(scene)
    O, V = [], []
    for _ in range(N_ORIGINS):
        o = np.array([rng.uniform(-5.0, 5.0), rng.uniform(-4.0, 4.0), rng.uniform(9.0, 15.0)])
        for j in range(N_DIRS):
            c, ext = tg[int(rng.integers(len(tg)))]
            aim = c + rng.uniform(-1.0, 1.0, size=3) * ext * (2.5 if j % 4 == 3 else 1.0)
            v = aim - o
            O.append(o)
            V.append(v / np.linalg.norm(v) * rng.uniform(0.2, 5.0))
    O, V = np.array(O).astype(F), np.array(V).astype(F)
    assert not (np.signbit(V) & (V == 0)).any()
    return O, V


def start_dirs(V):
    """The direction a traced ray's walk starts with: normalize(+0 + V) in binary32 (frag:863 on the 1x1 frame)."""
    return R.norm3(np.zeros(3, dtype=F) + np.asarray(V, dtype=F))


_REFS = {}


class TraceMaps:
    """The rigged scattered sets and their oracle references, made once per session and read-only."""

    def __init__(self, pkg, oracle, textures):
        self.pkg, self.oracle = pkg, oracle
        self.tr = T.Traces(pkg, oracle, textures)
        self.arr = textures[1]
        self.sky = R.random_sky()
        # check_end's skies (tests/test_gpu_ray_maps.py): RGBA, so that a ray whose colour is NaN under both
        # still shows in its alpha whether a get_bg term was added
        self.skies = {"random": self.sky, "black": np.array([[[0, 0, 0, 255]]], dtype=np.uint8),
                      "white": np.array([[[255, 255, 255, 0]]], dtype=np.uint8)}
        self._tex = {}
        self._c = _REFS

    def tex(self, sky):
        if sky not in self._tex:
            self._tex[sky] = self.oracle.TextureSet(self.skies[sky], self.arr)
        return self._tex[sky]

    def scene(self, key):
        """A scattered set's scene under the light rig (shading fields only: the geometry and the classes stay)."""
        k = ("rigged", key)
        if k not in self._c:
            self._c[k] = R.rigged(self.pkg, self.tr.scene(key))
        return self._c[k]

    def rays(self, key):
        return self.tr.rays(key)

    def params(self, steps=T.STEPS, **kw):
        return self.tr.params(steps, **kw)

    def frames(self, scene, O, V, params, overlay, sky="random"):
        """(float FragColor [N, 4], steps [N]) of rays, one 1x1 oracle frame each."""
        _, f, s = T.ray_frames(self.pkg, self.oracle, scene, O, V, params, self.tex(sky), self.tr.wd.test_rays[overlay])
        return f, s

    def ref(self, key, overlay, mode=T.CURVED, sky="random", steps=T.STEPS, **prm):
        """(float FragColor, steps) of the rigged set, read-only."""
        k = ("ref", key, overlay, mode, sky, steps, tuple(sorted(prm.items())))
        if k not in self._c:
            O, V, _ = self.rays(key)
            out = self.frames(self.scene(key), O, V, self.params(steps, raytrace_type=mode, **prm), overlay, sky)
            for a in out:
                a.setflags(write=False)
            self._c[k] = out
        return self._c[k]

    def ends_in_sky(self, key, overlay, mode=T.CURVED, steps=T.STEPS, **prm):
        """check_end's rule: the rays whose frames under the black and the white sky differ (rgb or alpha, as bits)."""
        black = self.ref(key, overlay, mode, "black", steps, **prm)[0]
        white = self.ref(key, overlay, mode, "white", steps, **prm)[0]
        return ~R.same_bits(black, white).all(-1)
