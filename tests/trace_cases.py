"""Ray sets for sr_trace_rays and their references from the unchanged oracle
(a helper, not a test module).

sr.h "Ray queries" defines ray i of a trace launch as pixel (0, 0) of a 1x1
pinhole frame of fov 90 with the camera at the ray's origin O and the camera
axes (0, 0, V) (tests/projection_cases.py has the method for a fixed camera
position: here the position moves with the ray). So the oracle needs no new
code:

- a camera-ray set (the rays sr_camera_rays gives for a w x h pinhole frame)
  takes one oracle frame, the frame itself;
- a scattered set takes one 1x1 oracle frame per ray (ray_frames).

Pick codes come by tests/pick_cases.py's method: the oracle's frames of the
recoloured scene (unlit, one colour per object) decoded to object codes. The
kernel's ids are held to them on that recoloured scene: an id depends on the
geometry and on the materials' sidedness alone, which recolouring keeps where
it matters (pick_cases.recoloured makes every object double-sided but the
ones a case flags).

The scattered sets (SCATTERED) are built on two scenes:

  "default"  the default scene's objects, with the accretion annulus and the
             rectangle given an untextured material of alpha 0.5: the
             unmodified default scene has no translucent surface, and the
             sets must send rays through one (tests/test_trace_cases.py);
  "large"    the 21-object stress scene (translucent materials, planes).

Origins: 22 points at r from 1.2 to 60 around the hole in random directions,
then the special ones (SPECIAL_ORIGINS): r = 1 exactly, r = 0.5, the centre,
r = 100 and a float either side of it, r = 150, 1e5 and 1e25, a point on the
first sphere's surface, a float either side of the first rectangle's plane,
inside the first box, inside the first sphere, and three non-finite points.
Every origin is paired with a menu of directions (directions()): aimed at
object centres, at the hole and at empty sky, exactly radial inward and
outward and a hair off the radius, tangential, zero, of length 1e-20 and 1e20, with -0 components, NaN.

A ray is *finite* when every component of its origin and direction is finite
and neither is zero; tests/test_trace_cases.py shows on the oracle alone that
among the finite rays of each set the classes of classify() hold their shares.
"""
from __future__ import annotations

import numpy as np

import extreme_cases as X
import pick_cases as K
from test_gpu_launch_matrix import World

F = np.float32
CURVED, FLAT = 0, 1  # sr.h SR_RAYTRACE_*
STEPS = 400
W, H = 68, 44  # the camera-ray sets' frame: every wave shape partial somewhere
# (scene key of World, overlay)
CAMERA_SETS = (("small", False), ("small", True), ("large", False), ("large", True), ("stacked", False))
SCATTERED = (("default", False), ("default", True), ("large", False), ("large", True))
NAN, INF = float("nan"), float("inf")
TRANSLUCENT_OBJECTS = {"default": (2, 4), "large": ()}  # the objects given the alpha-0.5 material
MIN_SHARE, MIN_ORIGIN_DEPENDENT = 0.05, 20
TYPE_ARRAY = {v: X.ARRAY_OF[k] for k, v in X.TYPE_OF.items()}


def transform_of(scene, i):
    o = scene.objects[i]
    rec = getattr(scene, TYPE_ARRAY[int(o.type)])[int(o.index)]
    return rec.plane.transform if hasattr(rec, "plane") else rec.transform, rec


def centres(scene):
    return [np.array(list(transform_of(scene, i)[0].pos), dtype=np.float64) for i in range(int(scene.num_objects))]


def first_of(scene, kind):
    """(transform, record) of the scene's first object of a type (extreme_cases.TYPE_OF)."""
    for i in range(int(scene.num_objects)):
        if int(scene.objects[i].type) == X.TYPE_OF[kind]:
            return transform_of(scene, i)
    raise LookupError(kind)


def scattered_scene(pkg, key):
    sc, abi = pkg.scenes, pkg.abi
    if key == "large":
        return sc.scene_stress()
    s = sc.scene_default(True)
    m = s.materials[3]
    X.plain_material(m, (0.2, 0.6, 0.9, 0.5))
    m.double_sided_normals = 1
    for i in TRANSLUCENT_OBJECTS[key]:
        s.objects[i].material_index = 3
    return s


def opaque_copy(pkg, scene):
    """The scene with every material untextured and of alpha 1: a ray whose
    step count differs from this scene's crossed a translucent surface."""
    s = pkg.scenes.struct_from_bytes(pkg.abi.Scene, pkg.scenes.struct_bytes(scene))
    for k in range(pkg.abi.MAX_MATERIALS):
        s.materials[k].texture_index = -1
        s.materials[k].color[3] = 1.0
    return s


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def special_origins(scene):
    sph_t, sph = first_of(scene, "sphere")
    rect_t, rect = first_of(scene, "rectangle")
    box_t, box = first_of(scene, "box")
    c = np.array(list(sph_t.pos), dtype=np.float64)
    r = float(sph.radius)
    out = [
        ("r=1", (0.0, 0.0, 1.0)), ("r=0.5", (0.3, 0.0, -0.4)), ("centre", (0.0, 0.0, 0.0)),
        ("r=100", (0.0, 100.0, 0.0)), ("r=100-", (0.0, float(np.nextafter(F(100), F(0))), 0.0)),
        ("r=100+", (0.0, float(np.nextafter(F(100), F(200))), 0.0)),
        ("r=150", tuple(150.0 * _unit((1.0, 2.0, -2.0)))), ("r=1e5", tuple(1.0e5 * _unit((-2.0, 1.0, 2.0)))),
        ("r=1e25", (0.0, 0.0, 1.0e25)),
        ("on-sphere", tuple(c + np.array([r, 0.0, 0.0]))),
        ("in-sphere", tuple(c + 0.3 * r * _unit((1.0, 1.0, 0.0)))),
    ]
    # a point of the rectangle, then a float either side of its plane along the normal's largest component
    ax = np.array(list(rect_t.axes), dtype=np.float64).reshape(3, 3)
    p = np.array(list(rect_t.pos), dtype=np.float64) + 0.3 * float(rect.width) * ax[0] + 0.3 * float(rect.height) * ax[2]
    p = p.astype(F)
    k = int(np.argmax(np.abs(ax[1])))
    for name, toward in (("rect-", -INF), ("rect+", INF)):
        q = p.copy()
        q[k] = np.nextafter(q[k], F(toward))
        out.append((name, tuple(float(v) for v in q)))
    bx = np.array(list(box_t.axes), dtype=np.float64).reshape(3, 3)
    inside = (np.array(list(box_t.pos), dtype=np.float64) + 0.5 * float(box.width) * bx[0] +
              0.5 * float(box.height) * bx[1] + 0.5 * float(box.depth) * bx[2])
    out.append(("in-box", tuple(inside)))
    out += [("nan", (NAN, 0.0, 5.0)), ("+inf", (INF, 0.0, 0.0)), ("-inf", (1.0, -INF, 1.0))]
    return out


def directions(rng, O, cs, n_aims, n_sky, special):
    """The menu of directions from origin O: (label, V) pairs."""
    O = np.asarray(O, dtype=np.float64)
    finite = bool(np.isfinite(O).all())
    o = O if finite else np.array([3.0, 2.0, 7.0])
    out = []
    for j in rng.choice(len(cs), size=n_aims, replace=False):
        out.append((f"obj{j}", cs[j] - o))
    out.append(("hole", -o + rng.normal(size=3) * 0.05))
    for _ in range(n_sky):
        out.append(("sky", rng.normal(size=3)))
    out.append(("radial-in", -o))
    out.append(("radial-out", o))
    t = np.cross(o, rng.normal(size=3))
    if not np.linalg.norm(t) > 0:
        t = np.array([0.0, 1.0, 0.0])
    out.append(("tangent", t))
    # a hair off the radius, beyond the radial test's 4.5e-4 rad: |u'| = u cot(angle) in the thousands
    tn = t / np.linalg.norm(t) * np.linalg.norm(o)
    out += [("near-out", o + 2.0e-3 * tn), ("near-in", -o + 2.0e-3 * tn), ("graze-out", o + 6.0e-4 * tn)]
    if special:
        u = _unit(rng.normal(size=3))
        out += [("zero", np.zeros(3)), ("tiny", 1.0e-20 * u), ("huge", 1.0e20 * u),
                ("-0a", np.array([-0.0, -0.3, -1.0])), ("-0b", np.array([1.0, -0.0, -0.0])),
                ("nan", np.array([0.2, NAN, 1.0]))]
    return out


def scattered_rays(pkg, key, seed=7):
    """(origins [N, 3], dirs [N, 3]) float32 and the rays' labels."""
    scene = scattered_scene(pkg, key)
    rng = np.random.default_rng(seed)
    cs = centres(scene)
    origins = []
    for r in np.exp(np.linspace(np.log(1.2), np.log(60.0), 22)):
        origins.append((f"r={r:.3g}", tuple(r * _unit(rng.normal(size=3))), False))
    origins += [(n, p, True) for n, p in special_origins(scene)]
    O, V, labels = [], [], []
    for name, p, special in origins:
        for lab, v in directions(rng, p, cs, 2 if special else 3, 3 if special else 7, special):
            O.append(p)
            V.append(v)
            labels.append(f"{name}/{lab}")
    with np.errstate(over="ignore"):
        return np.array(O, dtype=np.float64).astype(F), np.array(V, dtype=np.float64).astype(F), labels


def finite_rays(O, V):
    return np.isfinite(O).all(-1) & np.isfinite(V).all(-1) & (O != 0).any(-1) & (V != 0).any(-1)


def ray_frames(pkg, oracle, scene, O, V, params, tex, test_ray):
    """One 1x1 oracle frame per ray (the definition of sr.h "Ray queries") ->
    (rgba8 [N, 4], float rgba [N, 4], steps [N]). crosshair and the noise mask
    are off whatever params says."""
    p = pkg.scenes.struct_from_bytes(pkg.abi.Params, pkg.scenes.struct_bytes(params))
    p.crosshair, p.percent_black = 0, -1.0
    c = pkg.abi.Camera()
    c.fov = 90.0
    for k in range(9):
        c.transform.axes[k] = 0.0
    n = len(O)
    b = np.zeros((n, 4), dtype=np.uint8)
    f = np.zeros((n, 4), dtype=F)
    s = np.zeros((n,), dtype=np.int32)
    for i in range(n):
        for k in range(3):
            c.transform.pos[k] = float(O[i, k])
            c.transform.axes[6 + k] = float(V[i, k])
        pb, pf, ps = oracle.render(scene, c, p, 1, 1, tex, test_ray, nthreads=1)
        b[i], f[i], s[i] = pb[0, 0], pf[0, 0], ps[0, 0]
    return b, f, s


def classify(codes, steps, max_steps, radius, uf_radius=100.0):
    """The classes of a curved set's rays, from the oracle's codes and steps
    and the origins' radii alone: "flat" (ended by the flat tail before any
    integration: the radial test at the start, 0 steps, the only way a launch
    of max_steps > 0 executes none; or a start beyond 1 / u_f whose line
    misses that sphere, 1 step and the sky), else "object", "hole" or "sky"
    by the code."""
    assert max_steps > 1
    flat = (steps == 0) | ((steps == 1) & (codes == K.SKY) & (radius > uf_radius))
    return {"flat": flat, "object": ~flat & (codes >= 0), "hole": ~flat & (codes == K.HOLE),
            "sky": ~flat & (codes == K.SKY)}


def camera_rays_numpy(cam, projection, w, h):
    """sr_camera_rays in numpy (projection_cases.local_dirs and world_dirs):
    (origins, dirs) float32 [h, w, 3], NaN directions where a pixel has no ray."""
    import projection_cases as P

    L, ray = P.local_dirs(projection, cam.fov, w, h)
    V = P.world_dirs(cam, L).copy()
    V[~ray] = np.nan
    O = np.broadcast_to(np.array(list(cam.transform.pos), dtype=F), (h, w, 3)).copy()
    return O, V


_SETS = {}


class Traces:
    """The ray sets and their oracle references, made once per session and read-only."""

    def __init__(self, pkg, oracle, textures):
        self.pkg, self.oracle = pkg, oracle
        self.wd = World(pkg, oracle, textures)
        self.picks = K.Picks(pkg, oracle, textures)
        self.tex = self.wd.tex
        self._c = _SETS

    def params(self, steps=STEPS, **kw):
        p = self.wd.params(steps)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def _memo(self, key, make):
        if key not in self._c:
            out = make()
            for a in out:
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            self._c[key] = out
        return self._c[key]

    # ---- camera-ray sets
    def camera_set(self, key, overlay):
        """(origins [N, 3], dirs [N, 3]) of the W x H "view" frame, row-major."""
        def make():
            O, V = camera_rays_numpy(self.wd.cams["view"], 0, W, H)
            assert not (np.signbit(V) & (V == 0)).any(), "a -0 component: the trace's 0 + V would lose its sign"
            return O.reshape(-1, 3), V.reshape(-1, 3)
        return self._memo(("camrays",), make)

    def camera_ref(self, key, overlay):
        b, f, s = self.wd.ref(key, overlay)
        return b.reshape(-1, 4), f.reshape(-1, 4), s.reshape(-1)

    # ---- scattered sets
    def scene(self, key):
        return self._memo(("scene", key), lambda: (scattered_scene(self.pkg, key),))[0]

    def rays(self, key):
        return self._memo(("rays", key), lambda: scattered_rays(self.pkg, key))

    def scattered_ref(self, key, overlay, mode=CURVED, **prm):
        """(rgba8, float rgba, steps) of the set, one 1x1 oracle frame per ray."""
        O, V, _ = self.rays(key)
        k = ("ref", key, overlay, mode, tuple(sorted(prm.items())))
        return self._memo(k, lambda: ray_frames(self.pkg, self.oracle, self.scene(key), O, V,
                                                self.params(raytrace_type=mode, **prm), self.tex,
                                                self.wd.test_rays[overlay]))

    # ---- pick codes of the scattered sets (pick_cases' method)
    def pick_passes(self, key):
        flags = {i: {"translucent": True} for i in TRANSLUCENT_OBJECTS[key]}
        return self._memo(("passes", key), lambda: tuple(K.recoloured(self.pkg, self.scene(key), flags)))

    def pick_test_ray(self, overlay):
        return self.picks.test_rays[overlay]

    def scattered_codes(self, key, overlay, mode=CURVED):
        """(codes [N], decoded-exactly-once [N]) of the set on the recoloured scene."""
        def make():
            O, V, _ = self.rays(key)
            frames = [ray_frames(self.pkg, self.oracle, s, O, V, self.params(raytrace_type=mode), self.picks.tex,
                                 self.pick_test_ray(overlay))[1][:, None, :] for s in self.pick_passes(key)]
            codes, ok = K.decode(frames, int(self.scene(key).num_objects), bool(TRANSLUCENT_OBJECTS[key]))
            return codes[:, 0], ok[:, 0]
        return self._memo(("codes", key, overlay, mode), make)

    def translucent_crossings(self, key, overlay):
        """Rays whose step count changes when every material is made opaque."""
        def make():
            O, V, _ = self.rays(key)
            s0 = self.scattered_ref(key, overlay)[2]
            s1 = ray_frames(self.pkg, self.oracle, opaque_copy(self.pkg, self.scene(key)), O, V, self.params(),
                            self.tex, self.wd.test_rays[overlay])[2]
            return (s0 != s1,)
        return self._memo(("crossings", key, overlay), make)[0]

    def origin_dependent(self, key, overlay):
        """Rays whose result changes when only the origin is replaced by the set's first."""
        def make():
            O, V, _ = self.rays(key)
            b0, f0, s0 = self.scattered_ref(key, overlay)
            O1 = np.broadcast_to(O[0], O.shape).copy()
            b1, f1, s1 = ray_frames(self.pkg, self.oracle, self.scene(key), O1, V, self.params(), self.tex,
                                    self.wd.test_rays[overlay])
            return ((b0 != b1).any(-1) | (s0 != s1),)
        return self._memo(("origin", key, overlay), make)[0]
