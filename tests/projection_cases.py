"""Projected frames from the unchanged oracle, one pixel at a time (a helper,
not a test module).

sr_set_projection (sr.h "Projections") chooses how a pixel's local direction L
is formed; everything after rd = normalize(axes * L) is the reference's. The
oracle renders the reference's pinhole only, but a pixel of any projection is,
bit for bit, pixel (0, 0) of a 1x1 pinhole frame:

- let V = axes * L = (c0 * L.x + c1 * L.y) + c2 * L.z in binary32 (world_dirs);
- a 1x1 frame has uv = (0, 0), and fov 90 a forward term of exactly 1.0f, so
  with camera axes (0, 0, V) the oracle forms normalize((0 * 0 + 0 * 0) + V * 1)
  = normalize(V): the projected pixel's ray, from the same position;
- crosshair = 0 and percent_black < 0 keep the 1x1 frame's own uv = 0 out of
  the pixel (the crosshair and the noise mask are functions of the real
  frame's uv; tests/test_gpu_projection.py checks them against the
  rectilinear frame of the same size);
- raytrace_type is CURVED or FLAT as the pixel's own split rule on uv says.

One condition: 0 + V turns a -0 component into +0 where the kernel keeps it,
so the builder asserts that no V has a -0 component.

tests/test_projection_cases.py shows on the oracle alone that the method,
applied to the rectilinear L, reproduces the oracle's own frames.

local_dirs is the numpy statement of L (binary32 in the order of sr.h; sin and
cos are libm's binary64 functions rounded once), which
tests/test_projection_host.py holds sr_projection_dir to, bit for bit.
"""
from __future__ import annotations

import math

import numpy as np

from test_gpu_launch_matrix import World

RECTILINEAR, EQUIRECT, FISHEYE = 0, 1, 2  # sr.h SR_PROJECTION_*
NAMES = {RECTILINEAR: "rectilinear", EQUIRECT: "equirect", FISHEYE: "fisheye"}
F = np.float32
PI = F(3.1415926535)  # frag:10
CURVED, FLAT, HALF_WIDTH, HALF_HEIGHT = 0, 1, 2, 3  # sr.h SR_RAYTRACE_*


def _sin(x):
    return np.array([math.sin(float(v)) for v in np.ravel(x)], dtype=np.float64).astype(F).reshape(np.shape(x))


def _cos(x):
    return np.array([math.cos(float(v)) for v in np.ravel(x)], dtype=np.float64).astype(F).reshape(np.shape(x))


def uv_of(w, h):
    """(uv.x [h, w], uv.y [h, w]) of a w x h frame, binary32 (full_screen_quad.vert:7-10)."""
    x = (2 * np.arange(w) + 1).astype(F) / F(w) - F(1)
    y = (2 * np.arange(h) + 1).astype(F) / F(h) - F(1)
    return np.broadcast_to(x[None, :], (h, w)).copy(), np.broadcast_to(y[:, None], (h, w)).copy()


def half_angle(fov):
    return F(fov) / F(360.0) * PI


def local_dirs(projection, fov, w, h):
    """(L [h, w, 3] float32, has_ray [h, w] bool) by sr.h's rule; L of a pixel
    without a ray is zero."""
    ux, uy = uv_of(w, h)
    vx, vy = ux, uy * F(h) / F(w)
    a = half_angle(fov)
    L = np.zeros((h, w, 3), dtype=F)
    ray = np.ones((h, w), dtype=bool)
    if projection == RECTILINEAR:
        L[..., 0], L[..., 1] = vx, vy
        L[..., 2] = F(1) / F(math.tan(float(a)))
    elif projection == EQUIRECT:
        lon, lat = vx * a, vy * a
        cl = _cos(lat)
        L[..., 0], L[..., 1], L[..., 2] = cl * _sin(lon), _sin(lat), cl * _cos(lon)
    elif projection == FISHEYE:
        rho = np.sqrt(vx * vx + vy * vy)
        th = rho * a
        ray = th <= PI  # a NaN has no ray
        s = _sin(th)
        pos = rho > 0
        safe = np.where(pos, rho, F(1))
        L[..., 0] = np.where(pos, s * (vx / safe), F(0))
        L[..., 1] = np.where(pos, s * (vy / safe), F(0))
        L[..., 2] = np.where(pos, _cos(th), F(1))
        L[~ray] = 0
    else:
        raise ValueError(projection)
    assert L.dtype == F
    return L, ray


def world_dirs(cam, L):
    """V = axes * L in binary32, the kernel's mv: (c0 * L.x + c1 * L.y) + c2 * L.z."""
    ax = np.array(list(cam.transform.axes), dtype=F)
    c0, c1, c2 = ax[0:3], ax[3:6], ax[6:9]
    V = (c0 * L[..., 0:1] + c1 * L[..., 1:2]) + c2 * L[..., 2:3]
    assert V.dtype == F
    return V


def flat_mask(params, w, h):
    """The pixels the split rule sends along straight rays (frag:874-876)."""
    ux, uy = uv_of(w, h)
    edge = F(2.0) * F(params.curved_percentage) + F(-1.0)
    t = int(params.raytrace_type)
    if t == FLAT:
        return np.ones((h, w), dtype=bool)
    if t == HALF_WIDTH:
        return ux > edge
    if t == HALF_HEIGHT:
        return uy > edge
    return np.zeros((h, w), dtype=bool)


def copy_struct(pkg, cls, s):
    return pkg.scenes.struct_from_bytes(cls, pkg.scenes.struct_bytes(s))


def with_fov(pkg, cam, fov):
    c = copy_struct(pkg, pkg.abi.Camera, cam)
    if fov is not None:
        c.fov = float(fov)
    return c


def pixel_frame(pkg, oracle, scene, cam, params, w, h, projection, tex, test_ray=None):
    """The projected w x h frame (rgba8, float rgba, steps) from 1x1 oracle
    frames. The crosshair and the noise mask are off whatever params says
    (module docstring); a pixel without a ray is zero with 0 steps."""
    L, ray = local_dirs(projection, cam.fov, w, h)
    V = world_dirs(cam, L)
    assert not (np.signbit(V) & (V == 0))[ray].any(), "a -0 component: the oracle's 0 + V would lose its sign"
    flat = flat_mask(params, w, h)
    p = copy_struct(pkg, pkg.abi.Params, params)
    p.crosshair, p.percent_black = 0, -1.0
    c = copy_struct(pkg, pkg.abi.Camera, cam)
    c.fov = 90.0
    for k in range(6):
        c.transform.axes[k] = 0.0
    b = np.zeros((h, w, 4), dtype=np.uint8)
    f = np.zeros((h, w, 4), dtype=F)
    s = np.zeros((h, w), dtype=np.int32)
    for y in range(h):
        for x in range(w):
            if not ray[y, x]:
                continue
            for k in range(3):
                c.transform.axes[6 + k] = float(V[y, x, k])
            p.raytrace_type = FLAT if flat[y, x] else CURVED
            pb, pf, ps = oracle.render(scene, c, p, 1, 1, tex, test_ray, nthreads=1)
            b[y, x], f[y, x], s[y, x] = pb[0, 0], pf[0, 0], ps[0, 0]
    return b, f, s


def box_average(samples, ss):
    """sr_resolve_box in numpy: (sum + n / 2) / n per channel over ss x ss."""
    hh, ww, _ = samples.shape
    h, w = hh // ss, ww // ss
    t = samples.reshape(h, ss, w, ss, 4).astype(np.uint32).sum(axis=(1, 3))
    n = ss * ss
    return ((t + n // 2) // n).astype(np.uint8)


# ---- the cases ---------------------------------------------------------------------
# (id, projection, w, h, fov; None: the camera's own)
CASES = [
    ("equirect-68x44-fov120", EQUIRECT, 68, 44, 120.0),  # every wave shape partial
    ("fisheye-68x44-fov120", FISHEYE, 68, 44, 120.0),
    ("equirect-33x17-own", EQUIRECT, 33, 17, None),
    ("fisheye-33x17-own", FISHEYE, 33, 17, None),
    ("equirect-64x32-fov360", EQUIRECT, 64, 32, 360.0),  # the whole sphere
    ("fisheye-41x41-fov180", FISHEYE, 41, 41, 180.0),  # a dome master, its centre pixel at rho == 0
    ("fisheye-48x48-fov360", FISHEYE, 48, 48, 360.0),  # corners beyond th = PI: no ray
    ("equirect-1x1", EQUIRECT, 1, 1, None),
    ("fisheye-1x1", FISHEYE, 1, 1, None),
]
BY_ID = {c[0]: c for c in CASES}
BIG = ("equirect-68x44-fov120", "fisheye-68x44-fov120")
# (scene key of test_gpu_launch_matrix.World, overlay) -> the cases it renders
CELLS = {
    ("small", False): tuple(c[0] for c in CASES),
    ("small", True): BIG,
    ("large", False): BIG + ("equirect-64x32-fov360", "fisheye-41x41-fov180", "fisheye-48x48-fov360"),
    ("large", True): BIG,
    ("stacked", False): BIG,
}
STEPS = 400
# the frames of every Projected of the session (World's scenes, cameras and
# textures are the same in each): the CPU and the GPU modules share them
_REF = {}


class Projected:
    """World's scenes, cameras and test rays with the projected oracle frames, made once."""

    def __init__(self, pkg, oracle, textures):
        self.pkg, self.oracle = pkg, oracle
        self.wd = World(pkg, oracle, textures)
        self.tex = self.wd.tex
        self._ref = _REF

    def cam(self, name, fov=None):
        return with_fov(self.pkg, self.wd.cams[name], fov)

    def params(self, steps=STEPS, **kw):
        p = self.wd.params(steps)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def ref(self, key, overlay, projection, w, h, fov=None, cam="view", steps=STEPS, scene=None, tex=None,
            test_ray=None, tag=None, **prm):
        """(rgba8, float rgba, steps) of the projected frame, read-only.
        scene / tex / test_ray replace the cell's own (name them with tag)."""
        k = (key, overlay, projection, w, h, fov, cam, steps, tag, tuple(sorted(prm.items())))
        if k not in self._ref:
            out = pixel_frame(self.pkg, self.oracle, scene if scene is not None else self.wd.scene(key),
                              self.cam(cam, fov), self.params(steps, **prm), w, h, projection,
                              tex if tex is not None else self.tex,
                              test_ray if test_ray is not None else self.wd.test_rays[overlay])
            for a in out:
                a.setflags(write=False)
            self._ref[k] = out
        return self._ref[k]

    def case_ref(self, key, overlay, case_id):
        _, projection, w, h, fov = BY_ID[case_id]
        return self.ref(key, overlay, projection, w, h, fov)
