"""Scenes, adversarial chords, anchors and binary64 references for the culling
bounds of geodesic.hip (tests/test_bound_cases.py on the CPU,
tests/test_gpu_bounds.py on the device). Host only, fixed seeds.

Everything is built in binary64 and rounded to binary32 at the end. A chord is
a row {o[3], d[3], seg} (intersect()'s origin, unit direction and max_lambda).

Families of one primitive (`families`):
  graze_*   the chord meets the primitive's surface (or its plane / tube) at a
            point at extent x (1 + delta) of a rim, corner, edge, tube or
            sphere, |delta| = 1e-9 .. 1e-1 of either sign: inside (a hit) for
            delta < 0, outside (a miss) for delta > 0, undecided by rounding
            within a few ulp. The approach point lies inside and just outside
            the primitive's other bounds. Origins 1e-2 .. 60 away.
  far       the same with origins 60 .. 1e4 away (S is large)
  short     the same with origins 1e-6 .. 1e-2 away (chords of 1e-6 .. 1e-2)
  end       a chord aimed at an inner point of the surface that ends at
            lambda_hit x (1 + delta), and chords whose origin lies a few
            floats either side of the surface
  parallel  planar: |n . d| = 1e-8 .. 1 through an inner point (SR_EPS = 1e-7
            lies inside); cylinders: 1e-7 rad off the axis to perpendicular
  control   chords at least 2 br + 0.1 (|o|_1 + seg + 1 + |pos|_1) from the
            bounding centre (orthonormal, bounded objects only)
  bound     chords tangent to the bounding sphere (their closest approach to bc
            is the point they aim at) at the primitive's farthest points - a
            disk's rim, a corner, a cylinder's end circles - moved in or out by
            1e-9 .. 1e-1 of S = |o|_1 + seg + 1: what may_hit's mu S, br's own
            margin and a cylinder's lateral margin decide
"""
import zlib
from dataclasses import dataclass

import numpy as np

import extreme_cases as X
import host_precompute_cases as HP

N = 384          # chords per family of a primitive alone
N_EMBEDDED = 96  # per family and object of a scene with several
N_BOUND_FAR = 65536  # the far tangent chords of a small cylinder (few are accepted)
DELTA_LO, DELTA_HI = -9.0, -1.0
TYPES = ("sphere", "plane", "disk", "annulus", "cylinder", "rectangle", "box")
NAME_OF = {v: k for k, v in X.TYPE_OF.items()}
PERRS = (0.0, 1e-6, 1e-4, 1e-2)


# ---- small vector helpers (binary64) ----------------------------------------------
def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def random_units(rng, n):
    return unit(rng.normal(size=(n, 3)))


def perpendicular(rng, e):
    """Random unit vectors perpendicular to the unit vectors e [n, 3]."""
    v = rng.normal(size=e.shape)
    v -= e * np.sum(v * e, axis=-1, keepdims=True)
    bad = np.linalg.norm(v, axis=-1) < 1e-6
    v[bad] = np.cross(e[bad], np.eye(3)[np.argmin(np.abs(e[bad]), axis=-1)])
    return unit(v)


def log_uniform(rng, lo, hi, n):
    return 10.0 ** rng.uniform(np.log10(lo), np.log10(hi), n)


def deltas(rng, n):
    """|delta| = 1e-9 .. 1e-1, either sign."""
    return rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(DELTA_LO, DELTA_HI, n)


def l1(v):
    return np.sum(np.abs(v), axis=-1)


# ---- binary64 references --------------------------------------------------------------
def dist_sphere(p, c, r):
    return np.abs(np.linalg.norm(p - c, axis=-1) - abs(r))


def dist_plane(p, pos, n):
    return np.abs(np.sum((p - pos) * n, axis=-1))


def _planar(p, pos, n):
    q = p - pos
    y = np.sum(q * n, axis=-1)
    rho = np.sqrt(np.maximum(0.0, np.sum(q * q, axis=-1) - y * y))
    return y, rho


def dist_disk(p, pos, n, r):
    y, rho = _planar(p, pos, n)
    return np.hypot(np.maximum(0.0, rho - abs(r)), y)


def dist_annulus(p, pos, n, r_in, r_out):
    y, rho = _planar(p, pos, n)
    lo, hi = abs(r_in), abs(r_out)
    return np.hypot(np.maximum(0.0, np.maximum(lo - rho, rho - hi)), y)


def dist_rectangle(p, pos, a0, a1, a2, w, h):
    q = p - pos
    x, y, z = (np.sum(q * a, axis=-1) for a in (a0, a1, a2))
    ex = np.maximum(0.0, np.maximum(-x, x - w))
    ez = np.maximum(0.0, np.maximum(-z, z - h))
    return np.sqrt(ex * ex + y * y + ez * ez)


def dist_box(p, pos, a0, a1, a2, width, depth, height):
    """To the solid box (0 inside): at most the distance to its faces."""
    q = p - pos
    x, y, z = (np.sum(q * a, axis=-1) for a in (a0, a1, a2))
    e = [np.maximum(0.0, np.maximum(-v, v - s)) for v, s in ((x, width), (y, height), (z, depth))]
    return np.sqrt(e[0] ** 2 + e[1] ** 2 + e[2] ** 2)


def dist_cylinder_lateral(p, pos, a1, height, r):
    """To the lateral surface rho = r, 0 <= y <= height (no caps)."""
    y, rho = _planar(p, pos, a1)
    ey = np.maximum(0.0, np.maximum(-y, y - height))
    return np.hypot(rho - abs(r), ey)


def dist_point_segment(p, a, b):
    ab = b - a
    den = np.sum(ab * ab, axis=-1)
    t = np.clip(np.sum((p - a) * ab, axis=-1) / np.where(den > 0, den, 1.0), 0.0, 1.0)
    return np.linalg.norm(p - (a + ab * t[..., None]), axis=-1)


def dist_capsule(p, a, b, r):
    """To the capsule of radius r around the segment [a, b] (0 inside)."""
    return np.maximum(0.0, dist_point_segment(p, a, b) - r)


def dist_segment_sphere(o, e, c, r):
    """From the segment [o, e] to the ball of radius r around c (0: they meet)."""
    return np.maximum(0.0, dist_point_segment(np.asarray(c, dtype=np.float64), o, e) - r)


# ---- primitives -----------------------------------------------------------------------
@dataclass
class Prim:
    """One primitive of a scene, in binary64 (the float32 values of its record)."""
    kind: str
    index: int          # in scene.objects[]
    pos: np.ndarray
    axes: np.ndarray    # rows a0, a1, a2 (the record's columns)
    size: tuple         # the record's sizes, as given (signed)

    @property
    def finite(self):
        return bool(np.all(np.isfinite(self.pos)) and np.all(np.isfinite(self.axes)) and np.all(np.isfinite(self.size)))

    @property
    def orthonormal(self):
        """The packer's test (precompute.cpp orthonormal, 1e-5)."""
        g = self.axes @ self.axes.T
        return bool(np.all(np.abs(g - np.eye(3)) < 1e-5))

    @property
    def unit_normal(self):
        return bool(abs(self.axes[1] @ self.axes[1] - 1.0) < 1e-5)

    @property
    def inv(self):
        """M^-1 for M's rows a0, a1, a2: q = inv @ (alpha, y, beta)."""
        return np.linalg.inv(self.axes)

    def bound_radius(self):
        """The radius of the bounding sphere the packer takes before its margins
        (precompute.cpp pack_object; orthonormal frames), binary64; None for a plane."""
        s = [abs(v) for v in self.size]
        return {"sphere": lambda: s[0], "plane": lambda: None, "disk": lambda: s[0], "annulus": lambda: s[1],
                "cylinder": lambda: float(np.hypot(s[1], 0.5 * s[0])),
                "rectangle": lambda: 0.5 * float(np.hypot(s[0], s[1])),
                "box": lambda: 0.5 * float(np.sqrt(s[0] ** 2 + s[1] ** 2 + s[2] ** 2))}[self.kind]()

    def dist(self, p):
        """Binary64 distance from the points p [n, 3] (orthonormal frames; disks need a unit normal)."""
        a0, a1, a2 = self.axes
        k, s = self.kind, self.size
        if k == "sphere":
            return dist_sphere(p, self.pos, s[0])
        if k == "plane":
            return dist_plane(p, self.pos, a1)
        if k == "disk":
            return dist_disk(p, self.pos, a1, s[0])
        if k == "annulus":
            return dist_annulus(p, self.pos, a1, s[0], s[1])
        if k == "rectangle":
            return dist_rectangle(p, self.pos, a0, a1, a2, s[0], s[1])
        if k == "box":
            return dist_box(p, self.pos, a0, a1, a2, s[0], s[1], s[2])
        if k == "cylinder":
            return dist_cylinder_lateral(p, self.pos, a1, s[0], s[1])
        raise ValueError(k)


def _f64(a):
    return np.array([float(v) for v in a], dtype=np.float64)


def prims_of(scene):
    """The scene's objects as Prims (read back from the ctypes record: binary32 values)."""
    out = []
    for i in range(scene.num_objects):
        o = scene.objects[i]
        kind = NAME_OF.get(o.type)
        if kind is None or not 0 <= o.index < 3:
            continue
        rec = getattr(scene, X.ARRAY_OF[kind])[o.index]
        if kind in ("sphere", "cylinder", "box"):
            t = rec.transform
        elif kind == "plane":
            t = rec.transform
        else:
            t = rec.plane.transform
        size = {"sphere": lambda: (rec.radius,), "plane": lambda: (), "disk": lambda: (rec.radius,),
                "annulus": lambda: (rec.inner_radius, rec.outer_radius),
                "cylinder": lambda: (rec.height, rec.radius), "rectangle": lambda: (rec.width, rec.height),
                "box": lambda: (rec.width, rec.depth, rec.height)}[kind]()
        out.append(Prim(kind, i, _f64(t.pos), _f64(t.axes).reshape(3, 3), tuple(float(v) for v in size)))
    return out


HOLE = Prim("sphere", -1, np.zeros(3), np.eye(3), (1.0,))  # the r = 1 shell (winner SLOT_BH)


# ---- surface features -------------------------------------------------------------------
@dataclass
class Feature:
    """Points P0 on a rim / edge / tube / sphere, the unit direction e in which
    the primitive's extent grows there, the extent, and the surface normal n
    there for a surface the chord crosses (None: the chord is tangent, its
    direction perpendicular to e)."""
    name: str
    P0: np.ndarray
    e: np.ndarray
    ext: np.ndarray
    n: np.ndarray | None
    d: np.ndarray | None = None  # a tangent chord's direction (None: any perpendicular to e)


def _ring(rng, a0, a2, n):
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    return np.cos(phi)[:, None] * a0 + np.sin(phi)[:, None] * a2


def _inplane_basis(n):
    """Two unit vectors spanning the plane of (not necessarily unit) normal n."""
    n = unit(n)
    t = np.eye(3)[np.argmin(np.abs(n))]
    u = unit(t - n * (t @ n))
    return u, np.cross(n, u)


def features(p: Prim, rng, n):
    """The grazing features of a primitive."""
    a0, a1, a2 = p.axes
    k, s = p.kind, [abs(v) for v in p.size]
    out = []
    if k == "sphere":
        e = random_units(rng, n)
        out.append(Feature("sphere", p.pos + e * s[0], e, np.full(n, s[0]), None))
    elif k in ("disk", "annulus"):
        u, v = _inplane_basis(a1)
        for label, r, sign in ([("rim", s[0], 1.0)] if k == "disk" else [("inner", s[0], -1.0), ("outer", s[1], 1.0)]):
            e = _ring(rng, u, v, n)
            out.append(Feature(label, p.pos + e * r, e * sign, np.full(n, r), np.broadcast_to(unit(a1), (n, 3))))
    elif k == "cylinder":
        e = _ring(rng, unit(a0), unit(a2), n)
        # the tube: tangent chords at heights inside and just outside [0, h]
        y = rng.uniform(-0.1, 1.1, n) * s[0]
        # (directions across the axis, along it by at most height / diameter: the
        # chord's two roots stay near the height of its closest approach)
        tang = np.cross(np.broadcast_to(unit(a1), (n, 3)), e)
        along = rng.uniform(-1.0, 1.0, n) * min(1.0, s[0] / (2.0 * s[1]) if s[1] > 0 else 1.0)
        d = unit(tang * rng.choice([-1.0, 1.0], n)[:, None] + unit(a1) * along[:, None])
        out.append(Feature("tube", p.pos + a1 * y[:, None] + e * s[1], e, np.full(n, s[1]), None, d))
        # the rims: chords crossing the tube's surface at height h (1 + delta) or -h delta
        top = rng.random(n) < 0.5
        e2 = _ring(rng, unit(a0), unit(a2), n)
        base = p.pos + e2 * s[1] + np.where(top[:, None], a1 * s[0], 0.0)
        out.append(Feature("rim", base, np.where(top[:, None], unit(a1), -unit(a1)), np.full(n, s[0]), e2))
    elif k in ("rectangle", "box"):
        inv = p.inv
        w, h = (s[0], s[1])  # the rectangle's, or the box's top face (width x depth)
        origin = p.pos + (a1 * s[2] if k == "box" else 0.0)
        nrm = unit(a1)
        c0, c2 = inv[:, 0], inv[:, 2]  # q moves by these per unit of alpha, beta
        # an edge: alpha = w (1 + delta) or -w delta, beta inside and just outside [0, h]
        hi = rng.random(n) < 0.5
        beta = rng.uniform(-0.1, 1.1, n) * h
        P0 = origin + np.where(hi[:, None], c0 * w, 0.0) + beta[:, None] * c2
        e = np.where(hi[:, None], c0, -c0)
        out.append(Feature("edge", P0, unit(e), np.full(n, w) * np.linalg.norm(c0), np.broadcast_to(nrm, (n, 3))))
        # the other edge
        hi = rng.random(n) < 0.5
        alpha = rng.uniform(-0.1, 1.1, n) * w
        P0 = origin + np.where(hi[:, None], c2 * h, 0.0) + alpha[:, None] * c0
        e = np.where(hi[:, None], c2, -c2)
        out.append(Feature("edge2", P0, unit(e), np.full(n, h) * np.linalg.norm(c2), np.broadcast_to(nrm, (n, 3))))
        # a corner: both at once, along the diagonal
        ha, hb = rng.random(n) < 0.5, rng.random(n) < 0.5
        P0 = origin + np.where(ha[:, None], c0 * w, 0.0) + np.where(hb[:, None], c2 * h, 0.0)
        e = np.where(ha[:, None], c0 * w, -c0 * w) + np.where(hb[:, None], c2 * h, -c2 * h)
        ext = np.linalg.norm(e, axis=-1)
        e = np.where(ext[:, None] > 0, e / np.where(ext > 0, ext, 1.0)[:, None], unit(c0 + c2))
        out.append(Feature("corner", P0, e, ext, np.broadcast_to(nrm, (n, 3))))
    return out


def inner_points(p: Prim, rng, n):
    """(Q [n, 3], normal [n, 3]): points well inside the primitive's surface."""
    a0, a1, a2 = p.axes
    k, s = p.kind, [abs(v) for v in p.size]
    if k == "sphere":
        e = random_units(rng, n)
        return p.pos + e * s[0], e
    if k == "plane":
        u, v = _inplane_basis(a1)
        r = log_uniform(rng, 1e-2, 1e2, n)[:, None]
        return p.pos + _ring(rng, u, v, n) * r, np.broadcast_to(unit(a1), (n, 3))
    if k in ("disk", "annulus"):
        u, v = _inplane_basis(a1)
        lo, hi = (0.0, s[0]) if k == "disk" else (min(s), max(s))
        r = (lo + (hi - lo) * rng.uniform(0.05, 0.95, n))[:, None]
        return p.pos + _ring(rng, u, v, n) * r, np.broadcast_to(unit(a1), (n, 3))
    if k == "cylinder":
        e = _ring(rng, unit(a0), unit(a2), n)
        y = rng.uniform(0.05, 0.95, n) * s[0]
        return p.pos + a1 * y[:, None] + e * s[1], e
    inv = p.inv
    origin = p.pos + (a1 * s[2] if k == "box" else 0.0)
    al, be = rng.uniform(0.05, 0.95, n) * s[0], rng.uniform(0.05, 0.95, n) * s[1]
    return origin + al[:, None] * inv[:, 0] + be[:, None] * inv[:, 2], np.broadcast_to(unit(a1), (n, 3))


# ---- chords ---------------------------------------------------------------------------------
@dataclass
class Family:
    name: str
    chords: np.ndarray       # float32 [n, 7]
    delta: np.ndarray | None  # the signed delta of a grazing / ending chord (hit side: < 0)
    target: int              # the object's index in scene.objects[] (-1: the hole)


def pack(o, d, seg):
    return np.concatenate([o, d, np.asarray(seg)[:, None]], axis=1).astype(np.float32)


def _finite_rows(*arrays):
    ok = np.ones(arrays[0].shape[0], dtype=bool)
    for a in arrays:
        ok &= np.all(np.isfinite(a.reshape(a.shape[0], -1)), axis=1)
    return ok


def graze_chords(f: Feature, rng, lam_lo, lam_hi, short=False):
    n = f.P0.shape[0]
    dl = deltas(rng, n)
    lam = log_uniform(rng, lam_lo, lam_hi, n)
    if f.n is None and short:
        # a chord far shorter than the surface's radius cannot graze it (its sag
        # lam^2 / 2 ext lies below a float of the position): it crosses the
        # surface at P0 instead, from outside, and ends at lambda (1 - delta)
        c = log_uniform(rng, 1e-3, 1.0, n)
        d = unit(-f.e * c[:, None] + perpendicular(rng, f.e) * np.sqrt(np.maximum(0.0, 1.0 - c * c))[:, None])
        return pack(f.P0 - d * lam[:, None], d, lam * (1.0 - dl)), dl
    if f.n is None:
        # tangent: the closest approach is P. A chord whose origin lies lam from
        # P starts outside only while the half chord ext sqrt(2 |delta|) is
        # shorter: |delta| <= (lam / ext)^2 / 4 keeps delta < 0 a hit
        cap = np.where(f.ext > 0, (lam / np.where(f.ext > 0, f.ext, 1.0)) ** 2 / 4.0, np.inf)
        dl = np.sign(dl) * np.minimum(np.abs(dl), cap)
        d = perpendicular(rng, f.e) if f.d is None else f.d
    else:
        # crosses the surface at P, coming from the side n points to and moving
        # outward along e in the surface (away from the primitive's other parts)
        c = log_uniform(rng, 1e-3, 1.0, n)
        t = perpendicular(rng, f.n)
        t = np.where(np.sum(t * f.e, axis=-1, keepdims=True) < 0, -t, t)
        d = unit(-f.n * c[:, None] + t * np.sqrt(np.maximum(0.0, 1.0 - c * c))[:, None])
    P = f.P0 + f.e * (dl * f.ext)[:, None]
    o = P - d * lam[:, None]
    if f.n is None:
        return pack(o, d, lam * rng.uniform(1.2, 2.0, n)), dl
    # a crossing chord ends within half an extent past the surface (a skewed
    # box's other faces lie beyond)
    return pack(o, d, lam + np.minimum(lam, f.ext) * rng.uniform(0.05, 0.5, n)), dl


def end_chords(p: Prim, rng, n):
    Q, nrm = inner_points(p, rng, n)
    half = n // 2
    # aimed at Q from the side the normal points to, ending at lambda (1 + delta): a hit for delta > 0
    c = rng.uniform(0.2, 1.0, n)
    d = unit(-nrm * c[:, None] + perpendicular(rng, nrm) * np.sqrt(1.0 - c * c)[:, None])
    lam = log_uniform(rng, 1e-3, 60.0, n)
    dl = deltas(rng, n)
    o = Q - d * lam[:, None]
    seg = lam * (1.0 + dl)
    # origins a few floats either side of the surface, directions at random
    k = rng.choice([-4.0, -2.0, -1.0, 1.0, 2.0, 4.0], n)
    eps = np.spacing(np.maximum(np.max(np.abs(Q), axis=-1), 1e-30).astype(np.float32)).astype(np.float64)
    o2 = Q + nrm * (k * eps)[:, None]
    d2 = random_units(rng, n)
    toward = np.sum(d2 * nrm, axis=-1) * k < 0
    o[half:], d[half:], seg[half:] = o2[half:], d2[half:], log_uniform(rng, 1e-3, 60.0, n)[half:]
    dl[half:] = np.where(toward, -1.0, 1.0)[half:] * np.abs(k * eps)[half:]
    dl[:half] = -dl[:half]  # the hit side negative, as the grazing families'
    return pack(o, d, seg), dl


def parallel_chords(p: Prim, rng, n):
    Q, nrm = inner_points(p, rng, n)
    if p.kind == "cylinder":
        th = log_uniform(rng, 1e-7, np.pi / 2, n)
        ax = unit(p.axes[1]) * rng.choice([-1.0, 1.0], n)[:, None]
        side = unit(-nrm + perpendicular(rng, np.broadcast_to(unit(p.axes[1]), (n, 3))) * 0.5)
        side = unit(side - ax * np.sum(side * ax, axis=-1, keepdims=True))
        d = unit(ax * np.cos(th)[:, None] + side * np.sin(th)[:, None])
    else:
        c = log_uniform(rng, 1e-8, 1.0, n)
        d = unit(-nrm * c[:, None] + perpendicular(rng, nrm) * np.sqrt(np.maximum(0.0, 1.0 - c * c))[:, None])
    lam = log_uniform(rng, 1e-2, 60.0, n)
    return pack(Q - d * lam[:, None], d, lam * rng.uniform(1.1, 2.0, n)), None


def control_chords(rng, n, bc, br, pl1):
    """Chords whose binary64 distance from bc is at least 2 br + 0.1 (|o|_1 +
    seg + 1 + |pos|_1), measured on the float32 values the device gets."""
    out = []
    need = n
    for _ in range(64):
        m = 4 * n
        o = bc + random_units(rng, m) * (log_uniform(rng, 1.0, 1e3, m) * (1.0 + br) + 0.2 * (pl1 + l1(bc)))[:, None]
        d = random_units(rng, m)
        seg = log_uniform(rng, 1e-3, 60.0, m)
        ch = pack(o, d, seg)
        keep = control_margin(ch, bc, br, pl1) >= 0.0
        out.append(ch[keep][:need])
        need -= out[-1].shape[0]
        if need <= 0:
            break
    assert need <= 0, "control family: rejection sampling fell short"
    return np.concatenate(out)[:n]


def control_margin(ch, bc, br, pl1):
    """Binary64: (segment's distance from bc) - (2 br + 0.1 (|o|_1 + seg + 1 + |pos|_1))."""
    c = ch.astype(np.float64)
    o, d, seg = c[:, :3], c[:, 3:6], c[:, 6]
    dist = dist_point_segment(np.asarray(bc, dtype=np.float64), o, o + d * seg[:, None])
    return dist - (2.0 * br + 0.1 * (l1(o) + seg + 1.0 + pl1))


def bound_chords(p: Prim, rng, n, bc, lam_range=(1e-2, 1e4), d_range=(1e-9, 1e-1), outward=False):
    """Chords through P = P0 + e D perpendicular to P - bc, for the feature
    points P0 farthest from the bounding centre bc, D = +-(1e-9 .. 1e-1) S
    (outward: D > 0 only), origins lam_range away."""
    # (the features whose points lie on the primitive: a tube's and an edge's also run past its ends)
    fs = [f for f in features(p, rng, n) if f.name in ("sphere", "rim", "outer", "corner")]
    if not fs:
        return None
    far = max(float(np.max(np.linalg.norm(f.P0 - bc, axis=-1))) for f in fs)
    P0, e = [], []
    for f in fs:
        keep = np.linalg.norm(f.P0 - bc, axis=-1) >= 0.999 * far
        P0.append(f.P0[keep])
        e.append((f.n if f.name == "rim" else f.e)[keep])  # a cylinder's end circle: radially
    P0, e = np.concatenate(P0)[:n], np.concatenate(e)[:n]
    m = P0.shape[0]
    lam = log_uniform(rng, *lam_range, m)
    seg = lam * rng.uniform(1.2, 2.0, m)
    S = l1(P0) + lam + seg + 1.0
    sign = np.ones(m) if outward else rng.choice([-1.0, 1.0], m)
    P = P0 + e * (sign * log_uniform(rng, *d_range, m) * S)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        d = perpendicular(rng, np.nan_to_num(unit(P - bc)) + 1e-300)
    return pack(P - d * lam[:, None], d, seg)


def families(p: Prim, rng, n):
    """The families of one finite primitive (no controls: those need the packed bound)."""
    out = []
    for f in features(p, rng, n):
        ch, dl = graze_chords(f, rng, 1e-2, 60.0)
        out.append(Family(f"graze_{f.name}", ch, dl, p.index))
    fs = features(p, rng, n)
    if fs:
        per = max(1, n // len(fs))
        for name, lo, hi in (("far", 60.0, 1e4), ("short", 1e-6, 1e-2)):
            short = name == "short"
            parts = [graze_chords(Feature(f.name, f.P0[:per], f.e[:per], f.ext[:per], None if f.n is None else f.n[:per],
                                          None if f.d is None else f.d[:per]), rng, lo, hi, short) for f in fs]
            out.append(Family(name, np.concatenate([c for c, _ in parts]), np.concatenate([d for _, d in parts]),
                              p.index))
    ch, dl = end_chords(p, rng, n)
    out.append(Family("end", ch, dl, p.index))
    if p.kind != "sphere":
        ch, _ = parallel_chords(p, rng, n)
        out.append(Family("parallel", ch, None, p.index))
    for f in out:
        ok = _finite_rows(f.chords)
        f.chords = f.chords[ok]
        if f.delta is not None:
            f.delta = f.delta[ok]
    return [f for f in out if f.chords.shape[0]]


# ---- anchors for the clearance probes ----------------------------------------------------------
def anchors(p: Prim, rng, n):
    """Points at binary64 distance 1e-6 .. 1e2 from the primitive's surface on
    either side of it: off its inner points along the normal (inside a tube, a
    box or the shell for the negative side), off its rims and edges in the
    surface (an annulus's hole, the plane beyond a rim), and at random."""
    Q, nrm = inner_points(p, rng, n)
    D = log_uniform(rng, 1e-6, 1e2, n) * rng.choice([-1.0, 1.0], n, p=[0.35, 0.65])
    parts = [Q + nrm * D[:, None]]
    for f in features(p, rng, n // 2):
        m = f.P0.shape[0]
        parts.append(f.P0 + f.e * (log_uniform(rng, 1e-6, 1e2, m) * rng.choice([-1.0, 1.0], m, p=[0.3, 0.7]))[:, None])
    reach = 2.0 * max([abs(v) for v in p.size] + [0.0])  # beyond the primitive's bounding sphere
    m = 3 * n // 2
    parts.append(p.pos + random_units(rng, m) * (reach + log_uniform(rng, 1e-2, 1e2, m))[:, None])
    a = np.concatenate(parts).astype(np.float32)
    return a[_finite_rows(a)]


def guard_value(A, bc, br):
    """|A - bc| - br - 2e-3 (1 + |bc|_1 + br) - 3.6e-3 |A| in binary64: the
    sphere term of clearance_obj less rb's own margin and 1.8 mu a, mu <=
    SR_MU_QUADRATIC."""
    A = A.astype(np.float64)
    return (np.linalg.norm(A - bc, axis=-1) - br - 2e-3 * (1.0 + l1(np.asarray(bc, dtype=np.float64)) + br)
            - 3.6e-3 * np.linalg.norm(A, axis=-1))


# ---- the packed image (host only) ------------------------------------------------------------
# Word offsets into the packed image (csrc/device_scene.h sr_dev_scene, sr_dev_obj, sr_dev_slot), in the
# order lib/libsr_bnd.so's sr_debug_probe_layout reports them (tests/test_bound_cases.py compares the two):
# num_objects, tr_visible, tr_num_segments, tr_num_groups, tr_radius, num_budget, budget_idx, slots,
# words per slot, num_step, step_idx, flat_miss_r2, objs, words per object, obj.kind, obj.bc, obj.br
# (rb, mu, mp, pl1 follow it), slot.rb (mp, br, mu follow it), slot.br, slot.bc, SR_MAX_OBJECTS
LAYOUT = (0, 2, 3, 5, 6, 18, 19, 41, 28, 629, 630, 651, 676, 128, 3, 4, 7, 2, 4, 8, 21)


def image_views(pkg, img):
    """Reads bc, br, kind ... of every object and slot out of a packed scene image."""
    (o_nobj, o_vis, o_nseg, o_ngrp, o_rad, o_nb, o_bidx, o_slots, slot_w, o_ns, o_sidx, o_flat, o_objs, obj_w,
     k_kind, k_bc, k_br, s_rb, s_br, s_bc, max_obj) = LAYOUT
    i32 = img.view(np.int32)
    f32 = img.view(np.float32)
    assert img.nbytes == pkg.abi._precompute_sizes()[0]
    num_budget, num_step = int(i32[o_nb]), int(i32[o_ns])
    out = {"num_objects": int(i32[o_nobj]), "tr_visible": int(i32[o_vis]), "tr_num_segments": int(i32[o_nseg]),
           "tr_num_groups": int(i32[o_ngrp]), "tr_radius": float(f32[o_rad]), "num_budget": num_budget,
           "budget_idx": i32[o_bidx:o_bidx + max_obj][:num_budget].copy(), "num_step": num_step,
           "step_idx": i32[o_sidx:o_sidx + max_obj][:num_step].copy(), "flat_miss_r2": float(f32[o_flat]),
           "objs": [], "slots": []}
    for k in range(out["num_objects"]):
        b = o_objs + obj_w * k
        out["objs"].append({"type": int(i32[b]), "kind": int(i32[b + k_kind]),
                            "bc": f32[b + k_bc:b + k_bc + 3].astype(np.float64), "br": float(f32[b + k_br]),
                            "rb": float(f32[b + k_br + 1]), "mu": float(f32[b + k_br + 2]),
                            "mp": float(f32[b + k_br + 3]), "pl1": float(f32[b + k_br + 4])})
    for j in range(num_budget):
        b = o_slots + slot_w * j
        out["slots"].append({"type": int(i32[b]), "rb": float(f32[b + s_rb]), "mp": float(f32[b + s_rb + 1]),
                             "br": float(f32[b + s_br]), "mu": float(f32[b + s_br + 1]),
                             "bc": f32[b + s_bc:b + s_bc + 3].astype(np.float64)})
    return out


KIND_EXACT, KIND_BUDGET, KIND_CHORD = 0, 1, 2


# ---- scenes ---------------------------------------------------------------------------------
def skewed(axes, k=0.35):
    """a0 += k a1, a2 += 0.5 k a0: neither orthogonal nor unit."""
    a = np.array(axes, dtype=np.float64).reshape(3, 3)
    a[0] = a[0] + k * a[1]
    a[2] = 1.2 * a[2] + 0.5 * k * a[0]
    return tuple(float(np.float32(v)) for v in a.reshape(-1))


UP1 = X.axes_up((0.3, 1.0, 0.2))
UP2 = X.axes_up((-0.5, 0.4, 1.0))
ALONE = [
    # (name, spec): positions up to +-50, sizes 1e-3 .. 1e2
    ("sphere_small", {"type": "sphere", "pos": (3.0, 1.0, 5.0), "radius": 1e-3}),
    ("sphere_mid_far", {"type": "sphere", "pos": (-50.0, 20.0, 35.0), "radius": 2.5}),
    ("sphere_huge", {"type": "sphere", "pos": (10.0, -20.0, 30.0), "radius": 100.0}),
    ("plane_tilted", {"type": "plane", "pos": (0.0, -4.0, 0.0), "axes": UP1}),
    ("plane_far", {"type": "plane", "pos": (50.0, -50.0, 20.0), "axes": UP2}),
    ("disk_small", {"type": "disk", "pos": (1.0, -1.0, 6.0), "axes": X.TILT, "radius": 1e-3}),
    ("disk_mid_far", {"type": "disk", "pos": (40.0, 50.0, -30.0), "axes": UP1, "radius": 4.0}),
    ("disk_huge", {"type": "disk", "pos": (0.0, -3.0, 0.0), "axes": UP2, "radius": 100.0}),
    ("annulus_hole", {"type": "annulus", "pos": (0.0, 0.0, 0.0), "axes": X.DISK_AXES, "inner": 2.5, "outer": 5.0}),
    ("annulus_thin_far", {"type": "annulus", "pos": (-45.0, 10.0, 50.0), "axes": UP2, "inner": 3.0, "outer": 3.001}),
    ("annulus_huge", {"type": "annulus", "pos": (5.0, 5.0, -5.0), "axes": UP1, "inner": 1e-3, "outer": 100.0}),
    ("cylinder_thin", {"type": "cylinder", "pos": (-6.0, -8.0, 8.0), "axes": X.axes_up((0.6, 1.0, 0.0)),
                       "height": 20.0, "radius": 1e-3}),
    ("cylinder_thick_far", {"type": "cylinder", "pos": (50.0, -30.0, -40.0), "axes": UP1, "height": 3.0,
                            "radius": 8.0}),
    ("cylinder_huge", {"type": "cylinder", "pos": (0.0, -50.0, 0.0), "axes": UP2, "height": 100.0, "radius": 30.0}),
    ("cylinder_flat", {"type": "cylinder", "pos": (4.0, 2.0, -7.0), "axes": UP1, "height": 1e-3, "radius": 2.0}),
    ("cylinder_coin", {"type": "cylinder", "pos": (4.0, 2.0, -7.0), "axes": UP1, "height": 4e-3, "radius": 1e-2}),
    ("rectangle_small", {"type": "rectangle", "pos": (-2.0, -2.0, 7.0), "axes": X.TILT, "width": 1e-3, "height": 2e-3}),
    ("rectangle_mid_far", {"type": "rectangle", "pos": (-50.0, 45.0, 30.0), "axes": UP1, "width": 4.0, "height": 0.1}),
    ("rectangle_huge", {"type": "rectangle", "pos": (-40.0, 5.0, -50.0), "axes": UP2, "width": 100.0, "height": 80.0}),
    ("rectangle_skewed", {"type": "rectangle", "pos": (-2.0, -2.0, 7.0), "axes": skewed(X.TILT), "width": 4.0,
                          "height": 3.0}),
    ("rectangle_skewed_far", {"type": "rectangle", "pos": (30.0, -50.0, 12.0), "axes": skewed(UP2, 0.8), "width": 0.5,
                              "height": 20.0}),
    ("box_small", {"type": "box", "pos": (2.0, -1.0, 5.0), "axes": X.axes_up((0.2, 1.0, 0.3)), "width": 1e-3,
                   "depth": 2e-3, "height": 3e-3}),
    ("box_mid_far", {"type": "box", "pos": (45.0, -50.0, 50.0), "axes": UP1, "width": 2.0, "depth": 3.0, "height": 1.0}),
    ("box_huge", {"type": "box", "pos": (-40.0, -40.0, -40.0), "width": 80.0, "depth": 100.0, "height": 60.0}),
    ("box_skewed", {"type": "box", "pos": (2.0, -1.0, 5.0), "axes": skewed(X.axes_up((0.2, 1.0, 0.3)), 0.15), "width": 2.0,
                    "depth": 3.0, "height": 1.5}),
]
EXTREME_GROUPS = ("signed", "zero", "nonfinite")


@dataclass
class SceneCase:
    name: str
    scene: object
    test_ray: object | None  # None: the context's default (not visible)
    n: int                   # chords per family and object
    alone: bool              # one primitive: the CPU test's hit-rate check applies


def scene_cases(pkg):
    sc = pkg.scenes
    out = [SceneCase(f"alone/{name}", X.scene_alone(pkg, spec), None, N, True) for name, spec in ALONE]
    out.append(SceneCase("hole", sc.scene_black_hole_only(), None, N, True))
    out.append(SceneCase("stress", sc.scene_stress(), None, N_EMBEDDED, False))
    out.append(SceneCase("default", sc.scene_default(False), None, N_EMBEDDED, False))
    out += [SceneCase(f"random-{seed}", sc.scene_random(seed), None, N_EMBEDDED, False) for seed in (3, 5)]
    for c in X.CASES:
        if c.group in EXTREME_GROUPS:
            host = "default" if c.group == "nonfinite" else "alone"
            out.append(SceneCase(f"extreme/{c.name}", X.build(pkg, c, host), None, N_EMBEDDED, False))
    for name, tr in HP.test_rays(pkg):
        if name in ("default", "press-r", "overlay-1000"):
            out.append(SceneCase(f"test-ray/{name}", sc.scene_default(False), tr, N_EMBEDDED, False))
    assert len({c.name for c in out}) == len(out)
    return out


def seed_of(name):
    return zlib.crc32(name.encode()) ^ 0x5EED


def test_ray_points(tr):
    """The visible polyline's points [m, 3] in binary64 (empty when hidden)."""
    if tr is None or not tr.visible:
        return np.zeros((0, 3))
    m = min(int(tr.num_curved_points), len(tr.curved_points))
    return np.array([[tr.curved_points[i][k] for k in range(3)] for i in range(m)], dtype=np.float64)


def test_ray_families(tr, rng, n):
    """Chords grazing the polyline's tube: tangent at radius x (1 + delta) to a
    segment's axis, and across the tube."""
    pts = test_ray_points(tr)
    if pts.shape[0] < 2:
        return []
    i = rng.integers(0, pts.shape[0] - 1, n)
    a, b = pts[i], pts[i + 1]
    ax = b - a
    ok = np.linalg.norm(ax, axis=-1) > 0
    a, b, ax = a[ok], b[ok], unit(ax[ok])
    m = a.shape[0]
    e = perpendicular(rng, ax)
    r = float(tr.radius)
    f = Feature("tube", a + (b - a) * rng.uniform(0.0, 1.0, m)[:, None] + e * r, e, np.full(m, r), None)
    ch, dl = graze_chords(f, rng, 1e-2, 30.0)
    return [Family("graze_test_ray", ch, dl, -3)]


def chord_set(pkg, case: SceneCase):
    """[Family] of a scene: every finite object's families, the hole's, the
    test ray's, controls of the bounded orthonormal objects, and random chords."""
    rng = np.random.default_rng(seed_of(case.name))
    out = []
    prims = prims_of(case.scene)
    for p in prims:
        if p.finite:
            out += families(p, rng, case.n)
    hole = [f for f in families(HOLE, rng, case.n if case.name == "hole" else N_EMBEDDED)]
    out += hole
    out += test_ray_families(case.test_ray, rng, 4 * case.n)
    rc, img, _ = pkg.abi.debug_pack_scene(case.scene, case.test_ray)
    assert rc == 0, (case.name, rc)
    view = image_views(pkg, img)
    for p in prims:
        ob = view["objs"][p.index]
        if p.finite and p.orthonormal and ob["kind"] != KIND_EXACT and np.isfinite(ob["br"]):
            out.append(Family("control", control_chords(rng, case.n, ob["bc"], ob["br"], ob["pl1"]), None, p.index))
        if p.finite and ob["kind"] != KIND_EXACT and np.isfinite(ob["br"]):
            ch = bound_chords(p, rng, 2 * case.n, ob["bc"])
            if ch is not None and _finite_rows(ch).any():
                out.append(Family("bound", ch[_finite_rows(ch)], None, p.index))
        if case.alone and p.kind == "cylinder" and p.finite and abs(p.size[1]) <= 1.0 and np.isfinite(ob["br"]):
            # a small cylinder seen from 1e2 .. 1e4 away, the chord 1e-5 .. 3e-3 S outside its end circle:
            # the lateral quadratic accepts some of these by rounding (|X|^2 / r is large), and the chord
            # passes farther from bc than br + mu S: what lat_margin is in may_hit for
            ch = bound_chords(p, rng, N_BOUND_FAR, ob["bc"], (1e2, 1e4), (1e-5, 3e-3), True)
            out.append(Family("bound_far", ch[_finite_rows(ch)], None, p.index))
    m = case.n
    o = random_units(rng, m) * log_uniform(rng, 1e-2, 1e4, m)[:, None]
    out.append(Family("random", pack(o, random_units(rng, m), log_uniform(rng, 1e-6, 60.0, m)), None, -100))
    return out
