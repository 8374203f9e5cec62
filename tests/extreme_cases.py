"""Scenes no generator of scenes.py draws (a helper, not a test module).

CASES is a table of named cases for tests/test_scene_extremes_cases.py (the
oracle alone: is the case what it says?) and tests/test_gpu_scene_extremes.py
(the kernel against the oracle, culling on against off). A case is one
primitive (a spec, below), a camera, the u_f of its launches, its step
schedules and the share of a 64x40 frame the primitive must change:

    Case.group    signed | zero | horizon | enclosing | thin | far | frames | nonfinite
    Case.spec     {"type": sphere | plane | disk | annulus | cylinder |
                   rectangle | box, "pos": (x, y, z), "axes": nine floats
                   (column-major, default identity), sizes by type}
    Case.camera   (pos, target, fov)
    Case.u_f
    Case.beyond_uf  the primitive lies wholly beyond r = 1 / u_f (far group)
    Case.visible  the minimum share of pixels the primitive changes
                  (MIN_SHARE; 0: no minimum, see the group's comment)

Hosts: "alone" (the primitive, one untextured opaque double-sided material,
one light), "embedded" (the same primitive in place of the first object of
its type in scenes.scene_random(11, n_objects=21, translucent=False): the
large kernel instantiation, every budget slot used) and "default" (added to
scenes.scene_default(False): the zero-size and non-finite groups, whose
primitive may leave the frame as it was; the zero-size group runs alone too).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

W, H = 64, 40  # 4 x 3 tiles of 16 x 16, partial waves on two edges

# (max_steps, max_revolutions): step angles 0.031 and the app's 0.126
SCHEDULES = {"400x2": (400, 2), "100x2": (100, 2)}
FAR_SCHEDULES = {"600x2": (600, 2)}

MIN_SHARE = {"signed": 0.02, "horizon": 0.02, "enclosing": 0.02, "far": 0.02, "frames": 0.02, "thin": 0.01,
             "zero": 0.0, "nonfinite": 0.0}

IDENT = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
NAN, INF = float("nan"), float("inf")


@dataclass
class Case:
    name: str
    group: str
    spec: dict
    camera: tuple
    u_f: float = 0.01
    visible: float | None = None  # None: the group's MIN_SHARE
    schedules: dict = field(default_factory=lambda: SCHEDULES)
    beyond_uf: bool = False  # the primitive lies wholly beyond r = 1 / u_f

    @property
    def min_share(self) -> float:
        return MIN_SHARE[self.group] if self.visible is None else self.visible

    @property
    def hosts(self) -> tuple:
        if self.group == "nonfinite":
            return ("default",)
        return ("alone", "default") if self.group == "zero" else ("alone", "embedded")


def axes_up(up, ref=(1.0, 0.0, 0.0)):
    """Orthonormal column-major axes with axes[1] = normalize(up)."""
    u = np.asarray(up, dtype=np.float64)
    u = u / np.linalg.norm(u)
    a = np.asarray(ref, dtype=np.float64)
    a = a - u * np.dot(a, u)
    a = a / np.linalg.norm(a)
    c = np.cross(a, u)
    return tuple(float(np.float32(v)) for v in (*a, *u, *c))


def scaled_normal(axes, k):
    a = list(axes)
    for i in range(3, 6):
        a[i] = float(np.float32(a[i] * k))
    return tuple(a)


def sheared(axes, k=0.3):
    """c1 += k c0"""
    a = list(axes)
    for i in range(3):
        a[3 + i] = float(np.float32(a[3 + i] + k * a[i]))
    return tuple(a)


# ---- scene building ------------------------------------------------------------
TYPE_OF = {"sphere": 0, "plane": 1, "disk": 2, "annulus": 3, "cylinder": 4, "rectangle": 5, "box": 6}
ARRAY_OF = {"sphere": "spheres", "plane": "planes", "disk": "disks", "annulus": "hollow_disks",
            "cylinder": "cylinders", "rectangle": "rectangles", "box": "boxes"}


def _set_transform(t, spec):
    for i in range(3):
        t.pos[i] = spec["pos"][i]
    ax = spec.get("axes", IDENT)
    for i in range(9):
        t.axes[i] = ax[i]


def _set_plane(p, spec):
    _set_transform(p.transform, spec)
    p.texture_offset[0], p.texture_offset[1] = spec.get("texture_offset", (0.0, 0.0))
    p.repeat_texture = int(spec.get("repeat_texture", 0))
    p.texture_size[0], p.texture_size[1] = spec.get("texture_size", (1.0, 1.0))


def write_primitive(scene, k, spec):
    """The spec into slot k of its type's array."""
    kind = spec["type"]
    rec = getattr(scene, ARRAY_OF[kind])[k]
    if kind == "sphere":
        _set_transform(rec.transform, spec)
        rec.radius = spec["radius"]
    elif kind == "plane":
        _set_plane(rec, spec)
    elif kind == "disk":
        _set_plane(rec.plane, spec)
        rec.radius = spec["radius"]
    elif kind == "annulus":
        _set_plane(rec.plane, spec)
        rec.inner_radius, rec.outer_radius = spec["inner"], spec["outer"]
    elif kind == "cylinder":
        _set_transform(rec.transform, spec)
        rec.height, rec.radius = spec["height"], spec["radius"]
    elif kind == "rectangle":
        _set_plane(rec.plane, spec)
        rec.width, rec.height = spec["width"], spec["height"]
    elif kind == "box":
        _set_transform(rec.transform, spec)
        rec.width, rec.depth, rec.height = spec["width"], spec["depth"], spec["height"]
    else:
        raise ValueError(kind)


def plain_material(m, color=(0.9, 0.5, 0.2, 1.0)):
    """Untextured, opaque, double-sided."""
    for k in range(4):
        m.color[k] = color[k]
    m.ambient, m.diffuse, m.specular, m.shininess = 0.3, 0.7, 0.3, 16.0
    m.texture_index, m.normal_map_index = -1, -1
    m.invert_uv_x = m.invert_uv_y = m.swap_uvs = m.flip_normals = 0
    m.double_sided_normals = 1


def one_light(scene):
    scene.num_lights = 1
    L = scene.lights[0]
    for i in range(3):
        L.transform.pos[i] = (5.0, 12.0, 14.0)[i]
        L.color[i] = 1.0
    for i in range(9):
        L.transform.axes[i] = IDENT[i]
    L.intensity, L.attenuation_constant, L.attenuation_linear, L.attenuation_quadratic = 6.0, 1.0, 0.05, 0.01


def empty_scene(pkg):
    s = pkg.abi.Scene()
    pkg.abi.load().sr_scene_clear(C.byref(s))
    plain_material(s.materials[0])
    one_light(s)
    return s


def append_primitive(scene, spec, material_index=0):
    """Adds the primitive as the scene's last object, in the first free slot of its type."""
    t = TYPE_OF[spec["type"]]
    k = sum(1 for i in range(scene.num_objects) if scene.objects[i].type == t)
    assert k < 3 and scene.num_objects < len(scene.objects)
    write_primitive(scene, k, spec)
    o = scene.objects[scene.num_objects]
    o.type, o.index, o.material_index = t, k, material_index
    scene.num_objects += 1
    return scene


def scene_alone(pkg, spec):
    return append_primitive(empty_scene(pkg), spec)


def scene_embedded(pkg, spec):
    """The primitive in place of the first object of its type in the
    21-object scene (its material made the plain one)."""
    s = pkg.scenes.scene_random(11, n_objects=21, translucent=False)
    t = TYPE_OF[spec["type"]]
    n = next(i for i in range(s.num_objects) if s.objects[i].type == t)
    write_primitive(s, s.objects[n].index, spec)
    plain_material(s.materials[s.objects[n].material_index])
    return s


def scene_default_plus(pkg, spec):
    s = pkg.scenes.scene_default(False)
    # a material of its own (the default scene's are taken as they are)
    mi = pkg.abi.MAX_MATERIALS - 1
    plain_material(s.materials[mi])
    return append_primitive(s, spec, mi)


def build(pkg, case, host):
    return {"alone": scene_alone, "embedded": scene_embedded, "default": scene_default_plus}[host](pkg, case.spec)


def without_primitive(pkg, case, host):
    """The host scene with the case's primitive removed."""
    s = build(pkg, case, host)
    if host == "embedded":
        t = TYPE_OF[case.spec["type"]]
        n = next(i for i in range(s.num_objects) if s.objects[i].type == t)
        for i in range(n, s.num_objects - 1):
            src, dst = s.objects[i + 1], s.objects[i]
            dst.type, dst.index, dst.material_index = src.type, src.index, src.material_index
    s.num_objects -= 1
    return s


def camera_of(pkg, case):
    pos, target, fov = case.camera
    fwd = tuple(float(t) - float(p) for p, t in zip(pos, target))
    return pkg.scenes.camera_look(pos, fwd, fov=fov)


def params_of(pkg, case, schedule):
    steps, revs = case.schedules[schedule]
    return pkg.abi.default_params(max_steps=steps, max_revolutions=revs, u_f=case.u_f, percent_black=-1.0)


def cells():
    """(case, host, schedule) of the GPU matrix."""
    return [(c, h, s) for c in CASES for h in c.hosts for s in c.schedules]


# ---- the table -----------------------------------------------------------------
CAM0 = ((0.0, 2.0, 15.0), (0.0, 0.0, 0.0), 90.0)  # the app's camera position, looking at the hole
DISK_AXES = axes_up((0.05, 1.0, 0.1))              # the accretion disk's tilt
TILT = axes_up((0.2, 0.5, 1.0))                    # a planar primitive facing CAM0


def _c(name, group, spec, camera=CAM0, **kw):
    return Case(name, group, spec, camera, **kw)


CASES = [
    # -- signed sizes: every exact test squares a radius, so a negative one
    # renders as its magnitude; a negative extent or height is an empty range
    # (is_in_range(x, 0, negative)) and accepts nothing: no minimum there.
    _c("disk_radius_neg4", "signed", {"type": "disk", "pos": (1.0, -1.0, 6.0), "axes": TILT, "radius": -4.0}),
    _c("annulus_neg_neg", "signed", {"type": "annulus", "pos": (0.0, 0.0, 0.0), "axes": DISK_AXES, "inner": -2.5,
                                     "outer": -5.0}),
    _c("annulus_pos_neg", "signed", {"type": "annulus", "pos": (0.0, 0.0, 0.0), "axes": DISK_AXES, "inner": 2.5,
                                     "outer": -5.0}),
    _c("annulus_neg_pos", "signed", {"type": "annulus", "pos": (0.0, 0.0, 0.0), "axes": DISK_AXES, "inner": -2.5,
                                     "outer": 5.0}),
    _c("sphere_radius_neg", "signed", {"type": "sphere", "pos": (3.0, 1.0, 5.0), "radius": -1.5}),
    _c("cylinder_radius_neg", "signed", {"type": "cylinder", "pos": (-3.0, -1.0, 6.0), "axes": axes_up((0.3, 1.0, 0.1)),
                                         "height": 4.0, "radius": -1.0}),
    _c("box_width_neg", "signed", {"type": "box", "pos": (2.0, -1.0, 5.0), "axes": axes_up((0.2, 1.0, 0.3)),
                                   "width": -2.0, "depth": 3.0, "height": 3.0}),
    _c("rectangle_width_neg", "signed", {"type": "rectangle", "pos": (-2.0, -2.0, 7.0), "axes": TILT, "width": -4.0,
                                         "height": 4.0}, visible=0.0),
    _c("cylinder_height_neg", "signed", {"type": "cylinder", "pos": (-3.0, 1.0, 6.0), "height": -2.0, "radius": 1.0},
       visible=0.0),
    # -- zero sizes: sets of measure zero (a box of zero height still shows its two coincident faces)
    _c("disk_radius_0", "zero", {"type": "disk", "pos": (1.0, -1.0, 6.0), "axes": TILT, "radius": 0.0}),
    _c("annulus_inner_eq_outer", "zero", {"type": "annulus", "pos": (0.0, 0.0, 0.0), "axes": DISK_AXES, "inner": 6.5,
                                          "outer": 6.5}),
    _c("annulus_inner_gt_outer", "zero", {"type": "annulus", "pos": (0.0, 0.0, 0.0), "axes": DISK_AXES, "inner": 7.5,
                                          "outer": 5.5}),
    _c("sphere_radius_0", "zero", {"type": "sphere", "pos": (3.0, 1.0, 5.0), "radius": 0.0}),
    _c("cylinder_radius_0", "zero", {"type": "cylinder", "pos": (-3.0, -1.0, 6.0), "height": 4.0, "radius": 0.0}),
    _c("cylinder_height_0", "zero", {"type": "cylinder", "pos": (-3.0, 1.0, 6.0), "height": 0.0, "radius": 1.0}),
    _c("rectangle_width_0", "zero", {"type": "rectangle", "pos": (-2.0, -2.0, 7.0), "axes": TILT, "width": 0.0,
                                     "height": 4.0}),
    _c("box_height_0", "zero", {"type": "box", "pos": (2.0, 3.0, 5.0), "axes": axes_up((0.2, 1.0, 0.6)),
                                "width": 3.0, "depth": 3.0, "height": 0.0}),
    # -- at and inside the horizon (the hole's windows, crossings ending as ST_BH)
    _c("annulus_0p5_3_from_above", "horizon", {"type": "annulus", "pos": (0.0, 0.0, 0.0), "inner": 0.5, "outer": 3.0},
       ((0.0, 8.0, 3.0), (0.0, 0.0, 0.0), 60.0)),
    _c("annulus_1p02_1p6_from_above", "horizon", {"type": "annulus", "pos": (0.0, 0.0, 0.0), "inner": 1.02,
                                                  "outer": 1.6}, ((0.0, 6.0, 1.5), (0.0, 0.0, 0.0), 50.0)),
    _c("sphere_at_r1p3", "horizon", {"type": "sphere", "pos": (0.0, 0.5, 1.2), "radius": 0.35},
       ((0.0, 1.5, 5.0), (0.0, 0.5, 1.2), 30.0)),
    _c("rectangle_through_origin", "horizon", {"type": "rectangle", "pos": (-3.0, 0.0, -3.0), "width": 6.0,
                                               "height": 6.0}, ((0.0, 6.0, 8.0), (0.0, 0.0, 0.0), 60.0)),
    _c("cylinder_through_origin_r0p5", "horizon", {"type": "cylinder", "pos": (0.0, -4.0, 0.0), "height": 8.0,
                                                   "radius": 0.5}, ((0.0, 3.0, 10.0), (0.0, 0.0, 0.0), 60.0)),
    _c("cylinder_through_origin_r1p05", "horizon", {"type": "cylinder", "pos": (0.0, -4.0, 0.0), "height": 8.0,
                                                    "radius": 1.05}, ((0.0, 3.0, 10.0), (0.0, 0.0, 0.0), 60.0)),
    _c("box_holding_the_hole", "horizon", {"type": "box", "pos": (-1.2, -1.2, -1.2), "width": 2.4, "depth": 2.4,
                                           "height": 2.4}, ((3.0, 2.0, 6.0), (0.0, 0.0, 0.0), 50.0)),
    # -- enclosing and huge
    _c("sphere_r40_camera_inside", "enclosing", {"type": "sphere", "pos": (0.0, 0.0, 0.0), "radius": 40.0}),
    _c("cylinder_r30_h100_around", "enclosing", {"type": "cylinder", "pos": (0.0, -50.0, 0.0), "height": 100.0,
                                                 "radius": 30.0}),
    _c("box_80_around", "enclosing", {"type": "box", "pos": (-40.0, -40.0, -40.0), "width": 80.0, "depth": 80.0,
                                      "height": 80.0}),
    _c("disk_r300", "enclosing", {"type": "disk", "pos": (0.0, -3.0, 0.0), "radius": 300.0}),
    _c("plane_through_camera", "enclosing", {"type": "plane", "pos": (0.0, 2.0, 15.0), "axes": axes_up((0.2, 1.0, 0.1))}),
    _c("camera_inside_tube", "enclosing", {"type": "cylinder", "pos": (0.0, 2.0, 16.0), "axes": axes_up((0.0, 0.0, -1.0)),
                                           "height": 12.0, "radius": 1.0},
       ((0.0, 2.0, 15.0), (0.0, 2.0, 0.0), 90.0)),
    # -- thin
    _c("cylinder_r0p01_h20", "thin", {"type": "cylinder", "pos": (-6.0, -8.0, 8.0), "axes": axes_up((0.6, 1.0, 0.0)),
                                      "height": 20.0, "radius": 0.01}, ((0.0, 2.0, 15.0), (-0.5, 1.0, 8.0), 8.0)),
    _c("cylinder_r0p05_h20", "thin", {"type": "cylinder", "pos": (-6.0, -8.0, 8.0), "axes": axes_up((0.6, 1.0, 0.0)),
                                      "height": 20.0, "radius": 0.05}, ((0.0, 2.0, 15.0), (-0.5, 1.0, 8.0), 30.0)),
    _c("rectangle_0p1_by_20", "thin", {"type": "rectangle", "pos": (-8.0, -5.0, 7.0), "axes": axes_up((0.0, 0.2, 1.0)),
                                       "width": 20.0, "height": 0.1}, ((0.0, 2.0, 15.0), (0.0, -4.0, 7.0), 20.0)),
    _c("box_20_6_0p001", "thin", {"type": "box", "pos": (-10.0, -3.0, 4.0), "width": 20.0, "depth": 6.0,
                                  "height": 0.001}, ((0.0, 2.0, 15.0), (0.0, -3.0, 7.0), 60.0)),
    # -- far: beyond r = 1 / u_f, reached only through the reseed branch (the
    # cylinder at r = 90 lies inside it: its budget window's 32-unit cap)
    _c("sphere_r20_at_150_uf0p01", "far", {"type": "sphere", "pos": (60.0, 0.0, -137.5), "radius": 20.0},
       ((0.0, 2.0, 15.0), (60.0, 0.0, -137.5), 40.0), u_f=0.01, schedules=FAR_SCHEDULES, beyond_uf=True),
    _c("sphere_r20_at_150_uf0p05", "far", {"type": "sphere", "pos": (60.0, 0.0, -137.5), "radius": 20.0},
       ((0.0, 2.0, 15.0), (60.0, 0.0, -137.5), 40.0), u_f=0.05, schedules=FAR_SCHEDULES, beyond_uf=True),
    _c("rectangle_200_at_250", "far", {"type": "rectangle", "pos": (-100.0, 100.0, -250.0),
                                       "axes": axes_up((0.0, 0.0, 1.0)), "width": 200.0, "height": 200.0},
       ((0.0, 2.0, 15.0), (30.0, 20.0, -250.0), 60.0), u_f=0.01, schedules=FAR_SCHEDULES, beyond_uf=True),
    _c("cylinder_h60_r5_at_90", "far", {"type": "cylinder", "pos": (40.0, -30.0, -80.0), "height": 60.0,
                                        "radius": 5.0},
       ((0.0, 2.0, 15.0), (40.0, 0.0, -80.0), 50.0), u_f=0.01, schedules=FAR_SCHEDULES),
    _c("sphere_r8_at_30_uf0p05", "far", {"type": "sphere", "pos": (12.0, 3.0, -27.0), "radius": 8.0},
       ((0.0, 2.0, 15.0), (12.0, 3.0, -27.0), 50.0), u_f=0.05, schedules=FAR_SCHEDULES, beyond_uf=True),
    # -- frames only cylinders, rectangles and boxes were given: the normal
    # column scaled or sheared (disk-like primitives bounded without a unit
    # normal, planes tested on every chord), and a cylinder with an all-zero
    # frame (every local coordinate 0, the roots 0 / 0: it accepts nothing)
    *[_c(f"{kind}_{label}", "frames", {**spec, "axes": fn(spec["axes"])})
      for kind, spec in (
          ("disk", {"type": "disk", "pos": (1.0, -1.0, 6.0), "axes": TILT, "radius": 4.0}),
          ("annulus", {"type": "annulus", "pos": (0.0, 0.0, 0.0), "axes": DISK_AXES, "inner": 2.5, "outer": 5.0}),
          ("plane", {"type": "plane", "pos": (0.0, -4.0, 0.0), "axes": axes_up((0.1, 1.0, 0.0))}),
          ("sphere", {"type": "sphere", "pos": (3.0, 1.0, 5.0), "axes": axes_up((0.3, 1.0, 0.2)), "radius": 1.5}))
      for label, fn in (("normal_x1p3", lambda a: scaled_normal(a, 1.3)), ("normal_x0p7", lambda a: scaled_normal(a, 0.7)),
                        ("sheared", sheared))],
    _c("cylinder_zero_frame", "frames", {"type": "cylinder", "pos": (-3.0, -1.0, 6.0), "axes": (0.0,) * 9,
                                         "height": 4.0, "radius": 1.0}, visible=0.0),
    # -- non-finite: tested on every chord (SR_KIND_EXACT), every compare false
    _c("sphere_radius_nan", "nonfinite", {"type": "sphere", "pos": (3.0, 1.0, 5.0), "radius": NAN}),
    _c("cylinder_radius_nan", "nonfinite", {"type": "cylinder", "pos": (-3.0, -1.0, 6.0), "height": 4.0,
                                            "radius": NAN}),
    _c("disk_pos_inf", "nonfinite", {"type": "disk", "pos": (1.0, INF, 6.0), "axes": TILT, "radius": 4.0}),
    _c("plane_normal_nan", "nonfinite", {"type": "plane", "pos": (0.0, -4.0, 0.0),
                                         "axes": (1.0, 0.0, 0.0, 0.0, NAN, 0.0, 0.0, 0.0, 1.0)}),
]

# ---- one textured primitive of each type, filling a good part of a frame -------
# tests/test_gpu_texel_edges.py's objects and camera; tests/shading_cases.py builds on them too, and
# tests/golden/golden_r5.npz stores the scenes made from them (tests/test_oracle_golden_shading.py compares the bytes).
TEXEL_CAMERA = ((0.0, 0.0, 12.0), (0.0, 0.0, 0.0), 60.0)
TEXEL_FACING = axes_up((0.0, 0.0, 1.0))  # normal +z, columns x and -y
TEXEL_OBJECTS = {
    "sphere": {"type": "sphere", "pos": (0.0, 0.0, 6.0), "axes": axes_up((0.2, 1.0, 0.1)), "radius": 2.5},
    "disk": {"type": "disk", "pos": (0.0, 0.0, 6.0), "axes": TEXEL_FACING, "radius": 3.0},
    "annulus": {"type": "annulus", "pos": (0.0, 0.0, 6.0), "axes": TEXEL_FACING, "inner": 0.5, "outer": 3.0},
    "cylinder": {"type": "cylinder", "pos": (0.0, -2.5, 6.0), "axes": axes_up((0.1, 1.0, 0.0)), "height": 5.0,
                 "radius": 2.0},
    "rectangle": {"type": "rectangle", "pos": (-3.0, 1.75, 6.0), "axes": TEXEL_FACING, "width": 6.0, "height": 3.5},
    "box": {"type": "box", "pos": (-2.0, -2.0, 4.0), "axes": axes_up((0.3, 1.0, 0.2)), "width": 4.0, "depth": 4.0,
            "height": 4.0},
    "plane_patch": {"type": "plane", "pos": (0.0, 0.0, 6.0), "axes": TEXEL_FACING, "texture_offset": (-2.0, -1.5),
                    "repeat_texture": 0, "texture_size": (4.0, 3.0)},
    "plane_repeat": {"type": "plane", "pos": (0.0, 0.0, 6.0), "axes": TEXEL_FACING, "texture_offset": (-0.5, 0.25),
                     "repeat_texture": 1, "texture_size": (3.0, 2.0)},
}


def cell_id(cell):
    c, host, schedule = cell
    return f"{c.name}-{host}-{schedule}"


def changed_share(a, b):
    """The share of pixels in which two oracle frames (rgba8, rgba32, steps) differ."""
    fa, fb = a[1].view(np.uint32), b[1].view(np.uint32)
    both_nan = np.isnan(a[1]) & np.isnan(b[1])
    diff = ((fa != fb) & ~both_nan).any(-1) | (a[2] != b[2])
    return float(diff.mean())

