"""Cameras and frame parameters no other module sets (a helper, not a test module).

CASES is a table of named cases for tests/test_view_cases.py (the oracle
alone: is the case what it says?), tests/test_gpu_view_extremes.py (the kernel
against the oracle, culling on against off) and the finite ones for
tests/golden/make_golden.py --set r4 (the oracle against the reference
shader). A case is a camera, overrides of the frame parameters and the class
of frame the oracle must give:

    Case.group    u_f | revolutions | fov | position | axes | split | noise | schedule
    Case.pos      the camera's position; it looks at Case.target (from
                  LOOK_FROM when the position has no direction of its own)
    Case.fov
    Case.axes     a function of the look-at camera's nine axes (column-major:
                  right, up, forward), or None
    Case.params   overrides of PARAMS
    Case.size     (W, H) of the frame
    Case.expect   rich            >= 50 distinct colours, >= 2 % of the pixels
                                  differ from the default frame's
                  equals_default  the default frame, bit for bit
                  all_nan         one colour, every ray runs max_steps steps
                  no_steps        every ray ends before the step loop
                  one_step        every ray ends at its first step
                  near_default    >= 50 distinct colours; at least one pixel and
                                  fewer than 2 % differ from the default frame
                                  (percent_black = 0: rand() <= 0 masks the
                                  pixels whose rand() is exactly 0)
                  overshoot       every ray takes a step and at most three
                                  colours come out. A step angle of 45 rad:
                                  RK4 multiplies u by about 1.7e5 in the first
                                  step, so its chord runs from the camera to
                                  the origin and ends in the hole or in what
                                  lies between; no camera tried (fields of 10
                                  to 60 degrees, at the hole and past it, from
                                  r = 15, 25 and 30) gives more than three
                                  colours. The two cases of the class together
                                  must show two step counts and the scene's
                                  objects on each host
                                  (tests/test_view_cases.py)
    Case.finite   every field finite and every operation of the shader
                  defined (the GPU matrix runs these first)
    Case.pinned   golden_r4.npz pins the oracle to the shader's frame: the
                  finite cases and the non-finite ones on which the two
                  agree (tests/test_oracle_golden_extremes.py EXCLUDED says
                  of each other case which operation is undefined)

The default frame is the host scene from CAM0 with PARAMS at the case's size.
Hosts: "small" (scenes.scene_default(True)), "large" (scenes.scene_stress());
the shader's frames of golden_r4.npz are of scenes.scene_default(False).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

W, H = 68, 44  # tests/test_gpu_launch_matrix.py's frame: every wave shape is partial somewhere
STEPS = 400
PARAMS = {"max_steps": STEPS, "percent_black": -1.0, "crosshair": 0}
HOSTS = ("small", "large")
EXPECT = ("rich", "equals_default", "all_nan", "no_steps", "one_step", "near_default", "overshoot")
GROUPS = ("u_f", "revolutions", "fov", "position", "axes", "split", "noise", "schedule")
OVERLAY_GROUPS = ("u_f", "revolutions")  # the GPU matrix runs these with the press-R overlay too

NAN, INF = float("nan"), float("inf")
LOOK_FROM = (0.0, 2.0, 15.0)  # the app's camera position
F32 = np.float32


def f32(x) -> float:
    return float(F32(x))


def at_radius(r: float, direction=LOOK_FROM) -> tuple:
    d = np.asarray(direction, dtype=np.float64)
    d = d / np.linalg.norm(d)
    return tuple(f32(v * r) for v in d)


@dataclass
class Case:
    name: str
    group: str
    expect: str
    pos: tuple = LOOK_FROM
    target: tuple = (0.0, 0.0, 0.0)
    fov: float = 90.0
    axes: object = None
    params: dict = field(default_factory=dict)
    size: tuple = (W, H)
    finite: bool = True
    agrees: bool = False  # not finite, and yet the shader's frame on SwiftShader is the oracle's

    @property
    def pinned(self) -> bool:
        return self.finite or self.agrees


# ---- camera axes (column-major: right, up, forward) ------------------------------
def scaled(k):
    return lambda a: [f32(v * k) for v in a]


def sheared(a, k=0.3):
    """c1 += k c0"""
    a = list(a)
    for i in range(3):
        a[3 + i] = f32(a[3 + i] + k * a[i])
    return a


def left_handed(a):
    a = list(a)
    for i in range(3):
        a[i] = -a[i]
    return a


def zero_axes(a):
    return [0.0] * 9


def nan_forward(a):
    a = list(a)
    a[7] = NAN
    return a


def camera_of(pkg, case):
    """The look-at camera of the case's position (built from its finite
    stand-in where a component is not finite or the position is the origin),
    then the position, the field of view and the axes of the case."""
    look = tuple(p if np.isfinite(p) else l for p, l in zip(case.pos, LOOK_FROM))
    if not any(look):
        look = LOOK_FROM
    fwd = np.asarray(case.target, dtype=np.float64) - np.asarray(look, dtype=np.float64)
    fwd = fwd / np.linalg.norm(fwd)  # (in double: |pos|^2 overflows binary32 at r = 1e25)
    cam = pkg.scenes.camera_look(look, tuple(float(v) for v in fwd), fov=90.0)
    for i in range(3):
        cam.transform.pos[i] = case.pos[i]
    cam.fov = case.fov
    if case.axes is not None:
        ax = case.axes(list(cam.transform.axes))
        for i in range(9):
            cam.transform.axes[i] = ax[i]
    return cam


def params_of(pkg, case):
    return pkg.abi.default_params(**{**PARAMS, **case.params})


def default_camera(pkg):
    return camera_of(pkg, Case("default", "u_f", "equals_default"))


def default_params(pkg):
    return pkg.abi.default_params(**PARAMS)


def host_scene(pkg, host):
    sc = pkg.scenes
    return {"small": lambda: sc.scene_default(True), "large": sc.scene_stress,
            "golden": lambda: sc.scene_default(False)}[host]()


# ---- the table -------------------------------------------------------------------
def _name(x) -> str:
    return repr(x).replace("-", "m").replace(".", "p").replace("+", "")


def _uf(v, label=None, expect="rich", **kw):
    return Case("uf_" + (label or _name(v)), "u_f", expect, params={"u_f": v}, **kw)


# A negative max_revolutions makes every step angle negative: the traced
# point moves against the ray's direction in both its radial and tangential
# part, so the frame shows what lies behind the camera. Looking at the origin
# it is sky alone (the scene's objects change no pixel of it); these cameras
# look away from it (with u_f = 0.2 from inside r = 5: outside, every ray is
# flat from its first step).


def _rev(v, expect="rich", label=None, pos=LOOK_FROM, fov=90.0, **params):
    return Case("rev_" + (label or _name(v)), "revolutions", expect, pos=pos, fov=fov,
                target=tuple(2.0 * p for p in pos) if v < 0 else (0.0, 0.0, 0.0),
                params={"max_revolutions": v, **params}, finite=v != 0)


def _fov(v, expect="rich", **kw):
    return Case("fov_" + _name(v), "fov", expect, fov=v, **kw)


# The stress scene fills CAM0's frame: 0.8 % of its pixels see the reseed
# radius. From above, u_f <= 0 changes 28 % of its frame (89 % of the default
# scene's) against u_f = 0.01 from the same camera.
ABOVE = (0.0, 25.0, 5.0)

# r = 100 exactly in binary32 and in the host's double sum (60^2 + 80^2), and
# the positions one float above and below it
R100 = (0.0, 60.0, 80.0)
R100_UP = (0.0, 60.0, float(np.nextafter(F32(80.0), F32(INF))))
R100_DOWN = (0.0, 60.0, float(np.nextafter(F32(80.0), F32(0.0))))

CASES = [
    # -- u_f: the reseed radius 1 / u_f, the windows' lower bound, the coasting
    # loop's compares, uf_radius2 and xplane_s on the host. u_f <= 0 and NaN
    # never reseed (u < u_f is false until u < 0 ends the ray): one frame.
    _uf(0.0, "0", pos=ABOVE), _uf(-0.0, "m0", pos=ABOVE), _uf(-0.01, pos=ABOVE), _uf(1e-40, "denormal", pos=ABOVE),
    _uf(0.3), _uf(0.5),
    _uf(0.6),  # the coasting predicate's constant
    _uf(0.66), _uf(f32(2.0 / 3.0), "2_3"), _uf(1.0), _uf(2.0),
    _uf(INF, "inf", expect="one_step", finite=False, agrees=True),
    _uf(NAN, "nan", pos=ABOVE, finite=False, agrees=True),
    # win_ok's <=: uf_radius = 100 exactly, cameras at r = 100 and one float either side
    _uf(0.01, "0p01_r100", pos=R100, fov=30.0), _uf(0.01, "0p01_r100_up", pos=R100_UP, fov=30.0),
    _uf(0.01, "0p01_r100_down", pos=R100_DOWN, fov=30.0),
    # -- revolutions: the step angle's sign and size (max_angle, every table
    # entry, out_dip, max_dphi, bh_u2 / bh_u3)
    _rev(-2), _rev(-1), _rev(0, "all_nan"), _rev(1), _rev(3), _rev(8), _rev(50),
    _rev(50, "overshoot", label="50_steps7", max_steps=7),
    _rev(50, "overshoot", label="50_steps7_above", pos=ABOVE, fov=30.0, max_steps=7), _rev(-1, label="m1_uf0p2", pos=(0.0, 0.6, 4.5), u_f=0.2),
    # -- fov: tan(fov / 2) is 0, huge, negative, NaN
    _fov(0.0, "all_nan", finite=False),
    _fov(1.0, target=(0.0, 3.0, 0.0)),  # (at the origin a field of 1 degree shows the hole alone)
    _fov(179.0), _fov(180.0), _fov(181.0), _fov(270.0),
    _fov(360.0, "no_steps"), _fov(-90.0), _fov(NAN, "all_nan", finite=False),
    # -- camera position
    Case("pos_origin", "position", "all_nan", pos=(0.0, 0.0, 0.0), finite=False),
    # on the horizon (u = 1 at the start), looking along it: a third of the rays fall in, the others leave
    Case("pos_r1", "position", "rich", pos=(0.0, 0.0, 1.0), target=(1.0, 0.0, 1.0), finite=False),
    Case("pos_r1e5_fov2", "position", "rich", pos=at_radius(1e5), fov=2.0),
    Case("pos_r1e15_fov2", "position", "rich", pos=at_radius(1e15), fov=2.0),
    Case("pos_r1e25_fov2", "position", "one_step", pos=at_radius(1e25), fov=2.0),  # |pos|^2 = inf, u = 0
    Case("pos_nan_y", "position", "all_nan", pos=(0.0, NAN, 15.0), finite=False),
    Case("pos_inf_y", "position", "one_step", pos=(0.0, INF, 15.0), finite=False, agrees=True),
    # -- camera axes: the ray direction is normalize(axes * v), so a scale drops out
    Case("axes_x2", "axes", "equals_default", axes=scaled(2.0)),
    Case("axes_x1em20", "axes", "rich", axes=scaled(1e-20)),  # |axes * v|^2 is denormal
    Case("axes_sheared", "axes", "rich", axes=sheared),
    Case("axes_left_handed", "axes", "rich", axes=left_handed),
    Case("axes_zero", "axes", "all_nan", axes=zero_axes, finite=False),
    Case("axes_nan_forward", "axes", "all_nan", axes=nan_forward, finite=False),
    # -- split modes: uv.x (2) or uv.y (3) < curved_percentage is curved
    *[Case(f"split{t}_cp_{_name(cp)}", "split", expect, params={"raytrace_type": t, "curved_percentage": cp},
           finite=cp == cp, agrees=cp != cp)
      for t in (2, 3)
      for cp, expect in ((-0.5, "rich"), (0.0, "rich"), (1.0, "equals_default"), (1.5, "equals_default"),
                         (NAN, "equals_default"))],
    # -- noise mask: rand() < percent_black is black, rand() in [0, 1)
    *[Case(f"black_{_name(pb)}", "noise", expect, params={"percent_black": pb}, finite=pb == pb, agrees=pb != pb)
      for pb, expect in ((0.0, "near_default"), (0.5, "rich"), (1.0, "no_steps"), (2.0, "no_steps"),
                         (NAN, "equals_default"))],
    # -- schedule: dphi = 1.9e-4, out_dip's fixed 1e-6 dominates dphi^2 / 8
    Case("steps_65536", "schedule", "rich", params={"max_steps": 65536}, size=(16, 8)),
]

BY_NAME = {c.name: c for c in CASES}


def cells():
    """(case, host) of the GPU matrix and of the oracle's check."""
    return [(c, h) for c in CASES for h in HOSTS]


def cell_id(cell):
    return f"{cell[0].name}-{cell[1]}"


def changed(a, b):
    """The pixels in which two (rgba8, rgba32, steps) frames differ (NaN = NaN)."""
    fa, fb = a[1].view(np.uint32), b[1].view(np.uint32)
    both_nan = np.isnan(a[1]) & np.isnan(b[1])
    return (a[0] != b[0]).any(-1) | ((fa != fb) & ~both_nan).any(-1) | (a[2] != b[2])


def distinct_colours(rgba8) -> int:
    return len(np.unique(np.ascontiguousarray(rgba8).reshape(-1, 4).view(np.uint32)))


def check_expectation(case, frame, default, label):
    """The case's frame is of its class (conditions on the table's inputs)."""
    rgba8, _, steps = frame
    max_steps = {**PARAMS, **case.params}["max_steps"]
    if case.expect == "rich":
        n, share = distinct_colours(rgba8), float(changed(frame, default).mean())
        assert n >= 50 and share >= 0.02, f"{label}: {n} colours, {share:.4f} of the frame differs from the default"
    elif case.expect == "equals_default":
        assert not changed(frame, default).any(), f"{label}: {int(changed(frame, default).sum())} pixels differ"
    elif case.expect == "all_nan":
        assert distinct_colours(rgba8) == 1 and (steps == max_steps).all(), \
            f"{label}: {distinct_colours(rgba8)} colours, steps {steps.min()} .. {steps.max()}"
    elif case.expect == "no_steps":
        assert (steps == 0).all(), f"{label}: steps {steps.min()} .. {steps.max()}"
    elif case.expect == "one_step":
        assert (steps == 1).all(), f"{label}: steps {steps.min()} .. {steps.max()}"
    elif case.expect == "near_default":
        n, k = distinct_colours(rgba8), int(changed(frame, default).sum())
        assert n >= 50 and 1 <= k < 0.02 * steps.size, f"{label}: {n} colours, {k} pixels differ from the default"
    elif case.expect == "overshoot":
        n = distinct_colours(rgba8)
        assert n <= 3 and steps.min() >= 1, f"{label}: {n} colours, steps {steps.min()} .. {steps.max()}"
    else:
        raise ValueError(case.expect)
