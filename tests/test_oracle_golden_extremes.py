"""Pins the CPU oracle to the reference shader at the extremes.

tests/golden/golden_r4.npz (tests/golden/make_golden.py --set r4) holds the
reference fragment shader's frames and step maps, rendered on SwiftShader,
of tests/extreme_cases.py's primitives alone (every group but the non-finite
one, every schedule, 64x40) and of tests/view_cases.py's cameras and
parameters on scenes.scene_default(False) (68x44). The oracle is the only
judge of the kernel in tests/test_gpu_scene_extremes.py and
tests/test_gpu_view_extremes.py; this module is the last link of
"kernel == oracle == shader" there.

Every case is rebuilt from the tables, and the scene, camera and params bytes
stored with the shader's frame must equal the table's: the tables and the
fixture cannot drift apart.

The budget is tests/test_oracle_golden.py's for untextured scenes: >= 99.9 %
of the pixels within 2/255 per channel, none beyond 4/255, step counts equal
on >= 99.9 %, on every pinned case.

ALLOW names the exceptions as exact counts (pixels beyond 4/255, pixels beyond
2/255, pixels whose step counts differ), asserted with no margin - the oracle
and the fixture are both deterministic, so a regression cannot hide in them.
The generator prints the same figures for every case:
- box_height_0: two coincident faces. The two hits have equal lambda up to
  rounding and opposite normals; which one is nearer is decided in the last
  bit of two plane intersections, and the shading flips with it (7 pixels at
  400 steps, 1 at 100, max 186/255; every step count equal).
- cylinder_r0p05_h20: a cylinder 0.05 thick seen from 10 units. One pixel's
  chord grazes it (9/255 and 16/255), at 400 steps one more within 4/255 and
  one step count.
- pos_r1e5_fov2, pos_r1e15_fov2: the first reseed (frag:891-912) intersects
  the ray from r = 1e5 / 1e15 with the sphere r = 1 / u_f = 100 in binary32:
  the discriminant is the difference of (ro . rd)^2 and |ro|^2 - 1e4, numbers
  of 1e10 (ulp 1024) and 1e30 (ulp 7.6e22). From 1e5 the 14 pixels whose rays
  pass 56 .. 202 from the origin (true discriminants within 30 ulp of 0) get
  the other sign on SwiftShader (4 of them beyond 4/255); from 1e15 the
  sixteen central pixels, whose rays pass 5.6e11 .. 1.7e12 from the origin
  (true discriminants of 4 .. 40 ulp), do. Computed in doubles from the
  camera and the pixel; the oracle evaluates the shader's expression in IEEE
  binary32 without contraction, SwiftShader's dot and square round otherwise.
  The last bits of a far sphere intersection, not an error of the oracle; the
  kernel agrees with the oracle on these frames bit for bit.
  This is computed from the cameras and the frames, not read from a trace of
  the kernel (tools/trace_pixel.py needs a device and a printf build).
- uf_0p01_r100_up: the camera one float above r = 100 with u_f = 0.01. The
  first compare u < u_f is between 1 / length(pos) and 0.01f, which differ by
  one ulp when length and the division are correctly rounded (the oracle:
  r = 100.0000076, u = 0.0099999988 < 0.00999999978: every ray reseeds at
  step 0). GLSL ES grants length and division 2.5 ulp. That SwiftShader's u
  lands on the other side (no reseed at step 0) is inferred from its frame
  and step map, which differ on 744 and 784 pixels as a frame without that
  reseed does; its u was not read out. The cameras at r = 100 exactly and
  one float below have no exception.
- black_0p0: percent_black = 0 masks the pixels whose rand() =
  fract(sin(x) * 43758.5453) is <= 0, that is exactly 0 (frag:839-841). Which
  pixels those are is decided by the last bits of sin: the oracle masks 9,
  and 22 pixels are masked by one of the two and not the other (black against
  a picture: max 255, their step counts 0 against the ray's).
- black_0p5: the same rand() against 0.5. The two masks are uncorrelated
  where sin's last bits differ, 1466 of 2992 pixels; every pixel neither masks
  is within 2/255 with equal step counts. For these two cases the masked
  shares must also agree within 2 % (tests/test_oracle_golden.py's noise
  budget), in addition to the exact counts.

EXCLUDED names the cases whose shader result rests on an operation GLSL
leaves undefined, each with the operation; they stay in
tests/test_view_cases.py and tests/test_gpu_view_extremes.py. The fixture
holds their frames apart, and each must be beyond 4/255 on more than 1 % of
its pixels: a case the oracle matches is pinned, not excluded (the non-finite
u_f, position, curved_percentage and percent_black cases are: 0 pixels off).
Every group keeps pinned cases.
"""
from pathlib import Path

import numpy as np
import pytest

import extreme_cases as X
import view_cases as V

GOLDEN_R4 = Path(__file__).resolve().parent / "golden" / "golden_r4.npz"

# (pixels beyond 4/255, pixels beyond 2/255, pixels with other step counts), exact
ALLOW = {
    "scene/box_height_0/400x2": (7, 7, 0),
    "scene/box_height_0/100x2": (1, 1, 0),
    "scene/cylinder_r0p05_h20/400x2": (1, 2, 1),
    "scene/cylinder_r0p05_h20/100x2": (1, 1, 0),
    "view/pos_r1e5_fov2": (4, 4, 14),
    "view/pos_r1e15_fov2": (16, 16, 0),
    "view/uf_0p01_r100_up": (744, 760, 784),
    "view/black_0p0": (22, 22, 22),
    "view/black_0p5": (1466, 1466, 1466),
}
MASK_SHARE = ("view/black_0p0", "view/black_0p5")  # also: masked shares within 2 %

EXCLUDED = {
    "rev_0": "every step angle is 0, so every chord has zero length and its direction is normalize(0) = 0 / 0",
    "pos_r1": "u = 1 at the start: the orbit's tangent at the horizon, du = -u (rd . n) / (rd . t), is 0 / 0 for the "
              "radial rays and the first chord's end divides by u - 1 rounding to 0",
    "fov_0p0": "the ray direction is normalize of a vector with tan(0) = 0 in x and y; every ray is exactly radial "
               "and the orbital frame's tangent is normalize(0)",
    "fov_nan": "tan(NaN)",
    "pos_origin": "u = 1 / length(0) and the orbital frame's normal is normalize(0)",
    "pos_nan_y": "arithmetic on a NaN position",
    "axes_zero": "the ray direction is normalize(0)",
    "axes_nan_forward": "arithmetic on a NaN axis",
}


@pytest.fixture(scope="module")
def r4():
    if not GOLDEN_R4.exists():
        pytest.fail("tests/golden/golden_r4.npz missing (python tests/golden/make_golden.py --set r4)")
    return np.load(GOLDEN_R4)


@pytest.fixture(scope="module")
def texsets(pkg, oracle, r4):
    arr = pkg.scenes.default_texture_array()[0]
    out = {}
    for kind in ("scene", "view"):
        h, w = (int(v) for v in r4[f"meta_skybox_shape_{kind}"])
        out[kind] = oracle.TextureSet(pkg.scenes.skybox(w, h), arr)
    return out


def table_cases(pkg):
    """name -> (scene, camera, params, (W, H)) of every stored case, from the tables."""
    out = {}
    for c in X.CASES:
        if c.group == "nonfinite":
            continue
        for schedule in c.schedules:
            out[f"scene/{c.name}/{schedule}"] = (lambda c=c, s=schedule: (X.build(pkg, c, "alone"), X.camera_of(pkg, c),
                                                                          X.params_of(pkg, c, s), (X.W, X.H)))
    for c in V.CASES:
        out[f"view/{c.name}"] = (lambda c=c: (V.host_scene(pkg, "golden"), V.camera_of(pkg, c), V.params_of(pkg, c),
                                                  c.size))
    return out


def stored(r4):
    """name -> (group key, index) of the fixture."""
    out = {}
    for key in bytes(r4["meta_groups"]).decode().split("\n"):
        for k, name in enumerate(bytes(r4[f"{key}/cases"]).decode().split("\n")):
            out[name] = (key, k)
    return out


def pinned_names():
    names = [f"scene/{c.name}/{s}" for c in X.CASES if c.group != "nonfinite" for s in c.schedules]
    return names + [f"view/{c.name}" for c in V.CASES if c.pinned]


def excluded_names():
    return [f"view/{c.name}" for c in V.CASES if not c.pinned]


def test_fixture_and_tables_agree(pkg, r4):
    """The fixture holds exactly the tables' pinned cases, rendered by
    SwiftShader, with the skyboxes the issue names; the exclusions are the
    table's non-pinned cases, every group keeps a pinned one, and the
    allowances are pinned cases."""
    assert b"SwiftShader" in bytes(r4["meta_renderer"])
    assert [int(v) for v in r4["meta_skybox_shape_scene"]] == [128, 256]
    assert [int(v) for v in r4["meta_skybox_shape_view"]] == [256, 512]
    where = stored(r4)
    assert set(where) == set(table_cases(pkg)) == set(pinned_names()) | set(excluded_names())
    assert {n for n, (key, _) in where.items() if key.startswith("excluded_")} == set(excluded_names())
    assert {"view/" + n for n in EXCLUDED} == set(excluded_names())
    assert not any(c.finite and c.agrees for c in V.CASES)
    pinned = set(pinned_names())
    assert all(any(c.group == g and f"view/{c.name}" in pinned for c in V.CASES) for g in V.GROUPS)
    assert all(any(c.group == g and f"scene/{c.name}/{s}" in pinned for c in X.CASES for s in c.schedules)
               for g in X.MIN_SHARE if g != "nonfinite")
    assert set(ALLOW) <= pinned and set(MASK_SHARE) <= set(ALLOW)


def measure(pkg, oracle, r4, texsets, name):
    """The oracle's frame of the table's case against the stored one:
    (oracle rgba8, shader rgba8, per-pixel max byte difference, step counts equal)."""
    key, k = stored(r4)[name]
    scene, cam, params, (w, h) = table_cases(pkg)[name]()
    sc = pkg.scenes
    for what, struct in (("scene", scene), ("camera", cam), ("params", params)):
        assert np.array_equal(r4[f"{key}/{what}"][k], sc.struct_bytes(struct)), f"{name}: the stored {what} is not the table's"
    ref, ref_steps = r4[f"{key}/rgba8"][k], r4[f"{key}/steps"][k].astype(int)
    assert ref.shape == (h, w, 4)
    rgba8, _, steps = oracle.render(scene, cam, params, w, h, texsets[name.split("/")[0]])
    d = np.abs(rgba8.astype(int) - ref.astype(int)).max(-1)
    same_steps = ref_steps == steps % 65536  # (the shader's step map holds two bytes of the count)
    return rgba8, ref, d, same_steps


@pytest.mark.parametrize("name", pinned_names())
def test_oracle_within_budget_of_the_shader(pkg, oracle, r4, texsets, name):
    rgba8, ref, d, same_steps = measure(pkg, oracle, r4, texsets, name)
    figures = (int((d > 4).sum()), int((d > 2).sum()), int((~same_steps).sum()))
    print(f"MEASURED {name}: beyond 4/255 {figures[0]}, beyond 2/255 {figures[1]}, steps differ {figures[2]} of {d.size}")
    if name in ALLOW:
        assert figures == ALLOW[name], (name, figures)
        if name in MASK_SHARE:
            black_o, black_r = (rgba8 == 0).all(-1), (ref == 0).all(-1)
            assert abs(black_o.mean() - black_r.mean()) < 0.02, (name, black_o.mean(), black_r.mean())
            both = ~black_o & ~black_r
            assert both.any() and not (d[both] > 2).any() and same_steps[both].all(), name
    else:
        assert np.mean(d <= 2) >= 0.999, (name, figures)
        assert figures[0] == 0, (name, figures, int(d.max()))
        assert np.mean(same_steps) >= 0.999, (name, figures)


@pytest.mark.parametrize("name", excluded_names())
def test_excluded_cases_are_far_from_the_shader(pkg, oracle, r4, texsets, name):
    """A case is excluded because an undefined operation decides its frame,
    not because it is inconvenient: the oracle's frame is beyond 4/255 of
    SwiftShader's on more than 1 % of the pixels."""
    _, _, d, _ = measure(pkg, oracle, r4, texsets, name)
    print(f"MEASURED {name}: beyond 4/255 {int((d > 4).sum())} of {d.size}")
    assert (d > 4).mean() > 0.01, (name, int((d > 4).sum()))
