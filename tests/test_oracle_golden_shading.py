"""Pins the CPU oracle to the reference shader at the shading extremes.

tests/golden/golden_r5.npz (tests/golden/make_golden.py --set r5) holds the
reference fragment shader's frames and step maps, rendered on SwiftShader
under the "features" capacity profile (4 lights, 8 materials, 2 planes, 2
texture layers), of the cases of tests/shading_cases.py that fit it: the
"alone" host, every mode of the case, 65x41. The oracle is the only judge of
the kernel in tests/test_gpu_shading_extremes.py; this module is the last
link of "kernel == oracle == shader" there. tests/test_oracle_golden_extremes.py
does the same for the scene and view tables, under the same rules.

Every case is rebuilt from the table, and the scene, camera and params bytes
stored with the shader's frame must equal the table's: the table and the
fixture cannot drift apart.

The budget is tests/test_oracle_golden.py's: >= 99.9 % of the pixels within
2/255 per channel, none beyond 4/255, step counts equal on >= 99.9 %. A case
that samples no texture of its own is rendered with its own params (the
untextured budget). A case that samples a texture array, a normal map or a
skybox of its own is rendered with SwiftShader's filter
(oracle.FILTER_SWIFTSHADER, shading_cases.oracle_params_for_shader), as
test_oracle_golden.py's test_textured_all_pixels_with_swiftshader_filter
does: SwiftShader reads an opaque texel's alpha below 1, so its rays pass
textured surfaces, and with its filter the budget holds on every pixel.

ALLOW names the exceptions as exact counts (pixels beyond 4/255, pixels beyond
2/255, pixels whose step counts differ), asserted with no margin. The
generator prints the same figures for every case:
- light_at_hit, nm_disk: the centre pixel, where the light direction
  (light_at_hit) or the disk's tangent (nm_disk) is normalize(0). The oracle
  gives (NaN, NaN, NaN, 1), stored as 0; SwiftShader's pixel is the ambient
  term alone (69, 38, 15), as if that light added nothing. One pixel, so
  the case stays pinned on the other 2664.
- seam_sphere_pole, seam_disk_centre, seam_annulus_centre: the centre pixel,
  where phi = atan(0, 0), which GLSL leaves undefined: the oracle's atan2
  gives 0; SwiftShader's pixel is another blend of texels (up to 70/255
  off).
- the skyboxes seen looking up (and the 5x7x4 one looking down) in flat
  mode: the centre pixel's direction is (0, +-1, 0) exactly, u = atan(0, 0).
  The skyboxes one texel wide have one u and no exception; in curved mode
  the centre ray bends off the axis and there is none either.
- single_sided_behind, single_sided_flipped, single_sided_behind_flipped_half
  (crosshair on): rows 19 and 21, columns 38 to 47. The crosshair's
  horizontal arm is |uv.y * 41 / 2| < 1, and at rows 19 and 21 that product
  is 1 in exact arithmetic. The oracle computes uv.y = (2 y + 1) / 41 - 1 per
  pixel and gets no crosshair there; SwiftShader interpolates uv.y across
  the quad and lands below 1 on the right arm (on the left arm and on the
  vertical arm's neighbours, columns 31 and 33, the two agree). 20 pixels of
  128/255: the crosshair's 0.5. Inferred from the frames' differences, which
  lie exactly there; SwiftShader's uv was not read out.

EXCLUDED names the cases whose shader result rests on an operation GLSL
leaves undefined, each with the operation; they stay in
tests/test_shading_cases.py and tests/test_gpu_shading_extremes.py. The
fixture holds their frames apart, and each must be beyond 4/255 on more than
1 % of its pixels: a case the oracle matches is pinned, not excluded. Most
non-finite cases are pinned: pow(0, 0), pow(0, -2), shininess +-inf, every
NaN and infinite material, light and mapping term but the three below, the
divisions by a zero texture or plane size and the attenuation 1 / 0 all give
on SwiftShader what the oracle gives, 0 pixels off.
"""
from pathlib import Path

import numpy as np
import pytest

import shading_cases as S

GOLDEN_R5 = Path(__file__).resolve().parent / "golden" / "golden_r5.npz"
GOLDEN_R4 = GOLDEN_R5.with_name("golden_r4.npz")

# (pixels beyond 4/255, pixels beyond 2/255, pixels with other step counts), exact
CENTRE_PIXEL = (1, 1, 0)
CROSSHAIR_ROWS = (20, 20, 0)
ALLOW = {
    "light_at_hit/curved": CENTRE_PIXEL, "light_at_hit/flat": CENTRE_PIXEL,
    "nm_disk/curved": CENTRE_PIXEL,
    **{f"seam_{n}/{m}": CENTRE_PIXEL for n in ("sphere_pole", "disk_centre", "annulus_centre") for m in ("curved", "flat")},
    **{f"sky_{size}_up_f0/flat": CENTRE_PIXEL for size in ("2x1x3", "2x1x4", "3x2x3", "3x2x4", "5x7x3", "5x7x4")},
    "sky_5x7x4_down_f0/flat": CENTRE_PIXEL,
    "single_sided_behind/curved": CROSSHAIR_ROWS, "single_sided_flipped/curved": CROSSHAIR_ROWS,
    "single_sided_behind_flipped_half/curved": CROSSHAIR_ROWS,
}

EXCLUDED = {
    "spec_shin_nan": "pow with a NaN exponent (a non-finite uniform)",
    "light_pos_inf": "an infinite light position (a non-finite uniform): the light direction is normalize of a vector "
                     "with an infinite component, inf * 0",
    "nm_zero": "every texel of the normal map is 0: the shading normal is normalize(0)",
}


@pytest.fixture(scope="module")
def r5():
    if not GOLDEN_R5.exists():
        pytest.fail("tests/golden/golden_r5.npz missing (python tests/golden/make_golden.py --set r5)")
    return np.load(GOLDEN_R5)


def names(pin):
    return [f"{c.name}/{m}" for c in S.CASES if c.pin == pin for m in c.modes]


def stored(r5):
    """name -> (group key, index) of the fixture."""
    out = {}
    for key in bytes(r5["meta_groups"]).decode().split("\n"):
        for k, name in enumerate(bytes(r5[f"{key}/cases"]).decode().split("\n")):
            out[name] = (key, k)
    return out


def test_fixture_and_table_agree(r5):
    """The fixture holds exactly the table's pinned and excluded cases,
    rendered by SwiftShader; the exclusions are the table's "undefined"
    cases, every group keeps pinned ones, the allowances are pinned cases,
    the cases left out are those the shader cannot hold, and the file is no
    larger than golden_r4.npz."""
    assert b"SwiftShader" in bytes(r5["meta_renderer"])
    where = stored(r5)
    assert set(where) == set(names("pin")) | set(names("undefined"))
    assert {n for n, (key, _) in where.items() if key == "excluded"} == set(names("undefined"))
    assert set(EXCLUDED) == {c.name for c in S.CASES if c.pin == "undefined"}
    assert all(any(c.group == g and c.pin == "pin" for c in S.CASES) for g in S.GROUPS)
    assert set(ALLOW) <= set(names("pin"))
    assert GOLDEN_R5.stat().st_size <= GOLDEN_R4.stat().st_size


def test_cases_left_out_do_not_fit_the_shader(pkg):
    """pin = None: more primitives of a type or texture sizes than the
    "features" profile holds, a context without an upload, the weighted
    filter (the shader has one filter), or a skybox cell left out for the
    fixture's size (shading_cases.SKY_PINNED)."""
    for c in S.CASES:
        if c.pin is not None:
            continue
        bg, arr, _ = S.textures_of(pkg, c.textures)
        m = {**c.material, **c.material2}
        assert (len(c.specs) > 2 or bg is None or arr is None or c.params.get("filter_mode") == 1
                or m.get("normal_map_index", -1) >= 2 or c.group == "skybox"), c.name


def measure(pkg, oracle, r5, name):
    """The oracle's frame of the table's case against the stored one:
    (per-pixel max byte difference, step counts equal)."""
    key, k = stored(r5)[name]
    case, mode = S.BY_NAME[name.split("/")[0]], name.split("/")[1]
    scene, cam, params = S.build(pkg, case, "alone"), S.camera_of(pkg, case), S.params_of(pkg, case, mode)
    sc = pkg.scenes
    for what, struct in (("scene", scene), ("camera", cam), ("params", params)):
        assert np.array_equal(r5[f"{key}/{what}"][k], sc.struct_bytes(struct)), f"{name}: the stored {what} is not the table's"
    ref, ref_steps = S.decode_frames(r5[f"{key}/rgba8_planes_dx"][k:k + 1])[0], r5[f"{key}/steps"][k].astype(int)
    assert ref.shape == (S.H, S.W, 4)
    bg, arr, _ = S.textures_of(pkg, case.textures)
    rgba8, _, steps = oracle.render(scene, cam, S.oracle_params_for_shader(pkg, case, params), S.W, S.H,
                                    oracle.TextureSet(bg, arr))
    return np.abs(rgba8.astype(int) - ref.astype(int)).max(-1), ref_steps == steps


@pytest.mark.parametrize("name", names("pin"))
def test_oracle_within_budget_of_the_shader(pkg, oracle, r5, name):
    d, same_steps = measure(pkg, oracle, r5, name)
    figures = (int((d > 4).sum()), int((d > 2).sum()), int((~same_steps).sum()))
    print(f"MEASURED {name}: beyond 4/255 {figures[0]}, beyond 2/255 {figures[1]}, steps differ {figures[2]} of {d.size}")
    if name in ALLOW:
        assert figures == ALLOW[name], (name, figures)
        if ALLOW[name] == CENTRE_PIXEL:
            assert d[S.H // 2, S.W // 2] > 4, name
        else:
            rows, cols = np.nonzero(d > 4)
            assert set(rows) == {19, 21} and set(cols) == set(range(38, 48)), name
    else:
        assert np.mean(d <= 2) >= 0.999, (name, figures)
        assert figures[0] == 0, (name, figures, int(d.max()))
        assert np.mean(same_steps) >= 0.999, (name, figures)


@pytest.mark.parametrize("name", names("undefined"))
def test_excluded_cases_are_far_from_the_shader(pkg, oracle, r5, name):
    """A case is excluded because an undefined operation decides its frame,
    not because it is inconvenient: the oracle's frame is beyond 4/255 of
    SwiftShader's on more than 1 % of the pixels."""
    d, _ = measure(pkg, oracle, r5, name)
    print(f"MEASURED {name}: beyond 4/255 {int((d > 4).sum())} of {d.size}")
    assert (d > 4).mean() > 0.01, (name, int((d > 4).sum()))
