"""The table of tests/shading_cases.py is what it says, on the CPU oracle alone.

tests/test_gpu_shading_extremes.py compares the kernel with the oracle on
these materials, lights, mappings and skyboxes; a case whose extreme value
never reaches a pixel would pass there whatever shade_hit did with it. So for
every cell (case, host, mode):

- the frame differs from the baseline's (the same primitives, camera and
  params with plain_material, one_light and the standard textures) in at least
  2 % of the pixels (shading_cases.MIN_SHARE; the entries that declare 0 say
  why beside them);
- the float frame holds a NaN or an infinity exactly when the case is marked
  nonfinite;
- an aimed case shows its special value in the centre pixel;
- an alpha case changes the step count of at least 2 % of the pixels.

And per case: both signs of the attenuation denominator inside the
rectangle's image, more than SR_PS_HITS translucent hits in a row and an
exactly opaque "maybe" hit in front of logged ones for the hit-log case, one
colour from the 1x1 skyboxes and more than 100 from the larger ones, six
different faces of the box. These are conditions on the inputs: a case that
falls short gets another placement, never a lower bar.
"""
import numpy as np
import pytest

import shading_cases as S

CENTRE = (S.H // 2, S.W // 2)


@pytest.fixture(scope="module")
def render(pkg, oracle):
    """(case, host, mode, plain=False, scene=None) -> the oracle's read-only frame."""
    texsets = {}

    def tex(key):
        if key not in texsets:
            bg, arr, _ = S.textures_of(pkg, key)
            texsets[key] = oracle.TextureSet(bg, arr)
        return texsets[key]

    def run(case, host="alone", mode="curved", plain=False, scene=None):
        scene = scene if scene is not None else S.build(pkg, case, host, plain)
        out = oracle.render(scene, S.camera_of(pkg, case), S.params_of(pkg, case, mode), S.W, S.H,
                            tex("std" if plain else case.textures))
        for a in out:
            a.setflags(write=False)
        return out

    return run


def test_table_shape(pkg):
    """Every group and every listed value is in the table; names are unique."""
    assert {c.group for c in S.CASES} == set(S.GROUPS)
    assert len(S.BY_NAME) == len(S.CASES)
    assert (S.W % 2, S.H % 2) == (1, 1) and ((S.W + 15) // 16, (S.H + 15) // 16) == (5, 3)

    def has(vals, want):
        vals, want = [float(np.float32(v)) for v in vals], [float(np.float32(w)) for w in want]  # as the struct holds them
        return all(any((v != v and w != w) or v == w for v in vals) for w in want)

    mats = [c.material for c in S.CASES]
    assert has([m["shininess"] for m in mats if "shininess" in m], [0, 1, 2, 3, 0.5, 1e4, S.INF, -2, -S.INF, S.NAN])
    assert any(m.get("shininess") == -2.0 and m.get("specular") == 0.0 for m in mats)
    for f in ("ambient", "diffuse", "specular"):
        vals = [m[f] for m in mats if f in m and "shininess" not in m and "texture_index" not in m]
        assert has(vals, [S.INF, S.NAN]) and any(v < 0 for v in vals) and any(1 < v < S.INF for v in vals), f
    assert has([m["color"][3] for c, m in zip(S.CASES, mats) if "color" in m and c.group == "alpha"],
               [0, 0.5, S.BELOW_1, S.ABOVE_1, 2, -1, S.NAN, S.INF])
    assert S.BELOW_1 < 1.0 < S.ABOVE_1
    assert any(c.group == "light" and c.num_lights == 0 for c in S.CASES)
    lights = [c for c in S.CASES if c.group == "light" and c.lights]
    assert any(len(c.lights) == 4 for c in lights)
    four = next(c for c in lights if len(c.lights) == 4)
    assert len({(d["pos"], d["color"], d["intensity"], d["att"]) for d in four.lights}) == 4
    assert has([c.lights[0]["intensity"] for c in lights], [0, S.INF, S.NAN]) and any(c.lights[0]["intensity"] < 0
                                                                                   for c in lights)
    assert any(c.lights[0]["att"] == (0.0, 0.0, 0.0) for c in lights)
    assert any(c.lights[0]["att"][0] < 0 for c in lights) and any(c.lights[0]["att"][2] < 0 for c in lights)
    assert any(c.lights[0]["pos"] == S.HIT for c in lights) and any(c.lights[0]["pos"] == (0.0, 0.0, 0.0) for c in lights)
    assert any(c.lights[0]["pos"][0] == 1e30 for c in lights)
    assert has([c.lights[0]["pos"][0] for c in lights], [S.NAN, S.INF])
    assert has([k for c in lights for k in c.lights[0]["color"]], [S.NAN, 2.0, -0.5])
    assert {c.material.get("normal_map_index") for c in S.CASES if c.group == "mapping"} >= {0, 1, 2, 11}
    assert any(c.textures == "no_array" and c.material.get("texture_index", -1) >= 0 for c in S.CASES)
    assert any(c.textures == "no_bg" for c in S.CASES)
    sky = {c.textures for c in S.CASES if c.group == "skybox"}
    assert sky >= {f"sky{w}x{h}x{ch}" for w, h in ((1, 1), (2, 1), (1, 2), (3, 2), (5, 7)) for ch in (3, 4)}
    for key in sky - {"no_bg"}:
        bg = S.textures_of(pkg, key)[0]
        assert bg.shape[2] == 3 or bg[:, :, 3].max() < 255
    assert {c.params.get("filter_mode", 0) for c in S.CASES if c.group == "skybox"} == {0, 1}
    assert all(c.flat for c in S.CASES if c.group == "skybox")
    assert all(c.hosts == S.BOTH for c in S.CASES if c.group == "alpha" and c.specs is not S.LAYERS)
    assert {s["type"] for c in S.CASES if c.group == "normalmap" for s in c.specs} == set(S.X.TYPE_OF)
    assert any(c.group == "alpha" and c.params.get("crosshair") == 1 and c.material.get("flip_normals") for c in S.CASES)
    assert all(c.pin in (None, "pin", "undefined") for c in S.CASES)


@pytest.mark.parametrize("cell", S.cells(), ids=S.cell_id)
def test_case_is_what_it_says(pkg, oracle, render, cell):
    case, host, mode = cell
    label = S.cell_id(cell)
    frame, base = render(case, host, mode), render(case, host, mode, plain=True)
    share = float(S.changed(frame, base).mean())
    assert share >= case.visible, f"{label}: {share:.4f} of the frame differs from the baseline"
    if case.visible == 0.0:  # what the table says beside these entries: the frame is the baseline's, bit for bit
        assert share == 0.0, f"{label}: declared to show nothing, {share:.4f} of the frame differs from the baseline"
    bad = int((~np.isfinite(frame[1])).any(-1).sum())
    assert (bad > 0) == case.nonfinite, f"{label}: {bad} pixels with a NaN or an infinity, nonfinite = {case.nonfinite}"
    centre = frame[1][CENTRE]
    if case.aim == "nan_rgb":
        assert np.isnan(centre[:3]).all() and centre[3] == 1.0, f"{label}: centre pixel {centre}"
    elif case.aim is not None:
        kind, u, v = case.aim
        assert kind == "texel"
        want = oracle.sample_texture(S.textures_of(pkg, case.textures)[1][0], u, v, case.params.get("filter_mode", 0))
        assert np.array_equal(centre[:3].view(np.uint32), want[:3].view(np.uint32)), f"{label}: {centre} != {want}"
    if case.group == "alpha":
        steps = float((frame[2] != base[2]).mean())
        assert steps >= S.MIN_SHARE, f"{label}: {steps:.4f} of the step counts differ from the opaque baseline's"


def test_nonfinite_cells_hold_every_kind(render):
    """write_pixel's unorm8 stores NaN as 0, +inf as 255 and -inf as 0, and
    tests/test_gpu_shading_extremes.py checks each rule on the pixels that
    hold the value: NaN, +inf and -inf each occur in the float frames of the
    nonfinite cells, in the plain frame and in the 130x82 frame sr_render_ss
    averages (rendered here at the plain size: the same rays at other
    pixels), each on at least 2 % of some frame's channels."""
    best = {"nan": 0.0, "+inf": 0.0, "-inf": 0.0}
    for case, host, mode in S.cells():
        if not case.nonfinite:
            continue
        f = render(case, host, mode)[1]
        for kind, mask in (("nan", np.isnan(f)), ("+inf", f == np.inf), ("-inf", f == -np.inf)):
            best[kind] = max(best[kind], float(mask.mean()))
    assert all(v >= S.MIN_SHARE for v in best.values()), best


def test_attenuation_denominator_changes_sign(pkg, render):
    """att_const_neg: with one light in front of the rectangle the colour is
    ambient + (diffuse + specular) * intensity / denominator and the bracket
    is positive, so red above the ambient term is a positive denominator and
    red below it a negative one: both on at least 2 % of the frame."""
    case = S.BY_NAME["light_att_const_neg"]
    red = render(case)[1][:, :, 0]
    on = S.changed(render(case), render(case, scene=pkg.scenes.scene_black_hole_only()))
    ambient = np.float32(0.3) * np.float32(0.9)
    pos, neg = float((on & (red > ambient)).mean()), float((on & (red < ambient)).mean())
    assert pos >= S.MIN_SHARE and neg >= S.MIN_SHARE, (pos, neg)


def test_hit_log_fills_and_an_opaque_maybe_hit_hides_logged_ones(pkg, render):
    """hit_log_weighted. The same geometry with material 2
    untextured (1, 0, 0, 0) at ambient 1, material 0 opaque black and no
    light counts in red the translucent layers in front of the first layer
    of material 0: more than SR_PS_HITS on at least 2 % of the pixels, with
    the case's own ray running at least as far as that layer (so its log
    fills with four translucent hits and the next hit is shaded by a later
    round: that this is sr_resume_kernel's work is read from the kernel's
    code, nothing here or on the GPU observes the launch), and exactly one
    (layer A, then D1 in front of B and C) with the case's own ray ending
    there, at D1's step count, on at least 2 %."""
    case = S.BY_NAME["hit_log_weighted"]
    for host in case.hosts:
        s = S.build(pkg, case, host)
        for index, color in ((0, (0.0, 0.0, 0.0, 1.0)), (2, (1.0, 0.0, 0.0, 0.0))):
            S.X.plain_material(s.materials[index], color)
            s.materials[index].ambient = 1.0
        s.num_lights = 0
        count, frame = render(case, host, scene=s), render(case, host)
        n = count[1][:, :, 0]
        assert np.array_equal(n, np.round(n)), np.unique(n)  # (every ray ends on material 0: no sky in the count)
        # (a material-2 texel whose weighted alpha is exactly 1 would end the case's own ray in front of the first
        # material-0 layer, at a smaller step count than the count frame's: those pixels do not count as filled)
        filled = float(((n > S.PS_HITS) & (frame[2] >= count[2])).mean())
        hidden = float(((n == 1.0) & (frame[2] == count[2])).mean())
        assert filled >= S.MIN_SHARE and hidden >= S.MIN_SHARE, (host, filled, hidden)


def test_skybox_colours(render):
    """A 1x1 skybox gives one colour (two where the hole is in view: the sky
    and the hole's black); every larger one more than 100 distinct float
    colours, in every view, mode and filter."""
    for case in S.CASES:
        if case.group != "skybox" or case.specs or case.textures == "no_bg":
            continue
        for mode in case.modes:
            n = S.distinct_colours(render(case, "alone", mode))
            if case.textures.startswith("sky1x1x"):
                view = case.name.split("_")[2]
                assert n == (2 if view in S.HOLE_IN_VIEW else 1), (case.name, mode, n)
            else:
                assert n > 100, (case.name, mode, n)


def test_box_views_show_six_faces(render):
    """The six cameras around the box see six different faces: the centre
    pixels' colours are pairwise different."""
    centres = {v: render(S.BY_NAME["nm_box_" + v])[1][CENTRE].tobytes() for v in S.BOX_VIEWS}
    assert len(set(centres.values())) == 6
