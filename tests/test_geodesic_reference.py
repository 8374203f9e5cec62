"""tests/geodesic_reference.py deserves trust before the kernel is compared
with it (tests/test_gpu_lens_physics.py): its exact geodesics against closed
forms, its classes against the analytic rule, the golden files against a fresh
computation, its scheme model against the exact geodesics (truncation) and
against the unchanged oracle (convention errors, caught here where no GPU
test runs). CPU only.

Measured here (python tests/golden/make_lens_reference.py prints them too):
the float64 model's exit direction at 2000 steps is within 1e-5 rad of the
exact one on all but 27 of the 762 level-C sky rays, at most 4.6e-5 on those:
rays that leave the r = 1 / u_f sphere at a grazing angle (b from 89.6 to 100.4),
where the shader's last chord, not a tangent, is the exit direction. That
first-order term is bounded from the reference alone
(geodesic_reference.exit_chord_term, at most 9.4e-5 rad on this set) and the
assertion is max(1e-5, that bound) per ray. At 64, 128, 256 and 512 steps the
maxima are 3.5e-2, 2.0e-3, 3.4e-4 and 1.6e-4 rad (recorded, not asserted).
"""
import math

import numpy as np
import pytest

import geodesic_reference as G

F = np.float32
SKY_W, SKY_H = 32, 16  # texels of 0.196 rad: at 256 x 128 a fifth of the sky rays lie within their tolerance of a border
MAX_BORDER_SHARE = 0.10


@pytest.fixture(scope="module")
def lens():
    return G.Lens.load()


@pytest.fixture(scope="module")
def tol():
    return G.Lens.tolerances()


# ---- closed forms -------------------------------------------------------------------------
def closed_deflection(b):
    """2 int_0^{u_p} du / sqrt(1 / b^2 - u^2 + u^3) - pi at 30 digits, u_p the periapsis: with
    u = u_p - x^2 the integrand is smooth, 2 / sqrt((u_p - x^2 - u_1)(u_3 - u_p + x^2))."""
    import mpmath as mp

    with mp.workdps(30):
        b = mp.mpf(b)
        roots = sorted(mp.polyroots([1, -1, 0, 1 / b ** 2], maxsteps=200, extraprec=200), key=lambda z: z.real)
        assert all(abs(z.imag) < mp.mpf(10) ** -25 for z in roots), "b below critical"
        u1, up, u3 = (z.real for z in roots)
        edge = mp.sqrt(u3 - up)
        top = mp.sqrt(up)
        pts = [0, edge, top] if edge < top else [0, top]
        half = mp.quad(lambda x: 2 / mp.sqrt((up - x * x - u1) * (u3 - up + x * x)), pts)
        return 2 * half - mp.pi


def far_ray(b, r0=1.0e6):
    """(u0, u0', psi0) of the inward ray of impact parameter b from r0."""
    u0 = 1.0 / r0
    sin_psi = u0 / math.sqrt(1.0 / (b * b) + u0 ** 3)
    return u0, u0 * math.sqrt(1.0 - sin_psi ** 2) / sin_psi, math.asin(sin_psi)


def reference_deflection(b):
    """The reference's total deflection from r = 1e6 to u = 0 (u_f -> 0): the angle
    from V to the exit tangent, phi_exit - (pi - psi0), with the invariant's drift."""
    u0, du0, psi0 = far_ray(b)
    cls, phi, u, du, _, _, (t, y) = G.planar(u0, du0, 0.0, 16.0 * math.pi, path=True)
    assert cls == G.SKY and abs(u) < 1e-12
    e = y[1] ** 2 + y[0] ** 2 - y[0] ** 3
    return phi - math.pi + psi0, float(np.abs(e * b * b - 1.0).max())


@pytest.mark.parametrize("offset", [1e-4, 1e-3, 1e-2, 1e-1, 1.0, 10.0, 100.0])
def test_deflection_is_the_closed_form(offset):
    b = G.B_CRIT * (1.0 + offset)
    got, drift = reference_deflection(b)
    want = float(closed_deflection(b))
    print(f"b/b_crit - 1 = {offset:g}: deflection {got:.12f} closed form {want:.12f} diff {got - want:.2e} drift {drift:.2e}")
    assert abs(got - want) <= 1e-10, (offset, got, want)
    assert drift <= 1e-11, (offset, drift)


@pytest.mark.parametrize("b", [50.0, 100.0, 400.0])
def test_deflection_is_the_weak_field_series(b):
    """tests/test_physics.py's series, to its own remainder: the next term, (3465 pi / 64) m^4, within a tenth."""
    m = 0.5 / b
    series = 4 * m + 15 * math.pi / 4 * m ** 2 + 128.0 / 3.0 * m ** 3
    term = 3465 * math.pi / 64 * m ** 4
    got, _ = reference_deflection(b)
    print(f"b = {b:g}: deflection - series = {got - series:.3e}, next term {term:.3e}")
    assert abs(got - series - term) <= 0.1 * term + 1e-10, (b, got - series, term)


# ---- the set ------------------------------------------------------------------------------
def test_the_set_is_what_the_issue_lists(lens):
    O, V, kind = G.ray_set()
    assert len(O) <= 2048 and (kind == "near-radial").sum() == 64 and (kind == "flat").sum() == 64
    assert np.array_equal(lens.straight, kind == "flat"), "the straight rays are the 64 built to miss"
    r0 = lens.r0[kind == "grid"]
    for r in G.R0:
        k = np.abs(r0 / r - 1.0) < 1e-6
        x = lens.x[kind == "grid"][k]
        admitted = [o for o in G.OFFSETS if G.B_CRIT * (1.0 + o) <= G.b_max(min(r, 1.0 / G.U_F)) * G.MAX_B_SHARE]
        for o in admitted:
            assert (np.abs(x / o - 1.0) < 0.15).sum() >= G.COPIES, (r, o)
    # V is not unit, and every ray is rotated on its own: the orbital planes point everywhere
    n = np.linalg.norm(V.astype(np.float64), axis=-1)
    assert n.min() < 1e-2 and n.max() > 1e2 and np.abs(lens.ref["plane"][~lens.straight].mean(0)).max() < 0.1
    # float32 rounding of a far origin moves b by up to |O| 2^-24 / b: the set's b is the rounded ray's
    assert np.nanmin(np.abs(lens.x)) >= 0.8e-4
    ang = G.angle_between(np.where((np.sum(O * V, -1) < 0)[:, None], -O, O), V)
    assert (ang[kind == "near-radial"] > 1e-3).all()


def test_classification_is_the_analytic_one(lens):
    want = np.array([G.analytic_class(o, v) for o, v in zip(lens.O, lens.V)])
    for rev in G.REVOLUTIONS:
        got = lens.cls(rev)
        ended = got != G.OUT_OF_ANGLE
        assert np.array_equal(got[ended], want[ended]), rev
        print(f"max_revolutions {rev}: {int((~ended).sum())} rays out of angle, {int((got == G.CAPTURED).sum())} captured")
    assert (lens.cls(2) != G.OUT_OF_ANGLE).all() and (lens.cls(1) == G.OUT_OF_ANGLE).sum() > 50
    inside = lens.r0 < 1.5
    assert ((want == G.SKY) & inside & ~lens.straight).sum() > 20 and ((want == G.CAPTURED) & ~inside).sum() > 100


def test_late_rays_are_few(lens):
    """Level C leaves out the rays whose last chord is no tangent; the generator keeps them under 2 %."""
    share = lens.late().sum() / len(lens.O)
    print(f"late rays: {int(lens.late().sum())} of {len(lens.O)}")
    assert share <= G.MAX_LATE_SHARE


def test_golden_file_is_a_fresh_computation(lens):
    pick = np.sort(np.random.default_rng(5).choice(len(lens.O), size=len(lens.O) // 20, replace=False))
    fresh = G.exact_set(lens.O, lens.V, G.U_F, G.REVOLUTIONS, G.RADII, select=pick)
    for key, want in fresh.items():
        got = lens.ref[key][pick]
        if key in ("class", "straight"):
            assert np.array_equal(got, want), key
        elif key in ("s", "s_cross"):  # central differences at a relative 1e-6: a 1e-10 of the angle is 1e-4 of s
            assert np.array_equal(np.isnan(got), np.isnan(want)), key
            assert np.allclose(got, want, rtol=1e-3, atol=1e-4, equal_nan=True), key
        else:
            assert np.array_equal(np.isnan(got), np.isnan(want)), key
            scale = max(G.RADII) if key == "cross" else 1.0
            assert np.nanmax(np.abs(got - want), initial=0.0) <= 1e-10 * scale, key


def test_recorded_tolerances_are_the_measured_ones(lens, tol):
    """lens_tolerances.json's level-C pair is geodesic_reference.fit of the float32 model against the
    golden reference times the margin: measured, not chosen."""
    k = lens.c_sky()
    m32 = lens.model(G.LEVEL_C_STEPS, 2, F)
    assert (m32["class"][k] == G.SKY).all()
    err = G.angle_between(m32["dir"][k], lens.tangent(2)[k])
    for name, g in (("inside", ~lens.beyond[k]), ("beyond", lens.beyond[k])):
        eps, delta = G.fit(err[g], lens.s(2)[k][g])
        rec = tol["level_c"]["dir"][name]
        assert math.isclose(rec["eps_fit"], eps, rel_tol=1e-6) and math.isclose(rec["delta_fit"], delta, rel_tol=1e-6)
        assert rec["eps"] == tol["margin"] * rec["eps_fit"] and rec["delta"] == tol["margin"] * rec["delta_fit"]
    assert tol["margin"] == 4.0 and tol["rays"] == len(lens.O)


# ---- truncation ---------------------------------------------------------------------------
def test_the_float64_model_approaches_the_reference(lens, tol):
    k = lens.c_sky()
    worst = {}
    for n in G.TRUNCATION_STEPS:
        m = lens.model(n, 2, np.float64)
        same = k & (m["class"] == G.SKY)
        worst[n] = G.angle_between(m["dir"][same], lens.tangent(2)[same]).max()
        print(f"{n} steps: max {worst[n]:.3e} rad, {int((k & ~same).sum())} class flips")
        assert math.isclose(tol["level_c"]["truncation_f64_model"][str(n)]["max"], worst[n], rel_tol=1e-6)
    assert all(worst[a] > worst[b] for a, b in zip(G.TRUNCATION_STEPS, G.TRUNCATION_STEPS[1:]))
    m = lens.model(G.LEVEL_C_STEPS, 2, np.float64)
    assert (m["class"][lens.c_rays()] == np.where(lens.cls(2) == G.CAPTURED, G.CAPTURED, G.SKY)[lens.c_rays()]).all()
    err = G.angle_between(m["dir"][k], lens.tangent(2)[k])
    term = G.exit_chord_term(lens.ref["b"][k], lens.ref["du_exit"][k], G.LEVEL_C_STEPS)
    over = err > 1e-5
    print(f"2000 steps: {int(over.sum())} of {int(k.sum())} rays above 1e-5 rad, max {err.max():.3e}; "
          f"their exit-chord bound {term[over].min():.3e} .. {term[over].max():.3e}, b {lens.ref['b'][k][over].min():.1f} .. "
          f"{lens.ref['b'][k][over].max():.1f}")
    assert (err <= np.maximum(1e-5, term)).all()
    assert over.sum() <= 0.05 * k.sum() and (lens.ref["b"][k][over] > 0.8 / G.U_F).all()


# ---- the oracle tie -----------------------------------------------------------------------
def ramp_sky():
    """SKY_W x SKY_H texels of pairwise distinct colours (x, y, (x + w / 2) mod w): the library has no
    nearest filter, and of this sky the bilinear sample is the sample's own position, so the texel whose
    centre is nearest (the one floor(u w), floor(v h) names) is read off the float FragColor: its column from
    the red channel, or from the blue one where red blends across the seam, its row from the green one."""
    sky = np.zeros((SKY_H, SKY_W, 3), dtype=np.uint8)
    sky[..., 0] = np.arange(SKY_W, dtype=np.uint8)[None, :]
    sky[..., 1] = np.arange(SKY_H, dtype=np.uint8)[:, None]
    sky[..., 2] = (sky[..., 0] + SKY_W // 2) % SKY_W
    return sky


def ray_tolerance(lens, tol, rev=2):
    t = tol["level_c"]["dir"]
    s = np.where(lens.straight, 0.0, lens.s(rev))
    return np.where(lens.beyond, t["beyond"]["eps"] + t["beyond"]["delta"] * s, t["inside"]["eps"] + t["inside"]["delta"] * s)


def test_oracle_frames_are_the_reference_at_texel_resolution(pkg, oracle, lens, tol):
    import trace_cases as T

    params = pkg.abi.default_params(max_steps=G.LEVEL_C_STEPS, max_revolutions=2, u_f=G.U_F, percent_black=-1.0,
                                    crosshair=0, filter_mode=pkg.abi.FILTER_LERP)
    _, f, _ = T.ray_frames(pkg, oracle, pkg.scenes.scene_black_hole_only(), lens.O, lens.V, params,
                           oracle.TextureSet(ramp_sky(), None), None)
    rays = lens.c_rays() | lens.straight
    captured = rays & (lens.cls(2) == G.CAPTURED)
    assert (f[captured] == np.array([0, 0, 0, 1], dtype=F)).all()
    sky = rays & ~captured
    uv = np.stack([pkg.abi.sky_uv(d) for d in lens.tangent(2)[sky].astype(F)]).astype(np.float64)
    X, Y = uv[:, 0] * SKY_W, uv[:, 1] * SKY_H
    cos_lat = np.sqrt(np.maximum(0.0, 1.0 - lens.tangent(2)[sky][:, 1] ** 2))
    fx, fy = X - np.floor(X), Y - np.floor(Y)
    to_border = np.minimum(np.minimum(fx, 1.0 - fx) * (2.0 * math.pi / SKY_W) * cos_lat,
                           np.minimum(fy, 1.0 - fy) * (math.pi / SKY_H))
    t = ray_tolerance(lens, tol)[sky]
    # the green channel blends across the poles (the last row and the first): left out with the border rays
    edge = np.minimum(Y, SKY_H - Y) <= 0.5 + t / (math.pi / SKY_H)
    out = (to_border <= t) | edge
    print(f"{int(out.sum())} of {int(sky.sum())} sky rays within their tolerance of a texel border")
    assert out.mean() <= MAX_BORDER_SHARE
    c = f[sky].astype(np.float64) * 255.0
    seam = np.minimum(X, SKY_W - X) < 2.0
    got = np.stack([np.where(seam, (np.floor(c[:, 2] + 0.5) - SKY_W // 2) % SKY_W, np.floor(c[:, 0] + 0.5)),
                    np.floor(c[:, 1] + 0.5)], axis=-1)
    want = np.stack([np.floor(X), np.floor(Y)], axis=-1)
    bad = (got != want).any(-1) & ~out
    assert not bad.any(), (int(bad.sum()), np.flatnonzero(sky)[bad][:5].tolist(), got[bad][:5], want[bad][:5])
    assert (f[sky][:, 3] == 1).all()


@pytest.mark.parametrize("j", range(len(G.RADII)))
def test_oracle_frames_of_a_concentric_sphere_are_its_colour(pkg, oracle, lens, j):
    """The finite-radius rays of tests/test_gpu_lens_physics.py on the oracle alone: every ray whose geodesic
    reaches r = R ends on the sphere, every captured one in the hole; the steep rays the scheme may fling past
    a surface (Lens.flung) are few and left out."""
    import trace_cases as T

    color = (0.25, 0.5, 0.75, 1.0)
    params = pkg.abi.default_params(max_steps=G.LEVEL_C_STEPS, max_revolutions=2, u_f=G.U_F, percent_black=-1.0,
                                    crosshair=0)
    k = lens.within_radius(j) & ~lens.flung(j)
    _, f, _ = T.ray_frames(pkg, oracle, G.sphere_scene(pkg, G.RADII[j], color), lens.O[k], lens.V[k], params,
                           oracle.TextureSet(ramp_sky(), None), None)
    hit = lens.inside_radius(j)[k]
    assert hit.sum() > 200 and (lens.cls(2)[k][~hit] == G.CAPTURED).all()
    assert (f[hit] == np.array(color, dtype=F)).all()
    assert (f[~hit] == np.array([0, 0, 0, 1], dtype=F)).all()
    flung = lens.within_radius(j) & lens.flung(j)
    print(f"R = {G.RADII[j]:g}: {int(hit.sum())} rays, {int(flung.sum())} left out as steep")
    assert flung.sum() <= 0.25 * lens.within_radius(j).sum()  # (the steepest grid rays and most near-radial ones)
    m = lens.model(G.LEVEL_C_STEPS, 2, np.float64, G.RADII[j])
    assert (m["class"][k] == np.where(hit, G.SURFACE, G.CAPTURED)).all()
