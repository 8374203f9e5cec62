"""The lens map of sr_trace_ray_maps against binary64 Schwarzschild geodesics.

Every other GPU test holds the kernels to the CPU oracle bit for bit; this one
holds what they compute to the physics, through tests/geodesic_reference.py
(shown trustworthy on the CPU by tests/test_geodesic_reference.py) and the
recorded reference of tests/golden/lens_reference.npz:

  level C   the kernel against the exact geodesic at 2000 steps: class, exit
            direction within eps + delta s, the bend in the orbital plane, a
            unit sky_dir;
  level B   the kernel against the float64 model of the scheme at the same
            step count (64, 256, 2000 steps, 1, 2 and 4 revolutions): rounding
            only, whatever the truncation;
  finite    hit_point, hit_view and id on a sphere about the hole, against the
            geodesic's first crossing of its radius;
  flat      rays that miss the r = 1 / u_f sphere from outside keep
            normalize(V), bit for bit.

The tolerances are those of tests/golden/lens_tolerances.json, measured on
the float32 model, never on the kernel (tests/golden/make_lens_reference.py).
Every launch: at most 2048 rays and 2000 steps, with culling on and off.
"""
import numpy as np
import pytest

import geodesic_reference as G
import pick_cases as K
import ray_map_cases as R

pytestmark = pytest.mark.gpu

F = np.float32
ULP = float(np.spacing(F(1.0)))
CULL = (True, False)
_LAUNCHES = {}


@pytest.fixture(scope="module")
def lens():
    return G.Lens.load()


@pytest.fixture(scope="module")
def tol():
    return G.Lens.tolerances()


@pytest.fixture(scope="module")
def gpu(pkg):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    r = pkg.Renderer(0)
    yield r
    r.close()


def traced(gpu, pkg, lens, key, steps, rev, cull, which, select=None):
    """Renderer.trace_ray_maps of the set (or its rays `select`) in the hole-only scene (key None) or with
    the sphere of radius key -> {map: host array}; one launch per distinct call of the session."""
    import torch

    k = (key, steps, rev, cull, which)
    if k not in _LAUNCHES:
        assert steps <= 2000
        scene = pkg.scenes.scene_black_hole_only() if key is None else G.sphere_scene(pkg, key)
        gpu.set_culling(cull)
        gpu.set_projection("rectilinear")
        gpu.set_split(0)
        gpu.set_latency_mode(False)
        gpu.set_scene(scene)
        gpu.set_test_ray(pkg.abi.default_test_ray())
        params = pkg.abi.default_params(max_steps=steps, max_revolutions=rev, u_f=G.U_F, percent_black=-1.0, crosshair=0)
        O, V = (lens.O, lens.V) if select is None else (lens.O[select], lens.V[select])
        assert len(O) <= 2048
        dev = [torch.from_numpy(np.array(a, dtype=F, order="C")).cuda() for a in (O, V)]
        got = gpu.trace_ray_maps(dev[0], dev[1], params, which)
        torch.cuda.synchronize()
        _LAUNCHES[k] = {m: (v.cpu().numpy()[..., 0] if m in ("end", "id") else v.cpu().numpy()) for m, v in got.items()}
    return _LAUNCHES[k]


def pair_tolerance(pairs, beyond, s):
    """eps + delta s with the pair of the ray's origin (inside or beyond r = 1 / u_f)."""
    return np.where(beyond, pairs["beyond"]["eps"] + pairs["beyond"]["delta"] * s,
                    pairs["inside"]["eps"] + pairs["inside"]["delta"] * s)


def check(ok, label, values=None):
    bad = np.flatnonzero(~ok)
    detail = "" if values is None or not len(bad) else f", worst {np.asarray(values)[bad].max():.3e}"
    assert not len(bad), f"{label}: {len(bad)} of {len(ok)} rays, first {bad[:5].tolist()}{detail}"


def check_directions(lens, d, k, plane_tol, label):
    """On rays k (sky rays that are not straight): the bend lies in the orbital plane, sky_dir is unit."""
    d = d[k].astype(np.float64)
    off = np.abs(np.sum(d * lens.ref["plane"][k], axis=-1))
    print(f"{label}: out of plane max {off.max():.3e} (tolerance {plane_tol:.3e}), "
          f"| |sky_dir| - 1 | max {np.abs(np.linalg.norm(d, axis=-1) - 1.0).max():.3e}")
    check(off <= plane_tol, f"{label}: out of the orbital plane", off)
    check(np.abs(np.linalg.norm(d, axis=-1) - 1.0) <= 4 * ULP, f"{label}: |sky_dir| is not 1 within 4 ulp")


def report(label, err, s, x):
    """The table of DESIGN.md "Lens-map accuracy": printed, asserted nowhere."""
    print(f"{label}: error against the exact geodesic by |b / b_crit - 1|: rays, max rad, median rad, "
          "max and median as delta b / b")
    for row in G.error_table(err, s, x):
        print("   %-9s %4d  %.2e  %.2e  %.2e  %.2e" % row)


# ---- level C ------------------------------------------------------------------------------
@pytest.mark.parametrize("cull", CULL)
def test_level_c_kernel_against_the_exact_geodesic(gpu, pkg, lens, tol, cull):
    m = traced(gpu, pkg, lens, None, G.LEVEL_C_STEPS, 2, cull, ("end", "id", "sky_dir"))
    rays = lens.c_rays()
    captured = lens.cls(2) == G.CAPTURED
    check((m["end"] == np.where(captured, R.END_OPAQUE, R.END_SKY))[rays], "level C: end flips")
    check((m["id"] == np.where(captured, K.HOLE, K.SKY))[rays], "level C: id flips")
    k = lens.c_sky()
    err = G.angle_between(m["sky_dir"][k], lens.tangent(2)[k])
    t = pair_tolerance(tol["level_c"]["dir"], lens.beyond[k], lens.s(2)[k])
    report(f"level C, {G.LEVEL_C_STEPS} steps, culling {cull}", err, lens.s(2)[k], lens.x[k])
    print(f"   worst share of the tolerance {np.max(err / t):.3f}")
    check(err <= t, "level C: sky_dir off the exact tangent", err / t)
    check_directions(lens, m["sky_dir"], k, tol["level_c"]["plane"]["tol"], "level C")


# ---- level B ------------------------------------------------------------------------------
@pytest.mark.parametrize("cull", CULL)
@pytest.mark.parametrize("rev", G.REVOLUTIONS)
@pytest.mark.parametrize("steps", G.LEVEL_B_STEPS)
def test_level_b_kernel_against_the_float64_model(gpu, pkg, lens, tol, steps, rev, cull):
    """64 steps of 2 pi rev / 64 >= 0.098 rad: at rev 2 and 4 above the 0.1 rad at which a trace launch stops
    culling, 256 steps below it at every rev."""
    m = traced(gpu, pkg, lens, None, steps, rev, cull, ("end", "id", "sky_dir"))
    m64 = lens.model(steps, rev, np.float64)
    label = f"level B, {steps} steps, {rev} revolutions, culling {cull}"
    allowed = lens.model_flips(rev, m64)
    sky = G.ends_in_sky(m64["class"])
    print(f"{label}: the float64 model's class differs from the exact one on {int(allowed.sum())} rays")
    assert allowed.sum() == tol["level_b"][str(steps)]["f64_model_class_differs_from_exact"][str(rev)]
    check(((m["end"] == R.END_SKY) == sky) | allowed, f"{label}: end flips")
    check((m["id"] == np.where(sky, K.SKY, K.HOLE)) | allowed, f"{label}: id flips")
    k = lens.level_b(rev, m64) & (m["end"] == R.END_SKY)
    err = G.angle_between(m["sky_dir"][k], m64["dir"][k])
    t = pair_tolerance(tol["level_b"][str(steps)]["dir"], lens.beyond[k], lens.s(rev)[k])
    print(f"{label}: {int(k.sum())} directions, worst share of the tolerance {np.max(err / t):.3f}")
    check(err <= t, f"{label}: sky_dir off the model's", err / t)
    check_directions(lens, m["sky_dir"], (m["end"] == R.END_SKY) & ~lens.straight,
                     tol["level_b"][str(steps)]["plane"]["tol"], label)
    if rev == 2 and cull:
        e = lens.c_sky() & (m["end"] == R.END_SKY)
        report(label, G.angle_between(m["sky_dir"][e], lens.tangent(2)[e]), lens.s(2)[e], lens.x[e])


# ---- finite radius ------------------------------------------------------------------------
@pytest.mark.parametrize("cull", CULL)
@pytest.mark.parametrize("j", range(len(G.RADII)))
def test_hits_on_a_concentric_sphere(gpu, pkg, lens, tol, j, cull):
    radius = G.RADII[j]
    sel = lens.within_radius(j) & ~lens.flung(j)
    m = traced(gpu, pkg, lens, radius, G.LEVEL_C_STEPS, 2, cull, ("end", "id", "hit_point", "hit_view"), sel)
    hit = lens.inside_radius(j)[sel]
    label = f"R = {radius:g}, culling {cull}"
    check(m["id"] == np.where(hit, 0, K.HOLE), f"{label}: id is not the sphere's (object 0) or the hole's")
    check(m["end"] == R.END_OPAQUE, f"{label}: end")
    rec = tol["finite_radius"][str(int(radius))]
    s = lens.ref["s_cross"][sel, j][hit]
    p = m["hit_point"][hit].astype(np.float64)
    err = G.angle_between(p, lens.ref["cross"][sel, j][hit])
    t = rec["angle"]["eps"] + rec["angle"]["delta"] * s
    off = np.abs(np.linalg.norm(p, axis=-1) - radius)
    m64 = lens.model(G.LEVEL_C_STEPS, 2, np.float64, radius)
    view = G.angle_between(m["hit_view"][hit], m64["hit_view"][sel][hit])
    tv = rec["view"]["eps"] + rec["view"]["delta"] * s
    print(f"{label}: {int(hit.sum())} hits, hit_point off the crossing max {err.max():.3e} rad (worst share of the "
          f"tolerance {np.max(err / t):.3f}), | |hit_point| - R | max {off.max():.3e} (tolerance {rec['radius']['tol']:.3e}), "
          f"hit_view off the model's chord max {view.max():.3e} rad (worst share {np.max(view / tv):.3f})")
    check(err <= t, f"{label}: hit_point off the geodesic's first crossing", err / t)
    check(off <= rec["radius"]["tol"], f"{label}: |hit_point| is not R", off)
    check(view <= tv, f"{label}: hit_view is not minus the model's chord", view / tv)


# ---- flat rays ----------------------------------------------------------------------------
@pytest.mark.parametrize("cull", CULL)
def test_rays_that_miss_the_curved_region_keep_their_direction(gpu, pkg, lens, cull):
    m = traced(gpu, pkg, lens, None, G.LEVEL_C_STEPS, 2, cull, ("end", "id", "sky_dir"))
    k = lens.straight
    assert k.sum() == G.N_FLAT
    want = R.norm3(np.zeros(3, dtype=F) + lens.V[k])  # normalize(+0 + V) in binary32 (sr.h "Ray maps of ray queries")
    assert (m["end"][k] == R.END_SKY).all() and (m["id"][k] == K.SKY).all()
    assert R.same_bits(m["sky_dir"][k], want).all()
