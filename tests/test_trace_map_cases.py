"""tests/trace_map_cases.py held to the oracle alone (no GPU), and the
rejections of sr_trace_ray_maps that need no device.

tests/test_ray_map_cases.py shows the two numpy statements of
tests/ray_map_cases.py on frames whose rays all start at one camera position.
Here the rays have origins of their own, each a 1x1 oracle frame
(tests/trace_cases.py ray_frames): the statements still give the oracle's
float FragColor bit for bit and still notice one ulp of every input, so that
tests/test_gpu_trace_maps.py, which feeds them the GPU's maps of such rays,
checks those maps to the last bit. The scattered sets that module runs hold
enough rays of each class the statements apply to.
"""
import ctypes as C

import numpy as np
import pytest

import pick_cases as K
import ray_map_cases as R
import trace_cases as T
import trace_map_cases as M

F = np.float32


@pytest.fixture(scope="module")
def probes(pkg, oracle):
    """Per case: the rigged scene, its probe rays, their 1x1 oracle frames under the random sky and their hits."""
    sky = R.random_sky()
    tex = oracle.TextureSet(sky, None)
    prm = pkg.abi.default_params(max_steps=10, percent_black=-1.0, crosshair=0, raytrace_type=1)
    out = {}
    for name, scene in R.cpu_cases(pkg).items():
        O, V = M.probe_rays(scene)
        assert len(O) == M.N_ORIGINS * M.N_DIRS == 480
        length = np.sqrt((V.astype(np.float64) ** 2).sum(-1))
        assert length.min() < 0.5 and length.max() > 2.0 and (np.abs(length - 1.0) > 1e-3).mean() > 0.95
        assert len(np.unique(O, axis=0)) == M.N_ORIGINS
        _, f32, steps = T.ray_frames(pkg, oracle, scene, O, V, prm, tex, None)
        assert (steps == 0).all()
        rd = M.start_dirs(V)  # frag:863 on the 1x1 frame: rd = normalize(+0 + V)
        chords = np.concatenate([O, rd, np.full((len(O), 1), -1.0, dtype=F)], axis=1)
        winner, _, point, _ = oracle.intersect(scene, chords)
        out[name] = {"scene": scene, "f32": f32, "dir": rd, "winner": winner, "point": point, "sky": sky,
                     "mode": int(prm.filter_mode)}
    return out


def lit(case):
    """(ray indices, ids, point, normal, view, base) of the rays whose winner is an object."""
    scene, winner = case["scene"], case["winner"]
    k = np.flatnonzero(winner >= 0)
    ids = winner[k]
    point = case["point"][k]
    normal = np.zeros_like(point)
    base = np.zeros((len(k), 4), dtype=F)
    for obj in np.unique(ids):
        sel = ids == obj
        normal[sel] = R.geometric_normal(scene, int(obj), point[sel])
        base[sel] = np.array(list(scene.materials[scene.objects[int(obj)].material_index].color), dtype=F)
    assert (base[:, 3] == 1.0).all()
    return k, ids, point, normal, -case["dir"][k], base


def shade(scene, ids, point, normal, view, base):
    out = np.zeros((len(ids), 3), dtype=F)
    for obj in np.unique(ids):
        sel = ids == obj
        out[sel] = R.deferred_np(scene, int(obj), point[sel], normal[sel], view[sel], base[sel])
    return out


def sample(oracle, case, uv):
    return np.stack([oracle.sample_texture(case["sky"], u, v, case["mode"]) for u, v in uv])


def test_probe_rays_hold_sky_and_hits(oracle, probes):
    for name, c in probes.items():
        n = len(c["winner"])
        sky, hit = int((c["winner"] == oracle.HIT_NONE).sum()), int((c["winner"] >= 0).sum())
        print(f"MEASURED {name}: sky {sky / n:.3f} object hits {hit / n:.3f} of {n} rays")
        assert sky >= R.MIN_SKY_SHARE * n and hit >= R.MIN_HIT_SHARE * n, name


def test_sky_statement_on_rays_with_their_own_origins(oracle, probes):
    for name, c in probes.items():
        k = np.flatnonzero(c["winner"] == oracle.HIT_NONE)
        uv = R.sky_uv_np(c["dir"][k])
        ok = R.same_bits(sample(oracle, c, uv), c["f32"][k]).all(-1)
        assert ok.all(), f"{name}: {int((~ok).sum())} of {len(k)} sky rays differ"


def test_lighting_statement_on_rays_with_their_own_origins(probes):
    for name, c in probes.items():
        k, ids, point, normal, view, base = lit(c)
        want = c["f32"][k]
        got = shade(c["scene"], ids, point, normal, view, base)
        ok = R.same_bits(got, want[:, :3]).all(-1) & (want[:, 3] == 1.0)
        assert ok.all(), f"{name}: {int((~ok).sum())} of {len(k)} lit rays differ"
        shares = {}
        for label, arr in (("p", point), ("n", normal), ("v", view)):
            for axis in range(3):
                moved = arr.copy()
                moved[:, axis] = R.ulp_up(moved[:, axis])
                args = {"p": point, "n": normal, "v": view, label: moved}
                changed = ~R.same_bits(shade(c["scene"], ids, args["p"], args["n"], args["v"], base), want[:, :3]).all(-1)
                shares[label + "xyz"[axis]] = (int(changed.sum()), float(changed.mean()))
        print(f"MEASURED {name}: one ulp changes, of {len(k)} lit rays: " +
              " ".join(f"{key} {share:.3f}" for key, (_, share) in shares.items()))
        for key, (count, share) in shares.items():
            assert share >= R.MIN_LIT_SENSITIVE and count >= R.MIN_LIT_PIXELS, (name, key, count, share)


@pytest.mark.parametrize("key,overlay", T.SCATTERED)
def test_scattered_sets_carry_each_class(pkg, oracle, textures, key, overlay):
    """Among the finite rays of a scattered set under the rig: pure-sky rays (the sky statement's), rays whose
    first surface is opaque (the lighting statement's) and rays that end in the sky by check_end's rule. The codes
    and the translucent crossings are trace_cases' own, of the unrigged scene: the rig changes shading fields only."""
    tm = M.TraceMaps(pkg, oracle, textures)
    O, V, _ = tm.rays(key)
    fin = T.finite_rays(O, V)
    n = int(fin.sum())
    codes, ok = tm.tr.scattered_codes(key, overlay)
    cross = tm.tr.translucent_crossings(key, overlay)
    use = fin & ok & ~cross
    shares = {"pure sky": float((use & (codes == K.SKY)).sum()) / n,
              "opaque first": float((use & (codes >= 0)).sum()) / n,
              "ends in the sky": float((fin & tm.ends_in_sky(key, overlay)).sum()) / n}
    print(f"MEASURED {key} overlay={overlay}: of {n} finite rays " + " ".join(f"{k} {v:.3f}" for k, v in shares.items()))
    assert shares["pure sky"] >= R.MIN_SKY_SHARE, shares
    assert shares["opaque first"] >= R.MIN_HIT_SHARE, shares
    assert shares["ends in the sky"] >= M.MIN_END_SKY_SHARE, shares


def test_abi_rejections_without_a_device(pkg):
    """The symbol with sr.h's prototype; a null context, null params and null maps are SR_E_INVALID before
    anything of the context is read (the stand-in context below is never dereferenced)."""
    abi = pkg.abi
    lib = abi.load()
    fn = lib.sr_trace_ray_maps
    assert abi.SIGNATURES["sr_trace_ray_maps"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                             C.POINTER(abi.Params), C.POINTER(abi.RayMapPtrs),
                                                             C.c_void_p])
    assert fn.restype is C.c_int and list(fn.argtypes) == abi.SIGNATURES["sr_trace_ray_maps"][1]
    prm, maps = abi.default_params(), abi.RayMapPtrs()
    rays = np.zeros((4, 3), dtype=F)
    end = np.full(4, -77, dtype=np.int32)
    maps.end = end.ctypes.data
    stand_in = C.create_string_buffer(64)
    o = d = rays.ctypes.data
    assert fn(None, o, d, 4, C.byref(prm), C.byref(maps), None) == abi.SR_E_INVALID
    assert fn(None, None, None, 0, C.byref(prm), C.byref(maps), None) == abi.SR_E_INVALID
    assert fn(C.addressof(stand_in), o, d, 4, None, C.byref(maps), None) == abi.SR_E_INVALID
    assert fn(C.addressof(stand_in), o, d, 4, C.byref(prm), None, None) == abi.SR_E_INVALID
    assert (end == -77).all() and stand_in.raw == bytes(64)
