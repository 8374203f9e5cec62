"""tests/ray_map_cases.py held to the oracle alone (no GPU): the two numpy
statements reproduce the oracle's float FragColor bit for bit on flat-mode
frames, and those frames notice one ulp of every input of either statement,
so that tests/test_gpu_ray_maps.py, which feeds the statements the GPU's maps,
checks the maps to the last bit.

Flat mode: a pixel's ray is abi.camera_rays' normalised ray, its hit
oracle.intersect's, its view direction the ray's negative; the geometric
normals of the sphere and the rectangle are stated in numpy.
"""
import numpy as np
import pytest

import ray_map_cases as R

F = np.float32
W, H = R.W, R.H


@pytest.fixture(scope="module")
def frames(pkg, oracle):
    """Per case: the rigged scene, the oracle's float frame under the random sky, the rays and the hits."""
    abi = pkg.abi
    sky = R.random_sky()
    tex = oracle.TextureSet(sky, None)
    cam = R.camera(pkg)
    prm = abi.default_params(max_steps=10, percent_black=-1.0, crosshair=0, raytrace_type=1)
    o, d = abi.camera_rays(cam, "rectilinear", W, H)
    d = R.norm3(d)  # frag:863: rd = normalize(axes * L)
    chords = np.concatenate([o.reshape(-1, 3), d.reshape(-1, 3), np.full((W * H, 1), -1.0, dtype=F)], axis=1)
    out = {}
    for name, scene in R.cpu_cases(pkg).items():
        _, f32, _ = oracle.render(scene, cam, prm, W, H, tex)
        winner, _, point, _ = oracle.intersect(scene, chords)
        out[name] = {"scene": scene, "f32": f32.reshape(-1, 4), "dir": d.reshape(-1, 3), "winner": winner,
                     "point": point, "sky": sky, "mode": int(prm.filter_mode)}
    return out


def lit(case):
    """(pixel indices, ids, point, normal, view, base) of the opaque first hits."""
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


def test_frames_hold_sky_and_hits(frames):
    for name, c in frames.items():
        n = W * H
        sky, hit = int((c["winner"] == -100).sum()), int((c["winner"] >= 0).sum())
        print(f"MEASURED {name}: sky {sky / n:.3f} opaque first hits {hit / n:.3f} of {n} pixels")
        assert sky >= R.MIN_SKY_SHARE * n and hit >= R.MIN_HIT_SHARE * n, name


def test_sky_statement(oracle, frames):
    for name, c in frames.items():
        k = np.flatnonzero(c["winner"] == -100)  # oracle.HIT_NONE: pure sky
        uv = R.sky_uv_np(c["dir"][k])
        want = c["f32"][k]
        got = sample(oracle, c, uv)
        ok = R.same_bits(got, want).all(-1)
        assert ok.all(), f"{name}: {int((~ok).sum())} of {len(k)} sky pixels differ"
        shares = {}
        for axis, label in ((0, "u"), (1, "v")):
            moved = uv.copy()
            moved[:, axis] = R.ulp_up(moved[:, axis])
            shares[label] = float((~R.same_bits(sample(oracle, c, moved), want).all(-1)).mean())
        print(f"MEASURED {name}: one ulp of u changes {shares['u']:.3f}, of v {shares['v']:.3f} of {len(k)} sky pixels")
        assert min(shares.values()) >= R.MIN_UV_SENSITIVE, (name, shares)


def test_lighting_statement(frames):
    for name, c in frames.items():
        k, ids, point, normal, view, base = lit(c)
        want = c["f32"][k]
        got = shade(c["scene"], ids, point, normal, view, base)
        ok = R.same_bits(got, want[:, :3]).all(-1) & (want[:, 3] == 1.0)
        assert ok.all(), f"{name}: {int((~ok).sum())} of {len(k)} opaque-hit pixels differ"
        shares = {}
        for label, arr in (("p", point), ("n", normal), ("v", view)):
            for axis in range(3):
                moved = arr.copy()
                moved[:, axis] = R.ulp_up(moved[:, axis])
                args = {"p": point, "n": normal, "v": view, label: moved}
                changed = ~R.same_bits(shade(c["scene"], ids, args["p"], args["n"], args["v"], base), want[:, :3]).all(-1)
                shares[label + "xyz"[axis]] = (int(changed.sum()), float(changed.mean()))
        print(f"MEASURED {name}: one ulp changes, of {len(k)} opaque-hit pixels: " +
              " ".join(f"{key} {share:.3f}" for key, (_, share) in shares.items()))
        for key, (count, share) in shares.items():
            assert share >= R.MIN_LIT_SENSITIVE and count >= R.MIN_LIT_PIXELS, (name, key, count, share)
