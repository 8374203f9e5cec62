"""tests/trace_cases.py on the oracle alone (no GPU): the scattered ray sets are
not degenerate, the camera-ray method reproduces the oracle's own frame, and
sr_camera_rays equals its numpy statement bit for bit."""
import numpy as np
import pytest

import pick_cases as K
import projection_cases as P
import trace_cases as T


@pytest.fixture(scope="module")
def tr(pkg, oracle, textures):
    return T.Traces(pkg, oracle, textures)


def test_scattered_sets_hold_the_listed_origins_and_directions(tr):
    for key in ("default", "large"):
        O, V, labels = tr.rays(key)
        assert 550 <= len(O) <= 700 and O.dtype == np.float32 and V.dtype == np.float32
        r = np.sqrt((O.astype(np.float64) ** 2).sum(-1))
        names = {lab.split("/")[0] for lab in labels}
        for want in ("r=1", "r=0.5", "centre", "r=100", "r=100-", "r=100+", "r=150", "r=1e5", "r=1e25", "on-sphere",
                     "in-sphere", "rect-", "rect+", "in-box", "nan", "+inf", "-inf"):
            assert want in names, want
        kinds = {lab.split("/")[1].rstrip("0123456789") for lab in labels}
        assert kinds >= {"obj", "hole", "sky", "radial-in", "radial-out", "near-in", "near-out", "graze-out", "tangent", "zero", "tiny", "huge", "-0a",
                         "-0b", "nan"}
        assert (r == 1.0).any() and (r == 100.0).any() and (r == 0.0).any()
        y = O[[i for i, lab in enumerate(labels) if lab.startswith("r=100")], 1]
        assert set(np.unique(y)) == {np.nextafter(np.float32(100), np.float32(0)), np.float32(100),
                                     np.nextafter(np.float32(100), np.float32(200))}
        assert (np.signbit(V) & (V == 0)).any() and np.isnan(V).any() and np.isnan(O).any() and np.isinf(O).any()
        fin = T.finite_rays(O, V)
        assert 0.6 * len(O) < fin.sum() < len(O)


@pytest.mark.parametrize("key,overlay", T.SCATTERED)
def test_scattered_sets_are_not_degenerate(tr, key, overlay):
    """Among the finite rays every class holds 5 %, 5 % cross a translucent
    surface, and at least 20 rays depend on their origin."""
    O, V, labels = tr.rays(key)
    fin = T.finite_rays(O, V)
    _, _, steps = tr.scattered_ref(key, overlay)
    codes, ok = tr.scattered_codes(key, overlay)
    # the recoloured scene has the original's geometry: the same steps unless a translucent surface was crossed
    assert ok[fin].mean() > 0.97, f"{(~ok[fin]).sum()} finite rays do not decode to one code"
    n = int(fin.sum())
    radius = np.sqrt((O.astype(np.float64) ** 2).sum(-1))
    shares = {k: float(v[fin & ok].sum()) / n for k, v in T.classify(codes, steps, T.STEPS, radius).items()}
    print(key, overlay, n, shares)
    for k, v in shares.items():
        assert v >= T.MIN_SHARE, (k, shares)
    cross = tr.translucent_crossings(key, overlay)
    assert cross[fin].sum() / n >= T.MIN_SHARE, cross[fin].sum() / n
    dep = tr.origin_dependent(key, overlay)
    assert int(dep[fin].sum()) >= T.MIN_ORIGIN_DEPENDENT
    if overlay:
        assert np.isin(codes[fin & ok], (K.TR_FLAT, K.TR_CURVED)).any(), "no ray of the set meets the overlay"


@pytest.mark.parametrize("key", ("default", "large"))
def test_flat_sets_differ_from_curved(tr, key):
    b0, _, s0 = tr.scattered_ref(key, False)
    b1, _, s1 = tr.scattered_ref(key, False, T.FLAT)
    fin = T.finite_rays(*tr.rays(key)[:2])
    assert (s1 == 0).all()
    assert ((b0 != b1).any(-1) & fin).sum() > 0.2 * fin.sum()


def test_ray_frames_of_camera_rays_are_the_oracles_frame(tr):
    """The method on a fixed camera: the 1x1 frames of a 17x11 view's camera
    rays are the oracle's 17x11 frame (default scene, overlay on)."""
    w, h = 17, 11
    cam = tr.wd.cams["view"]
    O, V = T.camera_rays_numpy(cam, P.RECTILINEAR, w, h)
    assert not (np.signbit(V) & (V == 0)).any()
    got = T.ray_frames(tr.pkg, tr.oracle, tr.wd.scene("small"), O.reshape(-1, 3), V.reshape(-1, 3), tr.params(), tr.tex,
                       tr.wd.test_rays[True])
    want = tr.wd.ref("small", True, w=w, h=h)
    assert np.array_equal(got[0].reshape(h, w, 4), want[0])
    assert np.array_equal(got[1].reshape(h, w, 4).view(np.uint32), want[1].view(np.uint32))
    assert np.array_equal(got[2].reshape(h, w), want[2])


@pytest.mark.parametrize("projection,w,h,fov", [
    (P.RECTILINEAR, 33, 17, None), (P.RECTILINEAR, 68, 44, 60.0), (P.RECTILINEAR, 1, 1, None),
    (P.EQUIRECT, 33, 17, None), (P.EQUIRECT, 64, 32, 360.0),
    (P.FISHEYE, 33, 17, None), (P.FISHEYE, 41, 41, 180.0), (P.FISHEYE, 48, 48, 360.0),
])
def test_camera_rays_equal_the_numpy_statement(pkg, tr, projection, w, h, fov):
    """sr_camera_rays against projection_cases.local_dirs and world_dirs, bit
    for bit; the fisheye's pixels without a ray have NaN directions."""
    for name in ("view", "fly1"):
        cam = P.with_fov(pkg, tr.wd.cams[name], fov)
        O, V = pkg.camera_rays(cam, projection, w, h)
        wo, wv = T.camera_rays_numpy(cam, projection, w, h)
        assert O.shape == V.shape == (h, w, 3) and O.dtype == V.dtype == np.float32
        assert np.array_equal(O.view(np.uint32), wo.view(np.uint32))
        _, ray = P.local_dirs(projection, cam.fov, w, h)
        assert np.array_equal(np.isnan(V).all(-1), ~ray) and np.array_equal(np.isnan(V).any(-1), ~ray)
        assert np.array_equal(V[ray].view(np.uint32), wv[ray].view(np.uint32))
        if (projection, fov) == (P.FISHEYE, 360.0):
            assert (~ray).any() and ray.any()
    # a band of rows is the same rows of the whole frame
    cam = tr.wd.cams["view"]
    Ob, Vb = pkg.abi.camera_rays(cam, projection, w, h, h // 3, h)
    O, V = pkg.abi.camera_rays(cam, projection, w, h)
    assert np.array_equal(Vb.view(np.uint32), V[h // 3:].view(np.uint32)) and np.array_equal(Ob, O[h // 3:])


def test_camera_rays_rejections(pkg):
    import ctypes as C

    abi = pkg.abi
    lib = abi.load()
    cam = abi.default_camera()
    buf = np.zeros((4, 4, 3), dtype=np.float32)
    o, d = buf.ctypes.data, buf.copy().ctypes.data
    ok = (C.byref(cam), 0, 4, 4, 0, 4, o, d)
    assert lib.sr_camera_rays(*ok) == abi.SR_OK
    for i, bad in ((0, None), (1, 3), (1, -1), (2, 0), (3, 0), (4, -1), (5, 5), (4, 3), (6, None), (7, None),
                   (2, 2 ** 30)):
        args = list(ok)
        args[i] = bad
        if (i, bad) == (4, 3):
            args[5] = 2  # row_begin > row_end
        assert lib.sr_camera_rays(*args) == abi.SR_E_INVALID, (i, bad)
