"""tests/projection_cases.py on the oracle alone (no GPU): the per-pixel method
reproduces the oracle's own frames, and the cases show what they claim.
"""
import numpy as np
import pytest

import projection_cases as P


@pytest.fixture(scope="module")
def pj(pkg, oracle, textures):
    return P.Projected(pkg, oracle, textures)


@pytest.mark.parametrize("key", ["small", "large"])
def test_method_reproduces_the_oracles_own_frames(pj, key):
    """The rectilinear L through 1x1 frames == the oracle's 33x17 frame: RGBA8,
    float FragColor bits (NaN == NaN) and steps, every pixel."""
    w, h = 33, 17
    b, f, s = pj.ref(key, False, P.RECTILINEAR, w, h)
    rb, rf, rs = pj.wd.ref(key, False, "view", w, h, P.STEPS)
    fbits = (f.view(np.uint32) != rf.view(np.uint32)).any(-1) & ~(np.isnan(f).any(-1) & np.isnan(rf).any(-1))
    assert not (b != rb).any() and not fbits.any() and np.array_equal(s, rs), (
        int((b != rb).any(-1).sum()), int(fbits.sum()), int((s != rs).sum()))
    assert (s > 0).mean() > 0.5  # the frame integrates


@pytest.mark.parametrize("key", ["small", "large"])
def test_method_reproduces_the_split_modes(pj, key):
    """The per-pixel FLAT / CURVED choice == the oracle's half-width frame."""
    w, h = 33, 17
    prm = dict(raytrace_type=P.HALF_WIDTH, curved_percentage=0.4)
    b, f, s = pj.ref(key, False, P.RECTILINEAR, w, h, **prm)
    rb, rf, rs = pj.oracle.render(pj.wd.scene(key), pj.cam("view"), pj.params(**prm), w, h, pj.tex, pj.wd.test_rays[False])
    assert np.array_equal(b, rb) and np.array_equal(s, rs)
    flat = P.flat_mask(pj.params(**prm), w, h)
    assert 0 < flat.sum() < flat.size and (s[flat] == 0).all()


# The 1x1 cases are left out: their one pixel sits at uv = 0, where every
# projection's L is parallel to (0, 0, 1); the frame cannot differ.
BELOW_180 = [c for c in P.CASES if (c[4] is None or c[4] < 180.0) and c[2] * c[3] > 1]


DIFFER = [(key, c) for key in ("small", "large") for c in BELOW_180 if c[0] in P.CELLS[(key, False)]]


@pytest.mark.parametrize("key,case", DIFFER, ids=[f"{k}-{c[0]}" for k, c in DIFFER])
def test_cases_differ_from_the_rectilinear_frame(pj, key, case):
    """A projected frame is not the pinhole's: at least a quarter of the pixels
    differ from the oracle's own frame of the same camera."""
    cid, projection, w, h, fov = case
    b = pj.ref(key, False, projection, w, h, fov)[0]
    rb = pj.oracle.render(pj.wd.scene(key), pj.cam("view", fov), pj.params(), w, h, pj.tex, pj.wd.test_rays[False])[0]
    share = float((b != rb).any(-1).mean())
    assert share >= 0.25, f"{cid} on {key}: {share:.3f} of the pixels differ"


def test_fisheye_360_no_ray_pixels(pj):
    _, projection, w, h, fov = P.BY_ID["fisheye-48x48-fov360"]
    L, ray = P.local_dirs(projection, fov, w, h)
    assert int((~ray).sum()) == 500 and ray.size == 2304
    # the corners, never the inscribed disk
    ux, uy = P.uv_of(w, h)
    assert not ray[0, 0] and not ray[-1, -1] and ray[ux * ux + uy * uy <= 0.99].all()
    b, f, s = pj.ref("small", False, projection, w, h, fov)
    assert not b[~ray].any() and not f[~ray].any() and not s[~ray].any()
    assert int((s == 0).sum()) >= 500


def test_fisheye_180_has_every_ray_and_a_centre_pixel(pj):
    _, projection, w, h, fov = P.BY_ID["fisheye-41x41-fov180"]
    L, ray = P.local_dirs(projection, fov, w, h)
    assert ray.all()
    ux, uy = P.uv_of(w, h)
    assert ux[20, 20] == 0 and uy[20, 20] == 0  # rho == 0: the rule's other branch
    assert tuple(L[20, 20]) == (0.0, 0.0, 1.0)
    # the inscribed disk is the front hemisphere (the square's corners reach th = 127 degrees)
    assert (L[..., 2][ux * ux + uy * uy <= 1.0] >= -1e-6).all() and L[0, 0, 2] < 0


def test_equirect_360_is_the_whole_sphere():
    _, projection, w, h, fov = P.BY_ID["equirect-64x32-fov360"]
    L, ray = P.local_dirs(projection, fov, w, h)
    assert ray.all()
    n = np.linalg.norm(L.astype(np.float64), axis=-1)
    assert np.abs(n - 1).max() < 1e-6
    assert L[..., 2].min() < -0.99 and L[..., 2].max() > 0.99 and L[..., 0].min() < -0.99 and L[..., 0].max() > 0.99
    assert L[..., 1].min() < -0.99 and L[..., 1].max() > 0.99


def test_box_average_is_the_host_resolve(pkg):
    rng = np.random.default_rng(5)
    for ss in (2, 3):
        s = rng.integers(0, 256, size=(ss * 5, ss * 7, 4), dtype=np.uint8)
        assert np.array_equal(P.box_average(s, ss), pkg.abi.resolve_box(s, ss))
