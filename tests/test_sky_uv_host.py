"""sr_sky_uv (sr.h "Ray maps", include/sr/sky.hpp: the code the ray-map
kernels run) against tests/ray_map_cases.py's sky_uv_np, bit for bit, a NaN
matching a NaN. No GPU."""
import ctypes as C

import numpy as np

import ray_map_cases as R

F = np.float32


def host_uv(pkg, dirs):
    return np.stack([pkg.abi.sky_uv(d) for d in np.asarray(dirs, dtype=F).reshape(-1, 3)])


def check(pkg, dirs, label):
    dirs = np.asarray(dirs, dtype=F).reshape(-1, 3)
    got, want = host_uv(pkg, dirs), R.sky_uv_np(dirs)
    ok = R.same_bits(got, want).all(-1)
    assert ok.all(), (label, dirs[~ok][:4], got[~ok][:4], want[~ok][:4])
    return got


def test_equirect_frame(pkg):
    cam = pkg.scenes.camera_look((0.0, 0.0, 12.0), (0.2, -0.1, -1.0), fov=360.0)
    _, d = pkg.abi.camera_rays(cam, "equirect", 64, 32)
    uv = check(pkg, d, "equirect 64x32")
    assert np.isfinite(uv).all() and uv.min() >= 0.0 and uv.max() <= 1.0
    assert len(np.unique(uv[:, 0])) > 1000 and len(np.unique(uv[:, 1])) > 1000


def test_axes_poles_and_seam(pkg):
    axes = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    uv = check(pkg, axes, "axes")
    assert uv[2, 1] == 1.0 and uv[3, 1] == 0.0  # the poles: v = asin(+-1) / PI + 0.5
    # the u seam: x < 0 with z = +0 (u = 0.5 from above) and z = -0 (atan2 = -pi: + 2, * 0.5)
    seam = [(-1.0, 0.0, 0.0), (-1.0, 0.0, -0.0), (-0.5, 0.3, 0.0), (-0.5, 0.3, -0.0), (-1.0, 0.0, 1e-30), (-1.0, 0.0, -1e-30),
            (1.0, 0.0, -0.0), (0.0, 0.0, 0.0), (-0.0, 0.0, -0.0)]
    uv = check(pkg, seam, "seam")
    assert uv[0, 0] == 0.5 and uv[1, 0] == 0.5  # both sides of the seam meet: (-pi / PI + 2) * 0.5


def test_unnormalised_and_non_finite(pkg):
    nan, inf = float("nan"), float("inf")
    dirs = [(3.0, 0.5, -4.0), (1e-20, 0.25, 1e-20), (1e20, -0.75, -1e20),   # unnormalised
            (0.3, 1.5, 0.2), (0.3, -1.0000001, 0.2), (0.0, 2.0, 0.0),       # |y| > 1: asin is a NaN
            (nan, 0.1, 0.2), (0.1, nan, 0.2), (0.1, 0.2, nan), (nan, nan, nan),
            (inf, 0.1, 0.2), (0.1, 0.2, -inf), (inf, 0.0, inf), (-inf, 0.0, -inf), (0.1, inf, 0.2)]
    uv = check(pkg, dirs, "extremes")
    assert np.isnan(uv[3:6, 1]).all() and np.isfinite(uv[3:6, 0]).all()
    rng = np.random.default_rng(5)
    check(pkg, rng.normal(size=(500, 3)) * np.exp(rng.uniform(-10, 10, size=(500, 1))), "random")


def test_null_arguments(pkg):
    lib = pkg.abi.load()
    d, out = (C.c_float * 3)(1.0, 0.0, 0.0), (C.c_float * 2)(7.0, 7.0)
    assert lib.sr_sky_uv(None, out) == pkg.abi.SR_E_INVALID
    assert lib.sr_sky_uv(d, None) == pkg.abi.SR_E_INVALID
    assert lib.sr_sky_uv(None, None) == pkg.abi.SR_E_INVALID
    assert tuple(out) == (7.0, 7.0)
    assert lib.sr_sky_uv(d, out) == 0 and tuple(out) == (0.0, 0.5)
