"""sr_projection_dir (host only, no GPU): the library's statement of a pixel's
local direction, the code init_pixel runs, equals the numpy statement of
tests/projection_cases.py bit for bit, and the call rejects bad arguments.
"""
import ctypes as C

import numpy as np
import pytest

import projection_cases as P

OWN_FOV = 90.0  # World's "view" camera (scenes.camera_look's default)
# every case, and the pinhole at the sizes of the first ones
FRAMES = [(c[0], c[1], c[2], c[3], OWN_FOV if c[4] is None else c[4]) for c in P.CASES] + [
    ("rectilinear-68x44-fov120", P.RECTILINEAR, 68, 44, 120.0),
    ("rectilinear-33x17-own", P.RECTILINEAR, 33, 17, OWN_FOV),
    ("fisheye-17x11-fov300", P.FISHEYE, 17, 11, 300.0),
    ("equirect-17x11-fov33.3", P.EQUIRECT, 17, 11, 33.3),
]


def test_own_fov_is_the_view_cameras(pkg):
    assert pkg.scenes.camera_look((0.0, 2.0, 15.0), (0.0, -2.0, -15.0)).fov == OWN_FOV


@pytest.mark.parametrize("frame", FRAMES, ids=[f[0] for f in FRAMES])
def test_projection_dir_equals_the_numpy_statement(pkg, frame):
    _, projection, w, h, fov = frame
    lib = pkg.abi.load()
    L, ray = P.local_dirs(projection, fov, w, h)
    got = np.zeros((h, w, 3), dtype=np.float32)
    rcs = np.zeros((h, w), dtype=np.int32)
    buf = (C.c_float * 3)()
    for y in range(h):
        for x in range(w):
            buf[0] = buf[1] = buf[2] = 77.0
            rcs[y, x] = lib.sr_projection_dir(projection, fov, w, h, x, y, buf)
            got[y, x] = buf[:]
    assert np.array_equal(rcs == 1, ray) and np.array_equal(rcs == 0, ~ray), "the no-ray set differs"
    assert (got[~ray] == 77.0).all(), "a pixel without a ray had its output written"
    bad = (got.view(np.uint32) != L.view(np.uint32)).any(-1) & ray
    assert not bad.any(), f"{int(bad.sum())} of {int(ray.sum())} directions differ in bits"


def test_python_wrapper(pkg):
    abi = pkg.abi
    L, ray = P.local_dirs(P.FISHEYE, 360.0, 48, 48)
    assert abi.projection_dir(abi.PROJECTION_FISHEYE, 360.0, 48, 48, 0, 0) is None and not ray[0, 0]
    got = abi.projection_dir(abi.PROJECTION_FISHEYE, 360.0, 48, 48, 30, 20)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), L[20, 30].view(np.uint32))
    assert (abi.PROJECTION_RECTILINEAR, abi.PROJECTION_EQUIRECT, abi.PROJECTION_FISHEYE) == (0, 1, 2)
    assert abi.PROJECTIONS == {"rectilinear": 0, "equirect": 1, "fisheye": 2}


def test_nan_fov_has_no_fisheye_ray(pkg):
    lib = pkg.abi.load()
    buf = (C.c_float * 3)(1.0, 2.0, 3.0)
    assert lib.sr_projection_dir(P.FISHEYE, float("nan"), 8, 8, 3, 3, buf) == 0
    assert list(buf) == [1.0, 2.0, 3.0]


def test_bad_arguments_rejected(pkg):
    abi = pkg.abi
    lib = abi.load()
    buf = (C.c_float * 3)(5.0, 5.0, 5.0)
    E = abi.SR_E_INVALID
    assert lib.sr_projection_dir(-1, 90.0, 8, 8, 0, 0, buf) == E
    assert lib.sr_projection_dir(3, 90.0, 8, 8, 0, 0, buf) == E
    assert lib.sr_projection_dir(1, 90.0, 0, 8, 0, 0, buf) == E
    assert lib.sr_projection_dir(1, 90.0, 8, -1, 0, 0, buf) == E
    assert lib.sr_projection_dir(1, 90.0, 8, 8, -1, 0, buf) == E
    assert lib.sr_projection_dir(1, 90.0, 8, 8, 8, 0, buf) == E
    assert lib.sr_projection_dir(1, 90.0, 8, 8, 0, 8, buf) == E
    assert lib.sr_projection_dir(1, 90.0, 8, 8, 0, -3, buf) == E
    assert lib.sr_projection_dir(1, 90.0, 2**30, 8, 0, 0, buf) == E
    assert lib.sr_projection_dir(1, 90.0, 8, 8, 0, 0, None) == E
    assert list(buf) == [5.0, 5.0, 5.0]
    with pytest.raises(abi.SRError):
        abi.projection_dir(7, 90.0, 8, 8, 0, 0)
    # a null context
    assert lib.sr_set_projection(None, 1) == E and lib.sr_get_projection(None) == E
