"""Shutter frames (sr.h) without a device: the host form of sr_shutter_resolve
against numpy, the default phases, the kernel's division and every rejection
that needs no context.
"""
import ctypes as C

import numpy as np
import pytest

OK, INV, CAP, NOT_READY = 0, -1, -2, -5
FILL = 77


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.abi.load()


def rule(images, k):
    """[M k, rows, w, 4] -> [M, rows, w, 4] by the definition, in integers"""
    n, rows, w, _ = images.shape
    total = images.reshape(n // k, k, rows, w, 4).astype(np.int64).sum(1)
    return np.minimum(255, (total + k // 2) // k).astype(np.uint8)


class Buf:
    """n sentinel-padded images of rows x w in host memory: row r of image j at j * stride + r * pitch"""

    def __init__(self, n, rows, w, pad, tail, align=16, offset=0):
        self.n, self.rows, self.w = n, rows, w
        self.pitch = 4 * w + pad
        self.stride = self.pitch * rows + tail
        raw = np.full(n * self.stride + align + offset, FILL, dtype=np.uint8)
        o = (-raw.ctypes.data) % align + offset
        self.a = raw[o:o + n * self.stride]

    def ptr(self):
        return self.a.ctypes.data

    def put(self, images):
        v = self.a.reshape(self.n, self.stride)[:, :self.pitch * self.rows].reshape(self.n, self.rows, self.pitch)
        v[:, :, :4 * self.w] = images.reshape(self.n, self.rows, 4 * self.w)

    def get(self, label):
        """[n, rows, w, 4] once every padding byte is seen to hold the sentinel"""
        a = self.a.reshape(self.n, self.stride)
        assert (a[:, self.pitch * self.rows:] == FILL).all(), f"{label}: wrote between the images"
        a = a[:, :self.pitch * self.rows].reshape(self.n, self.rows, self.pitch)
        assert (a[:, :, 4 * self.w:] == FILL).all(), f"{label}: wrote behind a row"
        return np.ascontiguousarray(a[:, :, :4 * self.w]).reshape(self.n, self.rows, self.w, 4)


def images_of(kind, n, rows, w, rng):
    if kind == "zeros":
        return np.zeros((n, rows, w, 4), dtype=np.uint8)
    if kind == "ones":
        return np.full((n, rows, w, 4), 255, dtype=np.uint8)
    return rng.integers(0, 256, size=(n, rows, w, 4), dtype=np.uint8)


@pytest.mark.parametrize("kind", ["zeros", "ones", "random"])
def test_host_resolve_equals_numpy(lib, kind):
    """Every K in 1 .. 32, M in 1 .. 5, widths 1, 3, 4, 5, 17, padded pitches and strides."""
    rng = np.random.default_rng(20261021)
    for k in range(1, 33):
        M = 1 + (k - 1) % 5
        for w in (1, 3, 4, 5, 17):
            rows = 3
            src, dst = Buf(M * k, rows, w, 12, 40), Buf(M, rows, w, 20, 8)
            img = images_of(kind, M * k, rows, w, rng)
            src.put(img)
            rc = lib.sr_shutter_resolve(src.ptr(), src.pitch, src.stride, k, M, w, rows, dst.ptr(), dst.pitch, dst.stride,
                                        0, None)
            assert rc == OK, (k, M, w, rc)
            got = dst.get(f"K {k} M {M} w {w}")
            assert np.array_equal(got, rule(img, k)), f"{kind}: K {k} M {M} width {w}"
            assert np.array_equal(src.get("the images"), img), "the resolve changed its input"


def test_every_frame_count(lib):
    rng = np.random.default_rng(7)
    for M in range(1, 6):
        for k in (1, 3, 32):
            img = images_of("random", M * k, 2, 5, rng)
            src, dst = Buf(M * k, 2, 5, 4, 0), Buf(M, 2, 5, 0, 4)
            src.put(img)
            assert lib.sr_shutter_resolve(src.ptr(), src.pitch, src.stride, k, M, 5, 2, dst.ptr(), dst.pitch, dst.stride, 0,
                                          None) == OK
            assert np.array_equal(dst.get(f"M {M}"), rule(img, k))


def test_package_level_forms(pkg):
    rng = np.random.default_rng(11)
    img = images_of("random", 6, 4, 7, rng)
    assert np.array_equal(pkg.shutter_resolve(img, 3), rule(img, 3))
    assert np.array_equal(pkg.shutter_resolve(img, 1), img)
    with pytest.raises(ValueError):
        pkg.shutter_resolve(img, 4)
    assert pkg.shutter_phases(2, 4).tolist() == [list(p) for p in pkg.abi.phase_order(2)]


def test_default_phases_against_phase_order(lib, pkg):
    for ss in range(1, pkg.abi.MAX_SUPERSAMPLE + 1):
        order = pkg.abi.phase_order(ss)
        for k in (1, 2, ss * ss, ss * ss + 1, 32, 40):
            out = np.full(2 * k + 2, FILL, dtype=np.uint8)
            assert lib.sr_shutter_phases(ss, k, out.ctypes.data) == OK
            assert (out[2 * k:] == FILL).all()
            for j in range(k):
                assert (out[2 * j], out[2 * j + 1]) == order[j % (ss * ss)], (ss, k, j)
    out = np.zeros(8, dtype=np.uint8)
    assert lib.sr_shutter_phases(0, 2, out.ctypes.data) == INV
    assert lib.sr_shutter_phases(5, 2, out.ctypes.data) == INV
    assert lib.sr_shutter_phases(2, 0, out.ctypes.data) == INV
    assert lib.sr_shutter_phases(2, 2, None) == INV


def test_the_kernels_division_is_exact_for_every_operand(lib):
    """kernels/shutter_div.h through sr_debug_shutter_div: n div k for every n
    a sum plus its rounding term can be (k * 255 + k / 2 and beyond, up to
    2^16 - 1) and every k in 1 .. 256."""
    div = lib.sr_debug_shutter_div
    for k in range(1, 257):
        top = k * 255 + k // 2
        # every multiple of k and its neighbours (where a quotient can be off by one), and the range's ends
        ns = set()
        for q in range(0, 65536 // k + 1):
            ns.update((q * k - 1, q * k, q * k + 1))
        ns.update((0, top - 1, top, top + 1, 65535))
        for n in ns:
            if 0 <= n <= 65535:
                assert div(n, k) == n // k, (n, k)
    for k in (1, 2, 3, 7, 32, 255, 256):  # and every operand for some divisors
        for n in range(65536):
            assert div(n, k) == n // k, (n, k)
    assert div(65536, 3) == -1 and div(5, 0) == -1 and div(5, 257) == -1 and div(-1, 3) == -1


def test_resolve_rejections_write_nothing(lib):
    rng = np.random.default_rng(3)
    w, rows, k, M = 5, 3, 2, 2
    img = images_of("random", M * k, rows, w, rng)

    def call(images=True, out=True, pitch=None, stride=None, k=k, M=M, w=w, rows=rows, opitch=None, ostride=None,
             src_off=0, dst_off=0):
        src, dst = Buf(4, 3, 5, 12, 40, offset=src_off), Buf(2, 3, 5, 20, 8, offset=dst_off)
        src.put(img)
        rc = lib.sr_shutter_resolve(src.ptr() if images else None, src.pitch if pitch is None else pitch,
                                    src.stride if stride is None else stride, k, M, w, rows, dst.ptr() if out else None,
                                    dst.pitch if opitch is None else opitch, dst.stride if ostride is None else ostride,
                                    0, None)
        assert (dst.a == FILL).all(), "a rejected resolve wrote pixels"
        return rc

    assert call(images=False) == INV
    assert call(out=False) == INV
    assert call(k=0) == INV
    assert call(k=257) == INV
    assert call(M=0) == INV
    assert call(M=65536) == INV
    assert call(w=0) == INV
    assert call(rows=-1) == INV
    assert call(pitch=4 * w - 4) == INV
    assert call(opitch=4 * w - 4) == INV
    assert call(stride=(4 * w + 12) * rows - 4) == INV
    assert call(ostride=(4 * w + 20) * rows - 4) == INV
    assert call(pitch=4 * w + 2) == INV  # not a multiple of 4
    assert call(stride=(4 * w + 12) * rows + 42) == INV
    assert call(opitch=4 * w + 2) == INV
    assert call(ostride=(4 * w + 20) * rows + 10) == INV
    assert call(src_off=1) == INV
    assert call(dst_off=2) == INV
    assert call(rows=0) == OK  # no rows: nothing is written


def test_render_rejections_without_a_context(lib, pkg):
    """The checks ahead of the context's: a null context is SR_E_INVALID."""
    abi = pkg.abi
    cam, prm = abi.default_camera(), abi.default_params()
    cams = (abi.Camera * 4)(cam, cam, cam, cam)
    out = np.full(4 * 8 * 8 * 4, FILL, dtype=np.uint8)
    acc = np.full(8 * 8 * 4, FILL, dtype=np.uint16)
    blocks = (C.c_int * 1)(0)
    assert lib.sr_render_shutter(None, 0, cams, None, 2, 2, C.byref(prm), 8, 8, 0, 8, 1, out.ctypes.data, 32, 256,
                                 None) == INV
    assert lib.sr_render_shutter_block_list(None, 0, cams, None, 2, 2, C.byref(prm), 8, 8, 8, blocks, 1, 1,
                                            out.ctypes.data, 32, 256, None) == INV
    assert lib.sr_render_accumulate_shutter(None, 0, cams, None, 4, C.byref(prm), 8, 8, 0, 8, 1, 1, acc.ctypes.data, 64,
                                            None) == INV
    assert (out == FILL).all() and (acc == FILL).all()


def test_bindings_cover_the_header(pkg):
    for name in pkg.abi.SINCE_SHUTTER:
        assert name in pkg.abi.SIGNATURES and hasattr(pkg.abi.load(), name), name
    assert pkg.abi.SHUTTER_OWN_SCENE == -1
