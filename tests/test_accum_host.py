"""The host forms of sr_accum_add and sr_accum_resolve against numpy,
sr_phase_order against sr.h's table, and the argument rejections that need no
context (CPU). Nothing has a tolerance.

    add:     acc[y][x][c] = (acc[y][x][c] + sum_k image_k[y][x][c]) mod 2^16   (reset: without acc)
    resolve: out[y][x][c] = min(255, (acc[y][x][c] + n // 2) // n)
"""
import ctypes as C

import numpy as np
import pytest

COUNTS = [1, 2, 3, 4, 9, 16, 255, 256]
SIZES = [(1, 1), (3, 2), (17, 11), (300, 3)]  # (width, rows)
ORDERS = {
    1: [(0, 0)],
    2: [(0, 0), (1, 1), (1, 0), (0, 1)],
    3: [(1, 1), (0, 0), (2, 2), (2, 0), (0, 2), (1, 0), (1, 2), (0, 1), (2, 1)],
    4: [(0, 0), (2, 2), (2, 0), (0, 2), (1, 1), (3, 3), (3, 1), (1, 3),
        (1, 0), (3, 2), (3, 0), (1, 2), (0, 1), (2, 3), (2, 1), (0, 3)],
}


def add_reference(images, accum=None):
    s = images.astype(np.int64).sum(0)
    if accum is not None:
        s = s + accum.astype(np.int64)
    return (s % 65536).astype(np.uint16)


def resolve_reference(accum, n):
    return np.minimum(255, (accum.astype(np.int64) + n // 2) // n).astype(np.uint8)


def aligned(nbytes, fill):
    """A host byte buffer whose base is a multiple of 8."""
    raw = np.full(nbytes + 8, fill, dtype=np.uint8)
    o = (-raw.ctypes.data) % 8
    return raw[o:o + nbytes]


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("width,rows", SIZES)
def test_add_then_resolve(pkg, width, rows, n):
    """n random images added in two groups (a reset store, then an add) and
    resolved with n: the sum and the frame are numpy's."""
    abi = pkg.abi
    rng = np.random.default_rng(1000 * width + 10 * rows + n)
    images = rng.integers(0, 256, (n, rows, width, 4), dtype=np.uint8)
    k = max(1, n // 3)
    acc = abi.accum_add(images[:k], reset=True)
    assert np.array_equal(acc, add_reference(images[:k]))
    if k < n:
        assert abi.accum_add(images[k:], acc) is acc
    want = add_reference(images)
    assert np.array_equal(acc, want)
    assert np.array_equal(abi.accum_resolve(acc, n), resolve_reference(want, n))
    # the mean of n images is a byte: no clamp happens, and the rule is the rounded mean
    assert np.array_equal(abi.accum_resolve(acc, n), ((images.astype(np.int64).sum(0) + n // 2) // n).astype(np.uint8))


def test_all_255_at_256(pkg):
    """256 x 255 = 65280 fits the 16-bit field and resolves to 255."""
    abi = pkg.abi
    images = np.full((256, 2, 5, 4), 255, dtype=np.uint8)
    acc = abi.accum_add(images)
    assert (acc == 65280).all()
    assert (abi.accum_resolve(acc, 256) == 255).all()


def test_reset_ignores_and_add_keeps_the_accumulator(pkg):
    abi = pkg.abi
    rng = np.random.default_rng(5)
    images = rng.integers(0, 256, (3, 4, 9, 4), dtype=np.uint8)
    start = rng.integers(0, 65536, (4, 9, 4), dtype=np.uint16)
    start[0, 0], images[:, 0, 0] = 65535, 1  # wraps to 2
    acc = start.copy()
    abi.accum_add(images, acc, reset=False)
    assert np.array_equal(acc, add_reference(images, start))  # modulo 2^16 where it wraps
    assert (add_reference(images, start).astype(np.int64) != images.astype(np.int64).sum(0) + start).any()
    abi.accum_add(images, acc, reset=True)
    assert np.array_equal(acc, add_reference(images))
    one = abi.accum_add(images[0], reset=True)  # one [rows, W, 4] image
    assert np.array_equal(one, images[0].astype(np.uint16))


def test_resolve_is_exact_for_every_value_and_count(pkg):
    """Every acc in 0 .. 65535 with every n in 1 .. 256."""
    abi = pkg.abi
    acc = np.arange(65536, dtype=np.uint16).reshape(64, 256, 4)
    for n in range(1, 257):
        assert np.array_equal(abi.accum_resolve(acc, n), resolve_reference(acc, n)), n


def test_padded_pitches(pkg):
    """Image pitch 4 W + 12, a gap between images, accumulator pitch 8 W + 24,
    output pitch 4 W + 8: the payload is the reference's, the padding keeps
    its sentinel."""
    abi, lib = pkg.abi, pkg.abi.load()
    w, rows, n = 7, 5, 3
    rng = np.random.default_rng(9)
    images = rng.integers(0, 256, (n, rows, w, 4), dtype=np.uint8)
    start = rng.integers(0, 65536, (rows, w, 4), dtype=np.uint16)
    ip, ap, op = 4 * w + 12, 8 * w + 24, 4 * w + 8
    istride = ip * rows + 16
    src = aligned(n * istride, 0x3C)
    for k in range(n):
        for y in range(rows):
            o = k * istride + y * ip
            src[o:o + 4 * w] = images[k, y].reshape(-1)
    acc = aligned(rows * ap, 0xA5)
    for y in range(rows):
        acc[y * ap:y * ap + 8 * w] = start[y].reshape(-1).view(np.uint8)
    acc_want = acc.copy()
    sums = add_reference(images, start)
    for y in range(rows):
        acc_want[y * ap:y * ap + 8 * w] = sums[y].reshape(-1).view(np.uint8)
    assert lib.sr_accum_add(src.ctypes.data, ip, istride, n, w, rows, 0, acc.ctypes.data, ap, 0, None) == abi.SR_OK
    assert np.array_equal(acc, acc_want)
    out = aligned(rows * op, 0xA5)
    out_want = out.copy()
    px = resolve_reference(sums, n)
    for y in range(rows):
        out_want[y * op:y * op + 4 * w] = px[y].reshape(-1)
    assert lib.sr_accum_resolve(acc.ctypes.data, ap, w, rows, n, out.ctypes.data, op, 0, None) == abi.SR_OK
    assert np.array_equal(out, out_want)


@pytest.mark.parametrize("ss", [1, 2, 3, 4])
def test_phase_order(pkg, ss):
    order = pkg.abi.phase_order(ss)
    assert order == ORDERS[ss]
    assert sorted(order) == [(i, j) for i in range(ss) for j in range(ss)]  # a permutation of the grid


def test_phase_order_rejections(pkg):
    abi, lib = pkg.abi, pkg.abi.load()
    x, y = C.c_int(-7), C.c_int(-7)
    for ss, k in [(0, 0), (5, 0), (-1, 0), (2, 4), (2, -1), (4, 16), (1, 1)]:
        assert lib.sr_phase_order(ss, k, C.byref(x), C.byref(y)) == abi.SR_E_INVALID, (ss, k)
    assert lib.sr_phase_order(2, 0, None, C.byref(y)) == abi.SR_E_INVALID
    assert lib.sr_phase_order(2, 0, C.byref(x), None) == abi.SR_E_INVALID
    assert (x.value, y.value) == (-7, -7)
    with pytest.raises(abi.SRError):
        abi.phase_order(5)


def test_rejections_without_a_context(pkg):
    """Each bad call returns SR_E_INVALID (SR_E_CAPACITY above 32 phases) and
    writes nothing; the render calls refuse a null context after their own
    arguments."""
    abi, lib = pkg.abi, pkg.abi.load()
    w, rows = 4, 3
    img = aligned(2 * 4 * w * rows, 1)
    acc = aligned(8 * w * rows, 0xA5)
    out = aligned(4 * w * rows, 0xA5)
    I, A, O = img.ctypes.data, acc.ctypes.data, out.ctypes.data

    def add(images=I, pitch=4 * w, stride=4 * w * rows, n=2, width=w, r=rows, accum=A, ap=8 * w):
        return lib.sr_accum_add(images, pitch, stride, n, width, r, 0, accum, ap, 0, None)

    def resolve(accum=A, ap=8 * w, width=w, r=rows, n=4, o=O, pitch=4 * w):
        return lib.sr_accum_resolve(accum, ap, width, r, n, o, pitch, 0, None)

    bad_add = [dict(images=None), dict(accum=None), dict(width=0), dict(r=-1), dict(n=0), dict(n=257),
               dict(pitch=4 * w - 4), dict(ap=8 * w - 8), dict(stride=4 * w * rows - 4), dict(accum=A + 4),
               dict(accum=A + 2), dict(ap=8 * w + 4), dict(images=I + 1), dict(pitch=4 * w + 2)]
    for kw in bad_add:
        assert add(**kw) == abi.SR_E_INVALID, kw
    bad_resolve = [dict(accum=None), dict(o=None), dict(width=0), dict(r=-1), dict(n=0), dict(n=257), dict(n=-1),
                   dict(pitch=4 * w - 4), dict(ap=8 * w - 8), dict(accum=A + 4), dict(ap=8 * w + 4), dict(o=O + 2),
                   dict(pitch=4 * w + 2)]
    for kw in bad_resolve:
        assert resolve(**kw) == abi.SR_E_INVALID, kw
    assert (acc == 0xA5).all() and (out == 0xA5).all()
    assert add() == abi.SR_OK and resolve(n=2) == abi.SR_OK
    assert (acc.view(np.uint16) == 0xA5A5 + 2).all()  # the good calls after them: two images of ones added
    assert (out == min(255, (0xA5A5 + 2 + 1) // 2)).all()

    cam, prm = abi.default_camera(), abi.default_params()
    ph = (C.c_uint8 * 66)(*([0] * 66))

    def phase(ss=2, x=0, y=0, o=O):
        return lib.sr_render_phase(None, C.byref(cam), C.byref(prm), w, rows, 0, rows, ss, x, y, o, 4 * w, None)

    def accumulate(ss=2, phases=ph, n=1, accum=A, ap=8 * w):
        return lib.sr_render_accumulate(None, C.byref(cam), C.byref(prm), w, rows, 0, rows, ss, phases, n, 1, accum, ap,
                                        None)

    for kw in [dict(ss=0), dict(ss=5), dict(x=2), dict(x=-1), dict(y=2), dict(ss=1, y=1), dict(o=None), dict()]:
        assert phase(**kw) == abi.SR_E_INVALID, kw
    for kw in [dict(ss=0), dict(ss=5), dict(phases=None), dict(accum=None), dict(n=0), dict(accum=A + 4),
               dict(ap=8 * w + 4), dict(ap=8 * w - 8), dict(phases=(C.c_uint8 * 2)(0, 2)), dict()]:
        assert accumulate(**kw) == abi.SR_E_INVALID, kw
    assert accumulate(n=33) == abi.SR_E_CAPACITY
