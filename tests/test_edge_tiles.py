"""The host form of sr_edge_tiles (the tile selection of adaptive
supersampling, sr.h) against a numpy statement of its rule. No GPU.

Rule: two horizontal or vertical neighbours inside the frame are an edge pair
when max over the four channels of |a_c - b_c| > threshold; a 16x16 tile is
seeded when a pixel of it belongs to an edge pair (both tiles of a pair that
straddles a boundary); threshold < 0 seeds every tile, threshold >= 255 none;
the flagged set is the seeded set dilated `grow` times by the 3x3
neighbourhood on the tile grid. Nothing has a tolerance.
"""
import numpy as np
import pytest

SIZES = [(1, 1), (1, 40), (16, 16), (17, 33), (68, 44)]  # (width, height)
THRESHOLDS = [-1, 0, 7, 254, 255]


def rule(img, threshold, grow=0):
    """The definition in numpy: bool [ceil(H / 16), ceil(W / 16)]."""
    h, w = img.shape[:2]
    p = img.astype(np.int32)
    gy, gx = (h + 15) // 16, (w + 15) // 16
    m = np.zeros((gy, gx), dtype=bool)
    if threshold < 0:
        m[:] = True
    else:
        ys, xs = np.nonzero(np.abs(p[:, 1:] - p[:, :-1]).max(-1) > threshold)  # pairs (x, y), (x + 1, y)
        m[ys // 16, xs // 16] = True
        m[ys // 16, (xs + 1) // 16] = True
        ys, xs = np.nonzero(np.abs(p[1:] - p[:-1]).max(-1) > threshold)  # pairs (x, y), (x, y + 1)
        m[ys // 16, xs // 16] = True
        m[(ys + 1) // 16, xs // 16] = True
    for _ in range(grow):
        q = np.pad(m, 1)
        m = np.zeros_like(m)
        for j in range(3):
            for i in range(3):
                m |= q[j:j + gy, i:i + gx]
    return m


def flat(w, h, value=(40, 50, 60, 255)):
    return np.broadcast_to(np.array(value, dtype=np.uint8), (h, w, 4)).copy()


def flagged(pkg, img, threshold, grow=0):
    got = pkg.abi.edge_tiles(img, threshold, grow)
    assert got.dtype == np.uint8 and set(np.unique(got)) <= {0, 1}
    want = rule(img, threshold, grow)
    assert got.shape == want.shape
    assert np.array_equal(got.astype(bool), want), (threshold, grow, got, want.astype(np.uint8))
    return got.astype(bool)


@pytest.mark.parametrize("grow", [0, 1, 2])
@pytest.mark.parametrize("threshold", THRESHOLDS)
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_random_images(pkg, w, h, threshold, grow):
    """Noise (every tile has an edge pair at small thresholds), and a flat
    image with a few pixels changed by a few levels (some tiles flagged, some
    not, at thresholds 0 and 7)."""
    rng = np.random.default_rng(w * 1000 + h)
    noise = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    m = flagged(pkg, noise, threshold, grow)
    if threshold in (0, 7) and w * h >= 40:
        assert m.all()
    sparse = flat(w, h)
    for _ in range(3):
        y, x, c = rng.integers(0, h), rng.integers(0, w), rng.integers(0, 4)
        sparse[y, x, c] -= rng.integers(1, 16)
    m = flagged(pkg, sparse, threshold, grow)
    if threshold >= 254:
        assert not m.any()
    if threshold < 0:
        assert m.all()


def test_one_pixel_and_its_grown_sets(pkg):
    """One changed pixel inside a tile of a flat 68x44 image: that tile alone,
    its 3x3 and its 5x5 neighbourhood (clipped); the comparison is >, not >=."""
    img = flat(68, 44)
    img[20, 40, 1] += 9  # tile (2, 1), not at its border
    m0, m1, m2 = (flagged(pkg, img, 0, g) for g in (0, 1, 2))
    assert m0.sum() == 1 and m0[1, 2]
    assert m1.sum() == 9 and m1[0:3, 1:4].all()
    assert m2.sum() == 15
    assert flagged(pkg, img, 8, 0).sum() == 1 and flagged(pkg, img, 9, 0).sum() == 0  # > threshold, not >=


@pytest.mark.parametrize("pad", [4, 5, 37])
def test_padded_pitch(pkg, pad):
    """Rows pitch bytes apart, the padding filled with bytes that would be
    edges if they were read, the image not dword-aligned for odd pads."""
    abi, lib = pkg.abi, pkg.abi.load()
    w, h = 37, 21
    rng = np.random.default_rng(pad)
    img = flat(w, h)
    img[5, 15:17] = (200, 20, 30, 255)  # a pair inside row 5 that leaves tile 0 for tile 1
    pitch = 4 * w + pad
    buf = rng.integers(0, 256, pad + h * pitch, dtype=np.uint8)
    for y in range(h):
        buf[pad + y * pitch: pad + y * pitch + 4 * w] = img[y].reshape(-1)
    for threshold in (0, 100, 254):
        for grow in (0, 1):
            got = np.full((2, 3), 9, dtype=np.uint8)
            rc = lib.sr_edge_tiles(buf.ctypes.data + pad, pitch, w, h, threshold, grow, got.ctypes.data, 0, None)
            assert rc == abi.SR_OK
            assert np.array_equal(got.astype(bool), rule(img, threshold, grow)), (threshold, grow)
    assert rule(img, 100).sum() == 2


def test_single_pair_on_a_vertical_tile_boundary_flags_both_tiles(pkg):
    """A one-row image that steps between pixels 15 and 16: the frame's only
    edge pair straddles tiles 0 | 1."""
    img = flat(48, 1)
    img[0, 16:, 2] += 1
    assert flagged(pkg, img, 0).tolist() == [[True, True, False]]
    assert flagged(pkg, img, 1).tolist() == [[False, False, False]]


def test_single_pair_on_a_horizontal_tile_boundary_flags_both_tiles(pkg):
    img = flat(1, 48)
    img[32:, 0, 0] += 100  # rows 31 | 32
    assert flagged(pkg, img, 99).tolist() == [[False], [True], [True]]
    assert flagged(pkg, img, 99, 1).tolist() == [[True], [True], [True]]


def test_single_pair_on_tile_boundaries(pkg):
    """One changed pixel at a tile's corner pixel: its pairs with the
    neighbours across the vertical and the horizontal boundary seed those
    tiles too, the diagonal tile stays unflagged."""
    img = flat(48, 48)
    img[16, 16, 0] += 5  # the first pixel of tile (1, 1); neighbours (15, 16) in tile (0, 1), (16, 15) in tile (1, 0)
    m = flagged(pkg, img, 4)
    want = np.zeros((3, 3), dtype=bool)
    want[1, 1] = want[1, 0] = want[0, 1] = True
    assert np.array_equal(m, want)
    assert not flagged(pkg, img, 5).any()
    # a pair exactly on a horizontal boundary alone: rows 15 | 16 differ along a whole row band of one tile column
    img = flat(48, 48)
    img[16:, 20:24, 2] += 1
    img[17:, 20:24, 2] -= 1  # only row 16, columns 20 .. 23 differ: pairs with rows 15 and 17, and (19|20), (23|24)
    m = flagged(pkg, img, 0)
    want = np.zeros((3, 3), dtype=bool)
    want[0, 1] = want[1, 1] = True
    assert np.array_equal(m, want)


def test_pair_in_a_partial_last_tile(pkg):
    img = flat(68, 44)  # last tile column 4 pixels wide, last tile row 12 high
    img[43, 67, 3] = 0  # the frame's last pixel
    m = flagged(pkg, img, 254)
    want = np.zeros((3, 5), dtype=bool)
    want[2, 4] = True
    assert np.array_equal(m, want)
    img = flat(68, 44)
    img[40, 64:, 0] = 99  # the partial column's pixels of row 40; (63, 40) | (64, 40) straddles tiles 3 | 4
    m = flagged(pkg, img, 50)
    want = np.zeros((3, 5), dtype=bool)
    want[2, 3] = want[2, 4] = True
    assert np.array_equal(m, want)
    assert flagged(pkg, img, 50, 1).sum() == 6 and flagged(pkg, img, 50, 2).sum() == 12


def test_contrast_only_in_alpha(pkg):
    img = flat(32, 16)
    img[:, 20:, 3] = 200  # alpha 255 | 200 between columns 19 and 20, tile 1 only
    assert flagged(pkg, img, 54).tolist() == [[False, True]]
    assert flagged(pkg, img, 55).tolist() == [[False, False]]


def test_diagonal_only_contrast_flags_nothing(pkg):
    """Two pixels that touch only at a corner are not neighbours: red is
    5 (x % 2) + 5 (y % 2), so neighbours differ by 5 and the pixels of a
    (0, 0) - (1, 1) diagonal by 10."""
    yy, xx = np.mgrid[0:40, 0:40]
    img = flat(40, 40)
    img[..., 0] = (5 * (xx % 2) + 5 * (yy % 2)).astype(np.uint8)
    assert int(np.abs(img[1:, 1:, 0].astype(int) - img[:-1, :-1, 0]).max()) == 10
    assert not flagged(pkg, img, 5).any()
    assert flagged(pkg, img, 4).all()


def test_rejections(pkg):
    abi, lib = pkg.abi, pkg.abi.load()
    img = flat(20, 20)
    mask = np.full((2, 2), 7, dtype=np.uint8)
    p, m = img.ctypes.data, mask.ctypes.data

    def call(rgba=p, pitch=80, w=20, h=20, thr=0, grow=0, out=m):
        return lib.sr_edge_tiles(rgba, pitch, w, h, thr, grow, out, 0, None)

    assert call(rgba=None) == abi.SR_E_INVALID
    assert call(out=None) == abi.SR_E_INVALID
    assert call(w=0) == abi.SR_E_INVALID and call(h=0) == abi.SR_E_INVALID and call(w=-3) == abi.SR_E_INVALID
    assert call(pitch=79) == abi.SR_E_INVALID
    assert call(grow=-1) == abi.SR_E_INVALID and call(grow=3) == abi.SR_E_INVALID
    assert (mask == 7).all()  # nothing was written
    assert call() == abi.SR_OK and (mask == 0).all()
    assert call(thr=-(1 << 31)) == abi.SR_OK and (mask == 1).all()
    assert call(thr=(1 << 31) - 1) == abi.SR_OK and (mask == 0).all()
