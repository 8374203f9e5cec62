"""The box resolve of supersampled frames, without a GPU: the host form of
sr_resolve_box against numpy applying sr.h's rule

    out[y][x][c] = (sum of the ss x ss samples' bytes + (ss ss) / 2) div (ss ss)

on random and constructed bytes (no tolerance), its argument checks, and
dist.supersample_block_costs against a hand-written loop."""
import ctypes as C

import numpy as np
import pytest

SENTINEL = 0xA5


def box_reference(samples, ss):
    """The rule in numpy: [..., ss * rows, ss * W, 4] uint8 -> [..., rows, W, 4]."""
    s = np.asarray(samples)
    rows, w = s.shape[-3] // ss, s.shape[-2] // ss
    v = s.reshape(s.shape[:-3] + (rows, ss, w, ss, 4)).astype(np.int64)
    return ((v.sum(axis=(-4, -2)) + (ss * ss) // 2) // (ss * ss)).astype(np.uint8)


@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("rows", [1, 3, 11])
@pytest.mark.parametrize("width", [1, 5, 67])
@pytest.mark.parametrize("ss", [1, 2, 3, 4])
def test_host_resolve_equals_numpy_in_padded_buffers(pkg, ss, width, rows, frames):
    """Padded pitches and frame strides, the images in the middle of
    sentinel-filled buffers: the payload equals numpy's, and no byte outside
    the payload changed."""
    abi, lib = pkg.abi, pkg.abi.load()
    rng = np.random.default_rng(1000 * ss + 100 * width + 10 * rows + frames)
    samples = rng.integers(0, 256, (frames, ss * rows, ss * width, 4), dtype=np.uint8)
    want = box_reference(samples, ss)
    assert np.array_equal(abi.resolve_box(samples, ss), want)  # the dense form
    sp, op, guard = 4 * ss * width + 12, 4 * width + 20, 64
    sstride, ostride = sp * ss * rows + 40, op * rows + 28
    src = np.full(2 * guard + frames * sstride, 0x3C, dtype=np.uint8)
    dst = np.full(2 * guard + frames * ostride, SENTINEL, dtype=np.uint8)
    expect = dst.copy()
    for f in range(frames):
        for r in range(ss * rows):
            o = guard + f * sstride + r * sp
            src[o:o + 4 * ss * width] = samples[f, r].reshape(-1)
        for r in range(rows):
            o = guard + f * ostride + r * op
            expect[o:o + 4 * width] = want[f, r].reshape(-1)
    before = src.copy()
    rc = lib.sr_resolve_box(src.ctypes.data + guard, sp, sstride, width, rows, ss, dst.ctypes.data + guard, op,
                            ostride, frames, 0, None)
    assert rc == abi.SR_OK
    assert np.array_equal(src, before)
    bad = dst != expect
    assert not bad.any(), f"{int(bad.sum())} bytes differ (payload or padding)"


@pytest.mark.parametrize("ss", [1, 2, 3, 4])
def test_constructed_inputs(pkg, ss):
    abi = pkg.abi
    n = ss * ss
    shape = (ss * 3, ss * 5, 4)
    assert (abi.resolve_box(np.zeros(shape, np.uint8), ss) == 0).all()
    assert (abi.resolve_box(np.full(shape, 255, np.uint8), ss) == 255).all()
    # a single 255 among zeros, at every sample position of one pixel and in every channel
    for j in range(ss):
        for i in range(ss):
            for c in range(4):
                s = np.zeros(shape, np.uint8)
                s[ss * 1 + j, ss * 2 + i, c] = 255
                got = abi.resolve_box(s, ss)
                want = np.zeros((3, 5, 4), np.uint8)
                want[1, 2, c] = (255 + n // 2) // n
                assert np.array_equal(got, want), (ss, j, i, c)
    assert [(255 + k * k // 2) // (k * k) for k in (1, 2, 3, 4)] == [255, 64, 28, 16]


@pytest.mark.parametrize("ss", [2, 4])
def test_ties_round_up(pkg, ss):
    """Sums of exactly (k + 1/2) ss^2 (a tie of the average) give k + 1."""
    abi = pkg.abi
    n = ss * ss
    for k in (0, 1, 100, 254):
        total = k * n + n // 2  # the average is k + 0.5
        s = np.full((ss, ss, 4), k, np.uint8)
        flat = s.reshape(-1, 4)
        flat[:n // 2] += 1
        assert int(flat[:, 0].astype(int).sum()) == total
        assert (abi.resolve_box(s, ss) == k + 1).all(), (ss, k)
        # one below the tie rounds down
        flat[0] -= 1
        assert (abi.resolve_box(s, ss) == k).all(), (ss, k)
    # the tie reached by one large sample
    s = np.zeros((ss, ss, 4), np.uint8)
    s[ss - 1, ss - 1] = n // 2
    assert (abi.resolve_box(s, ss) == 1).all()


def test_rejections(pkg):
    abi, lib = pkg.abi, pkg.abi.load()
    INV = abi.SR_E_INVALID
    w, rows = 5, 3
    for ss in (0, 5, -1):
        src = np.zeros((max(1, abs(ss)) * rows, max(1, abs(ss)) * w, 4), np.uint8)
        dst = np.full((rows, w, 4), SENTINEL, np.uint8)
        assert lib.sr_resolve_box(src.ctypes.data, src.shape[1] * 4, 0, w, rows, ss, dst.ctypes.data, 4 * w, 0, 1, 0,
                                  None) == INV
        assert (dst == SENTINEL).all()
    ss = 2
    src = np.zeros((ss * rows, ss * w, 4), np.uint8)
    dst = np.full((rows, w, 4), SENTINEL, np.uint8)
    sp, op = 4 * ss * w, 4 * w

    def call(s=src.ctypes.data, d=dst.ctypes.data, sp_=sp, op_=op, w_=w, rows_=rows, n=1, sfs=0, ofs=0, dev=0):
        return lib.sr_resolve_box(s, sp_, sfs, w_, rows_, ss, d, op_, ofs, n, dev, None)

    assert call(s=None) == INV and call(d=None) == INV
    assert call(s=None, dev=1) == INV and call(d=None, dev=1) == INV  # checked before any device call
    assert call(op_=op - 1) == INV and call(sp_=sp - 1) == INV  # a pitch below 4 width (x ss)
    assert call(w_=0) == INV and call(rows_=-1) == INV and call(n=0) == INV
    assert call(n=2, sfs=sp * ss * rows, ofs=op * rows - 1) == INV  # frames would overlap
    assert call(n=2, sfs=sp * ss * rows - 1, ofs=op * rows) == INV
    assert (dst == SENTINEL).all()
    assert call(rows_=0) == abi.SR_OK and (dst == SENTINEL).all()
    assert call() == abi.SR_OK and (dst == 0).all()
    assert abi.MAX_SUPERSAMPLE == 4


def hand_costs(sample_costs, ss, height):
    out = []
    nb_sample = (ss * height + 7) // 8
    for b in range((height + 7) // 8):
        total = 0.0
        for k in range(ss * b, ss * b + ss):
            if k < nb_sample:
                total += float(sample_costs[k])
        out.append(total)
    return out


@pytest.mark.parametrize("height", [8, 16, 64, 1, 7, 11, 28, 44, 1080])
@pytest.mark.parametrize("ss", [1, 2, 3, 4])
def test_supersample_block_costs(pkg, ss, height):
    D = pkg.dist
    ns = (ss * height + 7) // 8
    sample = np.random.default_rng(height * 10 + ss).integers(1, 5000, ns).astype(np.float64)
    got = D.supersample_block_costs(sample, ss, height)
    want = hand_costs(sample, ss, height)
    assert got.dtype == np.float64 and got.shape == ((height + 7) // 8,)
    assert got.tolist() == want
    # every sample block is priced exactly once
    assert got.sum() == pytest.approx(sample.sum(), rel=1e-12)
    if ss == 1:
        assert got.tolist() == sample.tolist()
    # 16-row output blocks: pairs of the 8-row ones
    g16 = D.supersample_block_costs(sample, ss, height, block_rows=16)
    pairs = [sum(want[i:i + 2]) for i in range(0, len(want), 2)]
    assert g16.tolist() == pytest.approx(pairs, rel=1e-12)
    with pytest.raises(ValueError):
        D.supersample_block_costs(sample[:-1] if ns > 1 else np.zeros(2), ss, height)
    with pytest.raises(ValueError):
        D.supersample_block_costs(sample, ss, height, block_rows=12)
