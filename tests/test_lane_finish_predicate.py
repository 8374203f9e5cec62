"""certain_end (geodesic.hip): a reseed it accepts ends the ray.

The coasting loop parks a lane below u_f without running its reseed when
certain_end(u, up, uf_radius2) holds, and computes its last chord later. That
is only right if the reseed would have returned a status, i.e. if
sphere_lambda_r2 on the materialised chord finds no positive root (DESIGN.md
§5 "A certain end" has the proof). Here the kernel's point_at, settle_prev and
sphere_lambda_r2 are emulated in numpy binary32, one rounding per operation in
the kernel's order, over more than a million sampled chords and over chords
placed at the predicate's thresholds: no accepted sample may hit the sphere.
"""
import numpy as np

F = np.float32
DELTA = F(1.0 - 2.0 ** -10)  # SR_END_DELTA
R2LIM = F(1.0 - 2.0 ** -9)   # SR_END_R2
UMIN = F(2.0 ** -40)


def certain_end(u, up, r2):
    """The kernel's expression, binary32 (false for NaN operands)."""
    with np.errstate(all="ignore"):
        return (u >= UMIN) & (u < F(1.0)) & (up < F(1.0e30)) & ((u * u) * r2 < R2LIM) & (u <= up * DELTA)


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def nrm(a):
    k = F(1.0) / np.sqrt(dot(a, a))
    return [a[0] * k, a[1] * k, a[2] * k]


def cross(a, b):
    return [a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1]]


def point_at(nv, tv, u, c, s):
    return [(nv[k] * c + tv[k] * s) / u for k in range(3)]


def reseed_hits(nv, tv, u, up, c1, s1, c2, s2, r2):
    """settle_prev's chord from `up` to `u`, then sphere_lambda_r2 about the
    origin with max_lambda = -1: True where the reseed would go on."""
    with np.errstate(all="ignore"):
        A = point_at(nv, tv, up, c2, s2)
        B = point_at(nv, tv, u, c1, s1)
        delta = [B[k] - A[k] for k in range(3)]
        seg = np.sqrt(dot(delta, delta))
        d = [delta[k] / seg for k in range(3)]
        oc = [B[k] - F(0.0) for k in range(3)]
        b = dot(d, oc)
        D = b * b - dot(oc, oc) + r2
        sq = np.sqrt(D)
        first = -dot(d, oc)
        l1, l2 = first - sq, first + sq
        lam = np.full(u.shape, -1.0, dtype=F)
        both = (l1 > 0) & (l2 > 0)
        lam = np.where(both, np.where(l2 < l1, l2, l1), np.where(l1 > 0, l1, np.where(l2 > 0, l2, lam)))
        return ~(D < 0) & (lam >= 0)


def frames(rng, n, skew):
    """Orbital frames as the kernel builds them (nv = nrm(position), tv =
    nrm(cross(cross(nv, d), nv))), optionally off orthonormal by `skew`."""
    p = [rng.standard_normal(n).astype(F) for _ in range(3)]
    d = [rng.standard_normal(n).astype(F) for _ in range(3)]
    nv = nrm(p)
    tv = nrm(cross(cross(nv, d), nv))
    if skew:
        e = [(skew * rng.standard_normal(n)).astype(F) for _ in range(3)]
        tv = [tv[k] + e[k] * nv[k] + e[(k + 1) % 3] for k in range(3)]
    return nv, tv


def angles(rng, n):
    phi = rng.uniform(0.0, 4.0 * np.pi, n)
    dphi = 10.0 ** rng.uniform(-4.0, -0.5, n)  # 8000 steps of one revolution .. 20 steps of two
    return (np.cos(phi).astype(F), np.sin(phi).astype(F), np.cos(phi - dphi).astype(F), np.sin(phi - dphi).astype(F))


def check(nv, tv, u, up, cs, r2, what):
    ok = certain_end(u, up, r2)
    hit = reseed_hits(nv, tv, u, up, *cs, r2)
    bad = ok & hit
    assert not bad.any(), (f"{what}: {int(bad.sum())} accepted chords re-enter the sphere, first u={u[bad][0]!r} "
                           f"up={up[bad][0]!r} r2={r2[bad][0]!r}")
    return ok, hit


def uf_r2(u_f):
    r = F(1.0) / u_f.astype(F)
    return r * r


def test_accepts_nothing_without_a_positive_finite_u():
    bad_u = np.array([0.0, -0.0, -1.0e-3, -np.inf, np.inf, np.nan, 1.0, 2.0, 2.0 ** -41, 1.0e-45], dtype=F)
    for up in (F(0.5), F(np.inf), F(np.nan), F(1.0e-3)):
        for r2 in (F(1.0e4), F(0.0), F(np.inf), F(np.nan)):
            assert not certain_end(bad_u, np.full_like(bad_u, up), np.full_like(bad_u, r2)).any()
    good_u = np.full(5, 0.005, dtype=F)
    bad_up = np.array([np.nan, np.inf, 1.0e30, -1.0, 0.005], dtype=F)
    assert not certain_end(good_u, bad_up, np.full_like(good_u, 1.0e4)).any()
    bad_r2 = np.array([np.nan, np.inf, 4.0e4, 3.9937e4, 1.0e38], dtype=F)  # 0.005^-2 = 4e4: the sphere's edge
    assert not certain_end(good_u, np.full_like(good_u, 0.01), bad_r2).any()
    assert certain_end(F(0.005), F(0.00501), F(1.0e4))


def test_sampled_chords():
    rng = np.random.default_rng(20240611)
    n = 1 << 18
    total = accepted = 0
    rejected_hits = 0
    for rnd in range(6):
        nv, tv = frames(rng, n, [0.0, 0.0, 1.0e-6, 3.0e-6, 0.0, 1.0e-6][rnd])
        cs = angles(rng, n)
        if rnd < 4:   # escaping rays: u falls by 1e-5 .. 50 % per step, the sphere anywhere outside u
            u = (10.0 ** rng.uniform(-4.0, -0.22, n)).astype(F)
            up = (u.astype(np.float64) * (1.0 + 10.0 ** rng.uniform(-5.0, -0.3, n))).astype(F)
            u_f = (u.astype(np.float64) * (1.0 + 10.0 ** rng.uniform(-6.0, 0.0, n))).astype(F)
        elif rnd == 4:  # the whole range the predicate lets in
            u = (2.0 ** rng.uniform(-41.0, 0.0, n)).astype(F)
            up = (u.astype(np.float64) * (1.0 + 10.0 ** rng.uniform(-4.0, 3.0, n))).astype(F)
            u_f = (u.astype(np.float64) * 10.0 ** rng.uniform(-3.0, 3.0, n)).astype(F)
        else:  # chords heading back in, below u_f: the reseeds that go on
            u = (10.0 ** rng.uniform(-3.0, -0.5, n)).astype(F)
            up = (u.astype(np.float64) * rng.uniform(0.3, 1.001, n)).astype(F)
            u_f = (u.astype(np.float64) * (1.0 + 10.0 ** rng.uniform(-3.0, 0.0, n))).astype(F)
        ok, hit = check(nv, tv, u, up, cs, uf_r2(u_f), f"round {rnd}")
        total += n
        accepted += int(ok.sum())
        rejected_hits += int((hit & ~ok).sum())
    assert total >= 10 ** 6
    assert accepted > total // 4     # the predicate is not vacuous
    assert rejected_hits > 1000      # and the emulation does find the sphere where a chord heads back in


def test_chords_at_the_thresholds():
    """u within a few ulps of up (1 - 2^-10), u^2 r2 within a few ulps of
    1 - 2^-9, both at once, u just below u_f, the smallest u let in and u
    next to 1."""
    rng = np.random.default_rng(7)
    n = 1 << 16
    steps = np.arange(-4, 5)

    def ulps(x, k):
        x = x.copy()
        for _ in range(abs(k)):
            x = np.nextafter(x, F(np.inf) if k > 0 else F(-np.inf))
        return x

    accepted = 0
    for k in steps:
        nv, tv = frames(rng, n, 1.0e-6 if k % 2 else 0.0)
        cs = angles(rng, n)
        up = (10.0 ** rng.uniform(-4.0, -0.25, n)).astype(F)
        u_edge = ulps(up * DELTA, int(k))                     # u at the ratio's threshold
        u_f = (u_edge.astype(np.float64) * (1.0 + 10.0 ** rng.uniform(-6.0, 0.0, n))).astype(F)
        accepted += int(check(nv, tv, u_edge, up, cs, uf_r2(u_f), f"ratio {k:+d} ulp")[0].sum())
        u = (10.0 ** rng.uniform(-4.0, -0.25, n)).astype(F)
        r2_edge = ulps((R2LIM.astype(np.float64) / (u.astype(np.float64) ** 2)).astype(F), int(k))  # r2 at its threshold
        up2 = (u.astype(np.float64) * (1.0 + 10.0 ** rng.uniform(-5.0, -0.3, n))).astype(F)
        accepted += int(check(nv, tv, u, up2, cs, r2_edge, f"radius {k:+d} ulp")[0].sum())
        up3 = ulps(u / DELTA, int(k))                         # both at once
        accepted += int(check(nv, tv, u, up3, cs, r2_edge, f"both {k:+d} ulp")[0].sum())
        uf4 = (10.0 ** rng.uniform(-3.0, -0.3, n)).astype(F)  # u just below u_f: never accepted, whatever up
        u4 = ulps(uf4, -1 - abs(int(k)))
        ok4, _ = check(nv, tv, u4, up2 / u * u4, cs, uf_r2(uf4), f"u_f {k:+d} ulp")
        assert not ok4.any()
    tiny = ulps(np.full(n, UMIN, dtype=F), 0)
    nv, tv = frames(rng, n, 0.0)
    cs = angles(rng, n)
    for u in (tiny, ulps(np.ones(n, dtype=F), -1)):
        up = (u.astype(np.float64) * (1.0 + 10.0 ** rng.uniform(-3.1, 2.0, n))).astype(F)
        for scale in (1.0e-6, 0.5, 0.99, 1.0):
            r2 = (scale / u.astype(np.float64) ** 2).astype(F)
            accepted += int(check(nv, tv, u, up, cs, r2, "range ends")[0].sum())
    assert accepted > 100000
