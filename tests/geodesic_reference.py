"""Schwarzschild null geodesics in binary64, a numpy model of the shader's
walk, and the lens-map ray set (a helper, not a test module).

Every other helper here ties the kernels to the CPU oracle and the oracle to
the reference shader. This one ties the scheme to the physics: where a ray
ends, by the photon Binet equation u'' = -u (1 - 1.5 u), u = 1 / r, r_s = 1.

exact(O, V, ...)   the reference. The ray's plane is spanned by n = O / |O|
    and t = normalize((n x V) x n); u0 = 1 / |O|, u0' = -u0 (V.n) / (V.t).
    (u, u') is integrated over phi by scipy's DOP853 (rtol 1e-13) with
    terminal events: u rises to 1 (captured), u falls through u_f (escaped),
    phi reaches 2 pi max_revolutions (out of angle). Beyond r = 1 / u_f space
    is flat, as the shader defines it: an origin out there travels straight to
    that sphere and the geodesic starts at the entry point; a line that misses
    it stays a line. The angle psi between V and -n is a coordinate angle:
    1 / b^2 = u0'^2 + u0^2 - u0^3 = u0^2 / sin^2 psi - u0^3.

model(O, V, ...)   the shader's walk (oracle/sr_oracle.c
    shade) restated in numpy over all rays at once, in float32 or float64.
    In float32 it follows the oracle's operation order, so it draws its
    rounding from the oracle's distribution; it is not bit-exact (numpy may
    contract or reorder nothing, but the oracle's compiler may), and nothing
    relies on that. In float64 it isolates the scheme's truncation.

ray_set()          the deterministic set, <= 2048 rays.

fit(err, s)        the rule by which tests/golden/make_lens_reference.py turns
    the float32 model's measured errors into the tolerance eps + delta s.

Lens               the set with its reference (computed, or as recorded in
    tests/golden/lens_reference.npz), the ray classes of the tests and the
    models, made once per session.
"""
from __future__ import annotations

import math

import numpy as np

B_CRIT = 1.5 * math.sqrt(3.0)
CAPTURED, SKY, OUT_OF_ANGLE, SURFACE = 0, 1, 2, 3
PI_F = 3.1415926535  # frag:10
EPSILON = 0.0000001  # frag: EPSILON
RADII = (4.0, 20.0, 60.0)
REL_H = 1.0e-6  # the sensitivity's relative step in b

R0 = (1.2, 1.45, 1.5, 1.55, 2.0, 3.0, 5.0, 10.0, 30.0, 60.0, 99.0, 150.0, 1000.0)
OFFSETS = (-1e-4, 1e-4, -1e-3, 1e-3, -1e-2, 1e-2, -1e-1, 1e-1, 0.3, 1.0, 3.0, 10.0)
STEEP = (0.05, 0.3, 0.7)  # b / b_crit of the steep rays
NEAR_MAX = (0.9, 0.99, 0.999)  # b / b_max
MAX_B_SHARE = 1.0 - 1.0e-4  # no listed b above this share of the largest b the origin admits
COPIES = 3  # rotations per (r0, b, branch)
N_NEAR_RADIAL = N_FLAT = 64
U_F = 0.01


# ---- the exact reference ----------------------------------------------------------------
def _rhs(phi, y):
    return (y[1], -y[0] * (1.0 - 1.5 * y[0]))


def _unit(v):
    return v / np.sqrt(np.dot(v, v))


def frame(O, V):
    """(n, t, u0, du0) of a ray, binary64."""
    O, V = np.asarray(O, dtype=np.float64), np.asarray(V, dtype=np.float64)
    n = _unit(O)
    d = _unit(V)
    t = _unit(np.cross(np.cross(n, d), n))
    u0 = 1.0 / math.sqrt(float(np.dot(O, O)))
    return n, t, u0, -u0 * float(np.dot(d, n)) / float(np.dot(d, t))


def impact_parameter(u0, du0):
    return 1.0 / math.sqrt(du0 * du0 + u0 * u0 - u0 * u0 * u0)


def planar(u0, du0, u_f, phi_max, ends=(), radii=(), rtol=1e-13, atol=1e-15, path=False):
    """The geodesic in its plane from (u0, du0) at phi = 0 ->
    (class, phi_exit, u, u' at exit, [(phi, u, u') at each of `ends` (angles
    <= phi_max; the exit's own values where the ray ended sooner)],
    [phi at which u first falls through 1 / R for R in radii, NaN if never]);
    with path, the integrator's own points (phi [n], y [2, n]) as a seventh."""
    from scipy.integrate import solve_ivp

    def captured(phi, y):
        return y[0] - 1.0

    def escaped(phi, y):
        return y[0] - u_f

    captured.terminal, captured.direction = True, 1.0
    escaped.terminal, escaped.direction = True, -1.0
    events = [captured, escaped]
    for R in radii:
        def crossing(phi, y, R=R):
            return y[0] - 1.0 / R
        crossing.terminal, crossing.direction = False, -1.0
        events.append(crossing)
    sol = solve_ivp(_rhs, (0.0, phi_max), (u0, du0), method="DOP853", rtol=rtol, atol=atol, events=events,
                    dense_output=bool(ends))
    assert sol.status in (0, 1), sol.message
    if sol.status == 1 and len(sol.t_events[0]):
        cls, phi, y = CAPTURED, float(sol.t_events[0][0]), sol.y_events[0][0]
    elif sol.status == 1:
        cls, phi, y = SKY, float(sol.t_events[1][0]), sol.y_events[1][0]
    else:
        cls, phi, y = OUT_OF_ANGLE, float(sol.t[-1]), sol.y[:, -1]
    at = []
    for e in ends:
        if e < phi:
            ye = sol.sol(e)
            at.append((OUT_OF_ANGLE, float(e), float(ye[0]), float(ye[1])))
        else:
            at.append((cls, phi, float(y[0]), float(y[1])))
    cross = [float(ev[0]) if len(ev) else math.nan for ev in sol.t_events[2:]]
    out = (cls, phi, float(y[0]), float(y[1]), at, cross)
    return out + ((sol.t, sol.y),) if path else out


def tangent(n, t, phi, u, du):
    """The unit tangent of (cos phi n + sin phi t) / u, scaled by u^2 so that u = 0 is regular."""
    c, s = math.cos(phi), math.sin(phi)
    return _unit(u * (-s * n + c * t) - du * (c * n + s * t))


def enter(O, V, u_f):
    """The flat exterior: (start point, straight) of a ray, binary64. An origin
    beyond r = 1 / u_f moves along V to that sphere; straight = it misses."""
    O = np.asarray(O, dtype=np.float64)
    if u_f <= 0.0 or float(np.dot(O, O)) * u_f * u_f <= 1.0:
        return O, False
    d = _unit(np.asarray(V, dtype=np.float64))
    b = float(np.dot(d, O))
    D = b * b - float(np.dot(O, O)) + 1.0 / (u_f * u_f)
    if D < 0.0 or -b - math.sqrt(D) <= 0.0:
        return O, True
    return O + d * (-b - math.sqrt(D)), False


def exact(O, V, u_f=U_F, max_revolutions=(2,), radii=RADII, sensitivity=True):
    """The reference of one ray -> dict:
      b, phi_exit, du_exit (u' there), class [per max_revolutions], tangent [per max_revolutions, 3],
      phi_end [per max_revolutions] (the angle at which that launch's ray ends),
      s [per max_revolutions] (|d exit angle / d ln b|, NaN where the class
      changes within b (1 +- REL_H) or the ray is captured),
      cross [per R, 3] and s_cross [per R] (first point at r = R, NaN if none
      or if the origin is not inside R), plane [3] (the orbital plane's normal),
      straight (a flat ray: tangent = normalize(V), b = NaN).
    max_revolutions is sorted ascending; the integration runs once, to the largest."""
    revs = tuple(max_revolutions)
    assert revs == tuple(sorted(revs))
    nr, nR = len(revs), len(radii)
    out = {"b": math.nan, "phi_exit": math.nan, "du_exit": math.nan, "class": np.full(nr, SKY, dtype=np.int8),
           "tangent": np.full((nr, 3), np.nan), "phi_end": np.full(nr, np.nan), "s": np.full(nr, np.nan),
           "cross": np.full((nR, 3), np.nan), "s_cross": np.full(nR, np.nan), "plane": np.full(3, np.nan),
           "straight": False}
    V = np.asarray(V, dtype=np.float64)
    P, straight = enter(O, V, u_f)
    if straight:
        out["straight"] = True
        out["tangent"][:] = _unit(V)
        return out
    n, t, u0, du0 = frame(P, V)
    out["plane"] = np.cross(n, t)
    ends = [2.0 * math.pi * r for r in revs]
    inside = [R for R in radii if u0 * R > 1.0]

    def run(u0_, du0_):
        return planar(u0_, du0_, u_f, ends[-1], ends, inside)

    cls, phi, u, du, at, cross = run(u0, du0)
    b = impact_parameter(u0, du0)
    out["b"], out["phi_exit"], out["du_exit"] = b, phi, du
    tang = [tangent(n, t, a[1], a[2], a[3]) for a in at]
    for k, a in enumerate(at):
        out["class"][k], out["phi_end"][k], out["tangent"][k] = a[0], a[1], tang[k]
    kR = [radii.index(R) for R in inside]
    for j, k in enumerate(kR):
        if not math.isnan(cross[j]):
            out["cross"][k] = radii[k] * (math.cos(cross[j]) * n + math.sin(cross[j]) * t)
    if not sensitivity:
        return out
    side = []
    for h in (-REL_H, REL_H):
        e = 1.0 / (b * (1.0 + h)) ** 2 - u0 * u0 + u0 * u0 * u0
        if e < 0.0:
            return out
        side.append(run(u0, math.copysign(math.sqrt(e), du0)))
    for k in range(nr):
        a0, a1 = side[0][4][k], side[1][4][k]
        if a0[0] == a1[0] == at[k][0] != CAPTURED:
            d0, d1 = tangent(n, t, *a0[1:]), tangent(n, t, *a1[1:])
            out["s"][k] = math.atan2(float(np.linalg.norm(np.cross(d0, d1))), float(np.dot(d0, d1))) / (2.0 * REL_H)
    for j, k in enumerate(kR):
        out["s_cross"][k] = abs(side[1][5][j] - side[0][5][j]) / (2.0 * REL_H)
    return out


def exact_set(O, V, u_f=U_F, max_revolutions=(1, 2, 4), radii=RADII, select=None):
    """exact() over rays -> dict of stacked arrays (rows of `select` only, if given)."""
    idx = range(len(O)) if select is None else select
    rows = [exact(O[i], V[i], u_f, max_revolutions, radii) for i in idx]
    return {k: np.stack([np.asarray(r[k]) for r in rows]) for k in rows[0]}


def analytic_class(O, V, u_f=U_F):
    """Captured or not from b, the origin's side of the photon sphere and the
    branch alone (binary64): outside r = 1.5 a ray is captured iff b < b_crit
    and it heads inward; inside, iff it heads inward or b > b_crit (it turns
    back). Straight rays escape."""
    P, straight = enter(O, V, u_f)
    if straight:
        return SKY
    n, t, u0, du0 = frame(P, V)
    b = impact_parameter(u0, du0)
    inward = du0 > 0.0
    if u0 < 1.0 / 1.5:
        return CAPTURED if (b < B_CRIT and inward) else SKY
    return CAPTURED if (inward or b > B_CRIT) else SKY


# ---- the scheme model -------------------------------------------------------------------
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _norm(a):
    return a * (a.dtype.type(1.0) / np.sqrt(_dot(a, a)))[..., None]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _sphere(o, d, radius, max_lambda):
    """sphere_intersect (frag:457-478) of a sphere at the origin -> (hit, point, dist)."""
    T = o.dtype.type
    b = _dot(d, o)
    D = b * b - _dot(o, o) + T(radius) * T(radius)
    sq = np.sqrt(np.where(D < 0, T(0), D))
    first = -_dot(d, o)
    l1, l2 = first - sq, first + sq
    lam = np.where((l1 > 0) & (l2 > 0), np.minimum(l1, l2), np.where(l1 > 0, l1, np.where(l2 > 0, l2, T(-1.0))))
    hit = (D >= 0) & (lam >= 0) & ((max_lambda < 0) | (lam <= max_lambda))
    p = o + d * lam[..., None]
    q = p - o
    return hit, p, np.sqrt(_dot(q, q))


def model(O, V, max_steps, max_revolutions=2, u_f=U_F, dtype=np.float32, radius=None):
    """The shader's walk of rays (O, V as the kernel gets them: float32, taken
    to dtype) in a scene of the hole and, with radius, one opaque sphere of
    that radius about it -> dict: class [N] (CAPTURED, SKY, OUT_OF_ANGLE or
    SURFACE), dir [N, 3] (get_bg's argument where the class is SKY or
    OUT_OF_ANGLE), hit_point, hit_view [N, 3] (SURFACE), steps [N]."""
    assert np.dtype(dtype) in (np.dtype(np.float32), np.dtype(np.float64))
    T = np.dtype(dtype).type
    with np.errstate(all="ignore"):
        o = np.asarray(O, dtype=np.float32).astype(dtype)
        d = _norm(np.zeros(3, dtype=dtype) + np.asarray(V, dtype=np.float32).astype(dtype))
        N = len(o)
        cls = np.full(N, -1, dtype=np.int8)
        out_dir = np.full((N, 3), np.nan, dtype=dtype)
        hit_point = np.full((N, 3), np.nan, dtype=dtype)
        hit_view = np.full((N, 3), np.nan, dtype=dtype)
        steps = np.zeros(N, dtype=np.int32)

        def intersect(k, oo, dd, max_lambda):
            """intersect() for rays k (indices): the hole, then the sphere if nearer; ends those that hit."""
            hit, p, dist = _sphere(oo, dd, 1.0, max_lambda)
            surface = np.zeros(len(k), dtype=bool)
            if radius is not None:
                h2, p2, dist2 = _sphere(oo, dd, radius, max_lambda)
                surface = h2 & (~hit | (dist2 < dist))
            cls[k[hit & ~surface]] = CAPTURED
            cls[k[surface]] = SURFACE
            if radius is not None:
                hit_point[k[surface]] = p2[surface]
                hit_view[k[surface]] = -dd[surface]
            return hit | surface

        def flat(k, oo, dd):
            done = intersect(k, oo, dd, T(-1.0))
            cls[k[~done]] = SKY
            out_dir[k[~done]] = dd[~done]

        n = _norm(o)
        radial = np.abs(_dot(d, n)) >= T(1.0) - T(EPSILON)
        k = np.flatnonzero(radial)
        flat(k, o[k], d[k])
        t = _norm(_cross(_cross(n, d), n))
        u = T(1.0) / np.sqrt(_dot(o, o))
        du = -u * _dot(d, n) / _dot(d, t)
        phi = np.zeros(N, dtype=dtype)
        max_angle = T(2.0) * T(max_revolutions) * T(PI_F)
        uf, uf_radius = T(u_f), T(1.0) / T(u_f)
        for i in range(max_steps):
            live = cls < 0
            if not live.any():
                break
            steps[live] += 1
            k = np.flatnonzero(live & (u < uf))
            if len(k):
                hit, p, _ = _sphere(o[k], d[k], uf_radius, T(-1.0))
                flat(k[~hit], o[k][~hit], d[k][~hit])
                k, p = k[hit], p[hit]
                nn = _norm(p)
                rad = np.abs(_dot(d[k], nn)) >= T(1.0) - T(EPSILON)
                flat(k[rad], o[k][rad], d[k][rad])
                k, p, nn = k[~rad], p[~rad], nn[~rad]
                n[k] = nn
                t[k] = _norm(_cross(_cross(nn, d[k]), nn))
                u[k] = T(1.0) / np.sqrt(_dot(p, p))
                du[k] = -u[k] * _dot(d[k], nn) / _dot(d[k], t[k])
            k = np.flatnonzero(cls < 0)
            h = (max_angle - phi[k]) / T(max_steps - i)
            phi[k] += h
            uk, dk = u[k], du[k]

            def ddu(x):
                return -x * (T(1.0) - T(1.5) * x)

            k1, l1 = dk, ddu(uk)
            k2, l2 = dk + T(0.5) * l1 * h, ddu(uk + T(0.5) * k1 * h)
            k3, l3 = dk + T(0.5) * l2 * h, ddu(uk + T(0.5) * k2 * h)
            k4, l4 = dk + l3 * h, ddu(uk + k3 * h)
            uk = uk + h / T(6.0) * (k1 + T(2.0) * k2 + T(2.0) * k3 + k4)
            dk = dk + h / T(6.0) * (l1 + T(2.0) * l2 + T(2.0) * l3 + l4)
            u[k], du[k] = uk, dk
            neg = uk < 0
            cls[k[neg]] = SKY  # the break: get_bg of the direction the ray had
            out_dir[k[neg]] = d[k[neg]]
            k, uk = k[~neg], uk[~neg]
            ph = phi[k].astype(np.float64)
            c, s = np.cos(ph).astype(dtype), np.sin(ph).astype(dtype)
            prev = o[k]
            new = (n[k] * c[:, None] + t[k] * s[:, None]) / uk[:, None]
            delta = new - prev
            length = np.sqrt(_dot(delta, delta))
            dd = delta / length[:, None]
            o[k], d[k] = new, dd
            intersect(k, prev, dd, length)
        k = np.flatnonzero(cls < 0)
        cls[k] = OUT_OF_ANGLE
        out_dir[k] = d[k]
    return {"class": cls, "dir": out_dir, "hit_point": hit_point, "hit_view": hit_view, "steps": steps}


# ---- the ray set ------------------------------------------------------------------------
def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def b_max(r0):
    """The largest impact parameter a ray through radius r0 can have (a tangential one)."""
    return r0 / math.sqrt(1.0 - 1.0 / r0)


def _plane_ray(r0, b, inward, u_f):
    """(O, V) in the x-y plane of the ray whose geodesic has impact parameter
    b: from r0 on the x axis, or, for r0 beyond 1 / u_f, aimed from there so
    that it enters the 1 / u_f sphere with that b."""
    rs = min(r0, 1.0 / u_f)  # the radius at which the geodesic starts
    us = 1.0 / rs
    sin_psi = us / math.sqrt(1.0 / (b * b) + us ** 3)
    if r0 > rs:
        sin_psi *= rs / r0  # the same line seen from r0
    cos_psi = math.sqrt(1.0 - sin_psi * sin_psi)
    return np.array([r0, 0.0, 0.0]), np.array([-cos_psi if inward else cos_psi, sin_psi, 0.0])


def ray_set(u_f=U_F, seed=2024):
    """(O [N, 3], V [N, 3]) float32 and kind [N] ("grid", "near-radial", "flat")."""
    rng = np.random.default_rng(seed)
    O, V, kind = [], [], []

    def add(o, v, what):
        q = _rotation(rng)
        O.append(q @ o)
        V.append(q @ v * 10.0 ** rng.uniform(-3.0, 3.0))
        kind.append(what)

    for r0 in R0:
        top = b_max(min(r0, 1.0 / u_f))
        bs = [B_CRIT * (1.0 + x) for x in OFFSETS] + [B_CRIT * x for x in STEEP] + [top * x for x in NEAR_MAX]
        for b in sorted(set(x for x in bs if x <= top * MAX_B_SHARE)):
            for inward in (True, False):
                if r0 * u_f > 1.0 and not inward:
                    continue  # from beyond 1 / u_f only the inward branch meets the geodesic
                for _ in range(COPIES):
                    add(*_plane_ray(r0, b, inward, u_f), "grid")
    for _ in range(N_NEAR_RADIAL):
        r0 = R0[int(rng.integers(len(R0) - 2))]
        a = 10.0 ** rng.uniform(-3.0, -1.0) * 1.5  # the angle off the radius, > 1e-3
        sgn = -1.0 if rng.random() < 0.5 else 1.0
        add(np.array([r0, 0.0, 0.0]), np.array([sgn * math.cos(a), math.sin(a), 0.0]), "near-radial")
    for _ in range(N_FLAT):
        r0 = (1.0 / u_f) * 10.0 ** rng.uniform(0.01, 2.0)
        # aimed to pass the 1 / u_f sphere at 1.05 to 3 times its radius, or outward
        miss = (1.0 / u_f) * rng.uniform(1.05, 3.0)
        if miss < r0 and rng.random() < 0.7:
            s = miss / r0
            v = np.array([-math.sqrt(1.0 - s * s), s, 0.0])
        else:
            a = rng.uniform(0.0, 0.45 * math.pi)
            v = np.array([math.cos(a), math.sin(a), 0.0])
        add(np.array([r0, 0.0, 0.0]), v, "flat")
    O, V = np.array(O).astype(np.float32), np.array(V).astype(np.float32)
    assert len(O) <= 2048 and not (np.signbit(V) & (V == 0)).any()
    return O, V, np.array(kind)


def angle_between(a, b):
    """The angle between directions [..., 3], binary64, accurate near 0."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), np.sum(a * b, axis=-1))


FORMAT_FLOOR = 2.0 ** -21  # rad: a normalised float32 direction, four roundings of 2^-24 on each of three components


def fit(err, s):
    """The (eps, delta) covering err <= eps + delta s by the rule written here
    (the pairs that cover are many): the one with the least tolerance summed
    over the decades the fitted rays' sensitivities span, the integral of
    eps + delta s over ln s from min(s) to max(s). That is
    eps + delta a, a = (max - min) / ln(max / min), up to a factor, and with
    eps(delta) = max(err - delta s), the least floor a slope admits, it is
    convex in delta with the slope a - s[argmax]: bisection on that sign finds
    its minimum. eps is never below what the number format costs."""
    err, s = np.asarray(err, dtype=np.float64), np.asarray(s, dtype=np.float64)
    assert np.isfinite(err).all() and np.isfinite(s).all() and (s > 0).all() and (err >= 0).all()
    at = (s.max() - s.min()) / math.log(s.max() / s.min())
    lo, hi = 0.0, float(np.max(err / s))
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if s[np.argmax(err - mid * s)] > at:
            lo = mid
        else:
            hi = mid
    return max(float(np.max(err - hi * s)), FORMAT_FLOOR), hi


def exit_chord_term(b, du_exit, max_steps, max_revolutions=2, u_f=U_F):
    """The first-order part of the scheme's exit direction, bounded from the
    reference alone. The shader's sky direction is its last chord, which starts
    inside r = 1 / u_f and ends beyond it, not the tangent where the ray
    crosses that sphere. A chord's direction is the curve's tangent somewhere
    along it, and the tangent's angle theta = phi + atan2(u, -u') turns at
    d theta / d phi = u (u + u'') / (u^2 + u'^2) = 1.5 u^3 / (1 / b^2 + u^3),
    which grows with u. Along the last chord u <= u_f + |u'| dphi, so the
    chord's direction is within dphi times that rate of the tangent at the
    crossing. It matters where the exit grazes the sphere (b near 1 / u_f)."""
    dphi = 2.0 * math.pi * max_revolutions / max_steps
    u = u_f + np.abs(du_exit) * dphi
    return dphi * 1.5 * u ** 3 / (1.0 / np.asarray(b) ** 2 + u ** 3)


def sphere_scene(pkg, radius, color=(0.25, 0.5, 0.75, 1.0)):
    """The hole and one opaque unlit sphere of that radius about it (object 0):
    ambient 1 and no light, so that a hit's FragColor is the colour itself."""
    import extreme_cases as X

    s = X.empty_scene(pkg)
    s.num_lights = 0
    X.plain_material(s.materials[0], color)
    m = s.materials[0]
    m.ambient, m.diffuse, m.specular = 1.0, 0.0, 0.0
    return X.append_primitive(s, {"type": "sphere", "pos": (0.0, 0.0, 0.0), "radius": float(radius)})


def bins(x):
    """The table's rows: the index into BIN_EDGES' intervals of |b / b_crit - 1|."""
    return np.digitize(np.abs(x), BIN_EDGES) - 1


BIN_EDGES = (0.0, 3e-4, 3e-3, 3e-2, 0.3, 3.0, 1e9)
BIN_NAMES = ("1e-4", "1e-3", "1e-2", "1e-1", "0.3 .. 3", "> 3")


def error_table(err, s, x):
    """[(row name, rays, max, median, max of err / s, median of err / s)] by |b / b_crit - 1|."""
    err, s, k = np.asarray(err), np.asarray(s), bins(x)
    out = []
    for i, name in enumerate(BIN_NAMES):
        m = k == i
        if m.any():
            q = err[m] / s[m]
            out.append((name, int(m.sum()), float(err[m].max()), float(np.median(err[m])), float(q.max()),
                        float(np.median(q))))
    return out


# ---- the set with its reference -----------------------------------------------------------
LEVEL_C_STEPS = 2000
TRUNCATION_STEPS = (64, 128, 256, 512, 2000)
LEVEL_B_STEPS = (64, 256, 2000)
REVOLUTIONS = (1, 2, 4)
MAX_LATE_SHARE = 0.02
GOLDEN = "lens_reference.npz"
TOLERANCES = "lens_tolerances.json"


def ends_in_sky(cls):
    return (cls == SKY) | (cls == OUT_OF_ANGLE)


class Lens:
    """The ray set, its reference (computed, or as tests/golden holds it) and the models of it, made once."""

    _models = {}

    def __init__(self, O, V, ref):
        self.O, self.V, self.ref = O, V, ref
        self.r0 = np.linalg.norm(O.astype(np.float64), axis=-1)
        self.straight = ref["straight"].astype(bool)
        self.beyond = (self.r0 * U_F > 1.0) & ~self.straight
        self.x = ref["b"] / B_CRIT - 1.0

    @classmethod
    def compute(cls):
        O, V, _ = ray_set()
        ref = exact_set(O, V, U_F, REVOLUTIONS, RADII)
        ref["rays_O"], ref["rays_V"] = O, V
        return cls(O, V, ref)

    @classmethod
    def load(cls):
        from pathlib import Path

        ref = dict(np.load(Path(__file__).resolve().parent / "golden" / GOLDEN))
        O, V, _ = ray_set()
        assert np.array_equal(O, ref["rays_O"]) and np.array_equal(V, ref["rays_V"]), "the golden file is of another set"
        return cls(O, V, ref)

    @staticmethod
    def tolerances():
        import json
        from pathlib import Path

        return json.loads((Path(__file__).resolve().parent / "golden" / TOLERANCES).read_text())

    def cls(self, rev):
        return self.ref["class"][:, REVOLUTIONS.index(rev)]

    def s(self, rev):
        return self.ref["s"][:, REVOLUTIONS.index(rev)]

    def tangent(self, rev):
        return self.ref["tangent"][:, REVOLUTIONS.index(rev)]

    def late(self, steps=LEVEL_C_STEPS, rev=2):
        """Rays that reach neither capture nor 1 / u_f before the launch's last two steps:
        their last chord is no tangent. Left to level B."""
        return ~self.straight & ~(self.ref["phi_exit"] < 2.0 * math.pi * rev * (1.0 - 2.0 / steps))

    def c_rays(self):
        return ~self.straight & ~self.late()

    def c_sky(self):
        return self.c_rays() & (self.cls(2) == SKY)

    def model(self, steps, rev, dtype, radius=None):
        key = (steps, rev, np.dtype(dtype).name, radius)
        if key not in self._models:
            m = model(self.O, self.V, steps, rev, U_F, dtype, radius)
            for a in m.values():
                a.setflags(write=False)
            self._models[key] = m
        return self._models[key]

    def model_flips(self, rev, m64):
        """Rays on which the float64 model's class is not the exact one (to the sky or not)."""
        return ends_in_sky(m64["class"]) != ends_in_sky(self.cls(rev))

    def level_b(self, rev, m64):
        """Level B's direction rays: the float64 model ends in the sky and the reference has a sensitivity."""
        return ends_in_sky(m64["class"]) & np.isfinite(self.s(rev)) & ~self.straight

    def within_radius(self, j):
        return ~self.straight & (self.r0 < 0.99 * RADII[j])  # (an origin at R itself is on either side in float32)

    def flung(self, j, steps=LEVEL_C_STEPS, rev=2):
        """Steep rays the scheme may fling past a surface at r = RADII[j]: the
        walk leaves the loop when a step takes u below 0, before that step's
        chord is tested. With u' about -1 / b a step lowers u by dphi / b,
        which can pass 0 from inside the surface (u > 1 / R) only if
        b < R dphi. Twice that is kept clear of, from the reference alone."""
        return self.ref["b"] < 2.0 * RADII[j] * (2.0 * math.pi * rev / steps)

    def inside_radius(self, j):
        """Origins inside r = RADII[j] whose geodesic reaches it, the flung ones left out."""
        return self.within_radius(j) & np.isfinite(self.ref["cross"][:, j, 0]) & ~self.flung(j)
