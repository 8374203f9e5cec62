"""The exact-by-margin culling bounds of geodesic.hip, each held to its contract
on the device, on inputs built to sit on its edge (tests/bound_cases.py).

`make` also builds lib/libsr_bnd.so: the same kernel source with
-DSR_BOUND_PROBE (csrc/kernels/bound_probe.h), whose sr_debug_probe_* entry
points run one shipping device function per thread on the packed scene image
of sr_debug_pack_scene: the bounds with the device's own sqrt / rcp / rsq and
the packer's own br, rb, mu, mp, qk, flat_miss_r2 and test-ray bounds. What
the step loop keeps wave-uniform (slot, object, reach mask) is a kernel
argument: one launch per slot.

References: oracle.intersect (the oracle's intersect() per chord), the
exhaustive closest_hit_all on the device, and binary64 numpy geometry. Tests 2
to 6 assert a contract - no counter-example - and print the worst ratios they
met (run with -s); DESIGN.md §5 records them.

Worst values met on an MI355X (the device's winners are the oracle's, bit for bit):
  test 2  binary64 distance of an accepted point beyond br, over mu S: 0.092
          (spheres and planar primitives), 1.60 for cylinders (lat_margin's part)
  test_margin_safety_factors  the margin factor a winning chord needs, (its
          binary64 distance from bc - the bare bounding radius) / (1 + |bc|_1 +
          R + S): at most 2.4e-8 for disks, annuli, rectangles and boxes
          (SR_MU_PLANAR is 4000 times that) and 1.6e-4 for spheres
          (SR_MU_QUADRATIC is 12.6 times that); asserted at a quarter of those
          factors, as tests/test_cyl_lateral_margin.py sets its own
  test 4  smallest binary64 distance over clearance: 1.00017

Margins shrunk in a scratch copy of the source (never committed), the module
run on that build of the probe library (SR_BND_LIB), and what fails:
  SR_PATH_SLACK 0.5            test_clearances_are_sound_and_below_the_distance,
                               both test_clearance_tr cases
  SR_MU_PLANAR 1e-7            test_margin_safety_factors (a factor of 4 left
                               where 1000 is asserted). No winning chord is
                               lost even then: binary32 rounding moves these
                               chords by less than 1e-7 S; the factor is what
                               stands between the constant and a miss
  may_hit without lat_margin   test_chord_culling_keeps_the_winner: chords
                               tangent to a 1e-2 cylinder's end circle from
                               1e2 .. 1e4 away (family bound_far) win and are
                               culled
"""
import ctypes as C
import os
from pathlib import Path

import numpy as np
import pytest

import bound_cases as B
import view_cases as V

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
# (SR_BND_LIB: another build of the probe library, as SR_LIB names another libsr.so)
LIBBND = Path(os.environ.get("SR_BND_LIB", ROOT / "schwarzschild-raytracer_amd" / "lib" / "libsr_bnd.so"))
MAX_LAUNCH = 2 ** 18
SLOT_NONE, SLOT_BH, SLOT_TR_FLAT, SLOT_TR_CURVED = -100, -1, -2, -3
KEY_TR_CURVED0 = 2
TR_GROUP_SEGMENTS = 64  # SR_TR_BLOCK x SR_TR_GROUP (csrc/device_scene.h)
OBJECT_CYLINDER = 4


class Probe:
    """lib/libsr_bnd.so's entry points on numpy arrays."""

    def __init__(self, pkg):
        assert LIBBND.exists(), "lib/libsr_bnd.so not built (make -C schwarzschild-raytracer_amd)"
        self.pkg = pkg
        self.lib = lib = pkg.abi.load(LIBBND)
        p, i, u = C.c_void_p, C.c_int, C.c_uint32
        for name, args in {"hit_all": [p, p, p, i, p], "hit_chord": [p, p, u, p, i, p], "may_hit": [p, p, i, p, i, p],
                           "reach": [p, p, i, p, i, p], "clear": [p, p, i, p, i, p], "clear_tr": [p, p, p, i, p, p],
                           "flat": [p, p, p, i, p], "end": [p, p, p, i, p]}.items():
            fn = getattr(lib, "sr_debug_probe_" + name)
            fn.restype, fn.argtypes = C.c_int, args
        lib.sr_debug_probe_path_slack.restype = C.c_float
        self.path_slack = float(lib.sr_debug_probe_path_slack())  # SR_PATH_SLACK
        self.sizes = (C.c_size_t * 3)()
        assert lib.sr_debug_precompute_sizes(self.sizes, 3) == 0
        self._images = {}

    def image(self, case):
        """(image bytes, segment bytes, B.image_views) of a scene case."""
        if case.name not in self._images:
            # the probe library's own packer: the objects libsr.so links
            img, segs = np.zeros(self.sizes[0], dtype=np.uint8), np.zeros(self.sizes[1], dtype=np.uint8)
            rc = self.lib.sr_debug_pack_scene(C.byref(case.scene),
                                              C.byref(case.test_ray) if case.test_ray is not None else None,
                                              img.ctypes.data, segs.ctypes.data)
            assert rc == 0, (case.name, rc)
            self._images[case.name] = (img, segs, B.image_views(self.pkg, img))
        return self._images[case.name]

    def _run(self, name, case, rows, width, out, *lead, extra=None):
        img, segs, _ = self.image(case)
        a = np.ascontiguousarray(rows, dtype=np.float32)
        assert a.ndim == 2 and a.shape[1] == width and a.shape[0] <= MAX_LAUNCH, (name, a.shape)
        args = [img.ctypes.data, segs.ctypes.data, *lead, a.ctypes.data, a.shape[0], out.ctypes.data]
        if extra is not None:
            args.append(extra.ctypes.data)
        rc = getattr(self.lib, "sr_debug_probe_" + name)(*args)
        assert rc == 0, (name, case.name, rc)
        return out

    def hit_all(self, case, chords):
        """int32 [n, 8] rows {slot, face, key, dist, p[3], 0} (float words as bits)."""
        return self._run("hit_all", case, chords, 7, np.zeros((len(chords), 8), dtype=np.int32))

    def hit_chord(self, case, reach, chords):
        return self._run("hit_chord", case, chords, 7, np.zeros((len(chords), 8), dtype=np.int32), C.c_uint32(reach))

    def may_hit(self, case, k, chords):
        return self._run("may_hit", case, chords, 7, np.zeros(len(chords), dtype=np.int32), int(k))

    def reach(self, case, j, abp):
        return self._run("reach", case, abp, 7, np.zeros(len(abp), dtype=np.int32), int(j))

    def clear(self, case, j, anchors):
        return self._run("clear", case, anchors, 3, np.zeros(len(anchors), dtype=np.float32), int(j))

    def clear_tr(self, case, rows):
        gm = np.zeros(len(rows), dtype=np.uint32)
        e = self._run("clear_tr", case, rows, 5, np.zeros(len(rows), dtype=np.float32), extra=gm)
        return e, gm

    def flat(self, case, rays):
        return self._run("flat", case, rays, 6, np.zeros(len(rays), dtype=np.int32))

    def end(self, case, rows):
        return self._run("end", case, rows, 13, np.zeros((len(rows), 2), dtype=np.int32))


class World:
    def __init__(self, pkg, oracle):
        self.pkg, self.oracle = pkg, oracle
        self.probe = Probe(pkg)
        self.cases = B.scene_cases(pkg)
        self.by_name = {c.name: c for c in self.cases}
        self.sets = {c.name: B.chord_set(pkg, c) for c in self.cases}
        self._all = {}

    def chords(self, case):
        """(chords [n, 7], family index [n]) of a case."""
        fams = self.sets[case.name]
        return (np.concatenate([f.chords for f in fams]),
                np.concatenate([np.full(f.chords.shape[0], i) for i, f in enumerate(fams)]))

    def hit_all(self, case):
        """closest_hit_all on every chord of the case (computed once)."""
        if case.name not in self._all:
            self._all[case.name] = self.probe.hit_all(case, self.chords(case)[0])
        return self._all[case.name]


@pytest.fixture(scope="module")
def w(pkg, oracle):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return World(pkg, oracle)


def same_bits(a, b):
    """Equal bits, or NaN on both sides (float32 arrays)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def points_of(H):
    return np.ascontiguousarray(H[:, 4:7]).view(np.float32)


def ends_of(chords):
    """Binary64 end points of float32 chords: (o, o + seg d)."""
    c = chords.astype(np.float64)
    return c[:, :3], c[:, :3] + c[:, 3:6] * c[:, 6:7]


# ---- 1 -----------------------------------------------------------------------------
def test_primitive_parity_at_the_edges(w):
    """closest_hit_all equals oracle.intersect on every chord of every family:
    the winner, the box face or test-ray segment, and the bits of the point
    and its distance (NaN matches NaN)."""
    total = hits = 0
    for case in w.cases:
        chords, fam = w.chords(case)
        H = w.hit_all(case)
        winner, part, point, dist = w.oracle.intersect(case.scene, chords, case.test_ray)
        slot = H[:, 0]
        bad = slot != winner
        got_part = np.where(slot == SLOT_TR_CURVED, H[:, 2] - KEY_TR_CURVED0, H[:, 1])
        hit = winner != SLOT_NONE
        bad |= hit & (got_part != part)
        bad |= hit & ~same_bits(points_of(H), point).all(axis=1)
        bad |= hit & ~same_bits(np.ascontiguousarray(H[:, 3]).view(np.float32), dist)
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            names = [f.name for f in w.sets[case.name]]
            pytest.fail(f"{case.name}: {int(bad.sum())} of {len(bad)} chords differ from the oracle; first: family "
                        f"{names[fam[i]]}, chord {chords[i].tolist()}, device {H[i].tolist()} "
                        f"point {points_of(H)[i].tolist()}, oracle winner {winner[i]} part {part[i]} "
                        f"point {point[i].tolist()}")
        total += len(bad)
        hits += int(hit.sum())
    print(f"parity: {total} chords, {hits} hits")
    assert hits > total // 10


# ---- 2 -----------------------------------------------------------------------------
def test_chord_culling_keeps_the_winner(w):
    """closest_hit_chord with every slot reached returns the bits of
    closest_hit_all on every chord of every scene (test rays visible, the
    SR_KIND_EXACT objects included); may_hit is 0 on every control chord (R <=
    br + 2e-3 S + 4.1e-3 (Sc + r) lies below the controls' distance: the bound
    culls at all) and 1 on every chord the exhaustive intersect resolves to
    that object. Prints the largest binary64 distance of an accepted point
    beyond br, over mu S (cylinders apart: their reach adds lat_margin)."""
    worst, culled, kept = {False: 0.0, True: 0.0}, 0, 0
    for case in w.cases:
        chords, fam = w.chords(case)
        H = w.hit_all(case)
        Hc = w.probe.hit_chord(case, 0xFFFFFFFF, chords)
        floats = same_bits(H[:, 3:7].view(np.float32), Hc[:, 3:7].view(np.float32)).all(axis=1)
        same = (H[:, :3] == Hc[:, :3]).all(axis=1) & floats
        assert same.all(), (case.name, int((~same).sum()), chords[~same][0].tolist(), H[~same][0].tolist(),
                            Hc[~same][0].tolist())
        view = w.probe.image(case)[2]
        fams = w.sets[case.name]
        for i, f in enumerate(fams):
            if f.name == "control":
                assert view["objs"][f.target]["kind"] != B.KIND_EXACT
                m = w.probe.may_hit(case, f.target, f.chords)
                assert not m.any(), (case.name, f.target, int(m.sum()), f.chords[m != 0][0].tolist())
                culled += len(m)
        for k, ob in enumerate(view["objs"]):
            sel = H[:, 0] == k
            if ob["kind"] == B.KIND_EXACT or not sel.any():
                continue
            m = w.probe.may_hit(case, k, chords[sel])
            assert m.all(), (case.name, k, int((m == 0).sum()), chords[sel][m == 0][0].tolist())
            kept += int(sel.sum())
            if np.isfinite(ob["br"]):
                c = chords[sel].astype(np.float64)
                S = B.l1(c[:, :3]) + c[:, 6] + 1.0
                beyond = np.linalg.norm(points_of(H)[sel].astype(np.float64) - ob["bc"], axis=1) - ob["br"]
                ok = np.isfinite(beyond)
                if ok.any():
                    cyl = ob["type"] == OBJECT_CYLINDER
                    worst[cyl] = max(worst[cyl], float(np.max(beyond[ok] / (ob["mu"] * S[ok]))))
    print(f"may_hit: {culled} control chords culled, {kept} winning chords kept; worst (|p - bc| - br) / (mu S) = "
          f"{worst[False]:.4g} (cylinders {worst[True]:.4g})")
    assert culled > 10000 and kept > 10000


def test_margin_safety_factors(w):
    """How much of SR_MU_PLANAR and SR_MU_QUADRATIC the winning chords use.
    may_hit keeps a chord within br + mu S = R + mu (1 + |bc|_1 + R + S) of bc
    (R: the bare bounding radius, binary64 from the primitive's sizes), so a
    chord the exhaustive intersect resolves to the object needs the factor
    (dist64(chord, bc) - R) / (1 + |bc|_1 + R + S). The packed mu over the
    largest factor needed is the safety left: 4000 found for the planar
    primitives and 12.6 for spheres, asserted at a quarter of that (1000 and
    3). Cylinders (their lateral margin lives in the device code) and skewed
    frames (bounded by corners) are printed only."""
    need = {}
    for case in w.cases:
        chords, _ = w.chords(case)
        H = w.hit_all(case)
        view = w.probe.image(case)[2]
        for p in B.prims_of(case.scene):
            ob = view["objs"][p.index]
            sel = H[:, 0] == p.index
            if (not sel.any() or ob["kind"] == B.KIND_EXACT or not np.isfinite(ob["br"]) or not p.finite or
                    (p.kind in ("rectangle", "box", "cylinder") and not p.orthonormal)):
                continue
            o, e = ends_of(chords[sel])
            S = B.l1(o) + chords[sel][:, 6].astype(np.float64) + 1.0
            R = p.bound_radius()
            f = (B.dist_point_segment(ob["bc"], o, e) - R) / (1.0 + B.l1(ob["bc"]) + R + S)
            key = "cylinder" if p.kind == "cylinder" else "sphere" if p.kind == "sphere" else "planar"
            worst = max(float(np.max(f)), 1e-30)
            if key not in need or ob["mu"] / worst < need[key][0]:
                need[key] = (ob["mu"] / worst, worst, ob["mu"], case.name)
    for key, (safety, worst, mu, name) in sorted(need.items()):
        print(f"margin safety, {key}: mu {mu:.3g} over the factor needed {worst:.3g} = {safety:.4g} ({name})")
    assert need["planar"][0] >= 1000.0, need["planar"]
    assert need["sphere"][0] >= 3.0, need["sphere"]


# ---- 3 -----------------------------------------------------------------------------
def _perturbed(rng, A, B_, toward, perr, mode):
    """End points moved by |e| <= perr (binary64), then rounded to binary32."""
    n = A.shape[0]
    if mode == "random":
        e1 = B.random_units(rng, n) * rng.uniform(0.0, 1.0, n)[:, None]
        e2 = B.random_units(rng, n) * rng.uniform(0.0, 1.0, n)[:, None]
    else:
        s = 1.0 if mode == "toward" else -1.0
        with np.errstate(invalid="ignore", divide="ignore"):
            e1 = np.nan_to_num(B.unit(toward - A)) * s
            e2 = np.nan_to_num(B.unit(toward - B_)) * s
    return np.concatenate([A + e1 * perr, B_ + e2 * perr, np.full((n, 1), perr)], axis=1).astype(np.float32)


def _reach_rows(w, case, cylinders):
    """Yields (label, slot j, rows {A, B, perr}, expected) for the case's slots:
    every perr and direction of a slot in one launch."""
    chords, fam = w.chords(case)
    H = w.hit_all(case)
    view = w.probe.image(case)[2]
    fams = w.sets[case.name]
    rng = np.random.default_rng(B.seed_of(case.name) + 3)
    slots = [(0, SLOT_BH, None)] + [(j + 1, int(k), view["slots"][j]) for j, k in enumerate(view["budget_idx"])]
    for j, k, sl in slots:
        if (sl is not None and sl["type"] == OBJECT_CYLINDER) != cylinders:
            continue
        sel = H[:, 0] == k
        A, B_ = ends_of(chords[sel])
        P = points_of(H)[sel].astype(np.float64)
        modes = [(perr, mode) for perr in B.PERRS for mode in ("random", "toward", "away")]
        if sel.any():
            yield (f"{case.name} slot {j} hit", j,
                   np.concatenate([_perturbed(rng, A, B_, P, perr, mode) for perr, mode in modes]), 1)
        for i, f in enumerate(fams):
            if f.name == "control" and f.target == k:
                A, B_ = ends_of(f.chords)
                centre = np.broadcast_to(view["objs"][k]["bc"], A.shape)
                yield (f"{case.name} slot {j} control", j,
                       np.concatenate([_perturbed(rng, A, B_, centre, perr, mode) for perr, mode in modes]), 0)


def _check_reach(w, cylinders, wants=(0, 1)):
    """-> (rows that must reach, control rows); asserts after every slot ran."""
    count = {0: 0, 1: 0}
    report = []
    for case in w.cases:
        for label, j, rows, want in _reach_rows(w, case, cylinders):
            ok = np.isfinite(rows).all(axis=1)
            if want not in wants or not ok.any():
                continue
            got = w.probe.reach(case, j, rows[ok])
            bad = got != want
            if bad.any():
                report.append(f"{label}: {int(bad.sum())} of {len(bad)} rows give {1 - want}; first "
                              f"{rows[ok][bad][0].tolist()}")
            count[want] += len(got)
    print("\n".join(report))
    assert not report, "\n".join(report)
    return count[1], count[0]


def test_slot_reachable_is_sound(w):
    """Every chord the exhaustive intersect resolves to slot j's object (slot 0:
    the hole), its end points moved by |e| <= perr (perr = 0, 1e-6, 1e-4, 1e-2;
    at random, toward the hit point, away from it) and rounded to binary32,
    gives slot_reachable == 1; the control chords moved the same way give 0.
    Slots that are not cylinders (test_slot_reachable_is_sound_for_cylinders
    and test_slot_reachable_culls_cylinder_controls hold those)."""
    n_hit, n_ctl = _check_reach(w, cylinders=False)
    print(f"slot_reachable: {n_hit} reaching chords, {n_ctl} controls")
    assert n_hit > 50000 and n_ctl > 50000


def test_slot_reachable_is_sound_for_cylinders(w):
    """The same chords and perturbations on cylinder slots: slot_reachable == 1
    for every chord resolved to the cylinder."""
    n_hit, _ = _check_reach(w, cylinders=True, wants=(1,))
    print(f"slot_reachable, cylinders: {n_hit} reaching chords")
    assert n_hit > 5000


def test_slot_reachable_culls_cylinder_controls(w):
    """The control chords of cylinder slots give slot_reachable == 0.

    With SR_REACH_LAT 0 (the margin SR_CYL_QMARGIN Sc^2 / (r |d_perp|^2 / 2),
    and 1 outright within 1e-6 of the axis direction) the radius-1e-3 cylinder
    of `alone/cylinder_thin` was reached on 407 of its 4608 control rows: 4e-3
    Sc^2 / |d_perp|^2 there, more than the controls' 0.1 Sc. slot_reachable
    takes may_hit's lat_margin since (SR_REACH_LAT 1, at most 4.1e-3 (Sc + r)
    for every direction), and test_slot_reachable_is_sound_for_cylinders holds
    that to the winning chords."""
    _, n_ctl = _check_reach(w, cylinders=True, wants=(0,))
    print(f"slot_reachable, cylinders: {n_ctl} controls")
    assert n_ctl > 5000


# ---- 4 -----------------------------------------------------------------------------
def _toward(prim, A):
    """Unit vectors from the points A toward the primitive (-grad dist, binary64)."""
    d0 = prim.dist(A)
    h = np.maximum(1e-9, 1e-5 * np.maximum(d0, 1e-3))
    g = np.stack([(prim.dist(A + h[:, None] * e) - prim.dist(A - h[:, None] * e)) / (2.0 * h) for e in np.eye(3)],
                 axis=1)
    nrm = np.linalg.norm(g, axis=1, keepdims=True)
    return np.where(nrm > 1e-6, -g / np.where(nrm > 0, nrm, 1.0), 0.0)


def ball_chords(rng, A, rho, toward, per=4):
    """Chords whose two ends lie in the balls of radius rho around the anchors
    A (binary64 [n, 3], exactly float32 values): toward `toward` at full
    length, `per` pairs near the ball's pole facing it, `per` random pairs.
    Rounded to binary32, then those whose ends left the ball are dropped.
    -> (chords [m, 7], anchor index [m])."""
    n = A.shape[0]
    spacing = np.spacing(np.max(np.abs(A), axis=1).astype(np.float32)).astype(np.float64)
    r = np.maximum(0.0, rho * (1.0 - 1e-6) - 2.0 * spacing)
    rows, idx = [], []

    def add(P1, P2, i):
        o = P1.astype(np.float32).astype(np.float64)
        dv = P2 - o
        seg = np.linalg.norm(dv, axis=1)
        ok = seg > 0
        d = np.where(ok[:, None], dv / np.where(ok, seg, 1.0)[:, None], [1.0, 0.0, 0.0])
        rows.append(B.pack(o, d, seg))
        idx.append(i)

    every = np.arange(n)
    add(A, A + toward * r[:, None], every)
    for _ in range(per):
        pole = [B.unit(toward + 0.3 * rng.normal(size=(n, 3)) + 1e-12) for _ in range(2)]
        add(A + pole[0] * r[:, None], A + pole[1] * r[:, None], every)
        inside = [B.random_units(rng, n) * (r * rng.uniform(0.0, 1.0, n) ** (1.0 / 3.0))[:, None] for _ in range(2)]
        add(A + inside[0], A + inside[1], every)
    ch, ix = np.concatenate(rows), np.concatenate(idx)
    o, e = ends_of(ch)
    keep = (np.isfinite(ch).all(axis=1) & (np.linalg.norm(o - A[ix], axis=1) <= rho[ix]) &
            (np.linalg.norm(e - A[ix], axis=1) <= rho[ix]))
    return ch[keep], ix[keep]


def test_clearances_are_sound_and_below_the_distance(w):
    """From an anchor A with c = clearance_obj(A) > 0 (clearance_bh for the
    hole), no chord whose ends lie in the ball of radius c / SR_PATH_SLACK
    around A is resolved to that object by the exhaustive intersect of the
    one-object scene: the chord toward the binary64-nearest point at full
    length, pairs at the ball's pole facing the primitive, random pairs.
    Orthonormal slots: c <= the binary64 distance from A to the primitive.
    Anchors keeping the CPU test's guard (non-cylinder slots): c >= the guard
    value - 1e-4. Each anchor set runs shuffled (near and far anchors share
    waves) and sorted by distance (whole waves are far: clearance_obj skips the
    primitive's own distance there). Prints the smallest distance / c."""
    worst = np.inf
    n_pos = n_chords = n_guard = 0
    for case in w.cases:
        if not case.alone:
            continue
        view = w.probe.image(case)[2]
        hole = case.name == "hole"
        if hole:
            prim, j, target = B.HOLE, 0, SLOT_BH
        else:
            (prim,) = B.prims_of(case.scene)
            if view["num_budget"] != 1:
                continue
            j, target = 1, 0
        ob = None if hole else view["objs"][0]
        rng = np.random.default_rng(B.seed_of(case.name) + 1)
        A32 = B.anchors(prim, rng, B.N)
        rng.shuffle(A32)
        order = np.argsort(np.linalg.norm(A32.astype(np.float64) - (np.zeros(3) if hole else ob["bc"]), axis=1))
        for label, A in (("shuffled", A32), ("sorted", A32[order])):
            c = w.probe.clear(case, j, A).astype(np.float64)
            A64 = A.astype(np.float64)
            exact = (hole or prim.kind == "sphere" or
                     (prim.unit_normal if prim.kind in ("plane", "disk", "annulus") else prim.orthonormal))
            if exact:
                dist = prim.dist(A64)
                over = c > dist
                assert not over.any(), (case.name, label, A[over][0].tolist(), float(c[over][0]), float(dist[over][0]))
                pos = c > 0
                if pos.any():
                    worst = min(worst, float(np.min(dist[pos] / c[pos])))
            if not hole and ob["type"] != OBJECT_CYLINDER and np.isfinite(ob["br"]):
                g = B.guard_value(A, ob["bc"], ob["br"])
                sel = g >= 0.05
                low = sel & ~(c >= g - 1e-4)
                assert not low.any(), (case.name, label, A[low][0].tolist(), float(c[low][0]), float(g[low][0]))
                n_guard += int(sel.sum())
            pos = np.isfinite(c) & (c > 0)
            if not pos.any():
                continue
            n_pos += int(pos.sum())
            Ap, rho = A64[pos], c[pos] / w.probe.path_slack
            toward = _toward(prim, Ap) if exact else B.unit(prim.pos - Ap + 1e-30)
            ch, ix = ball_chords(rng, Ap, rho, toward)
            for s in range(0, len(ch), MAX_LAUNCH):
                H = w.probe.hit_all(case, ch[s:s + MAX_LAUNCH])
                bad = H[:, 0] == target
                assert not bad.any(), (case.name, label, int(bad.sum()), ch[s:s + MAX_LAUNCH][bad][0].tolist(),
                                       Ap[ix[s:s + MAX_LAUNCH][bad][0]].tolist(), float(rho[ix[s:s + MAX_LAUNCH][bad][0]]))
            n_chords += len(ch)
    print(f"clearances: {n_pos} positive anchors, {n_chords} ball chords, {n_guard} guard anchors; "
          f"smallest binary64 distance / c = {worst:.6g}")
    assert n_pos > 10000 and n_chords > 50000 and n_guard > 5000
    assert worst >= 1.0


# ---- 5 -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["test-ray/press-r", "test-ray/overlay-1000"])
def test_clearance_tr(w, name):
    """clearance_tr(A, rlen) -> (e, gm): for chords whose ends lie within rlen
    of A the exhaustive intersect's winner is never a curved segment of a group
    whose gm bit is clear, never the flat cylinder when bit 31 is clear, and
    never any test-ray part when gm == 0 and e is infinite; and for chords in
    the ball of radius e / SR_PATH_SLACK (e > 0) it is never a test-ray part.
    Anchors from inside the polyline's tube out to 1e2."""
    case = w.by_name[name]
    tr = case.test_ray
    pts = B.test_ray_points(tr)
    rng = np.random.default_rng(B.seed_of(name) + 5)
    n = 4096
    i = rng.integers(0, len(pts) - 1, n)
    on_axis = pts[i] + (pts[i + 1] - pts[i]) * rng.uniform(0.0, 1.0, n)[:, None]
    off = B.log_uniform(rng, 1e-3 * float(tr.radius), 1e2, n)
    A = (on_axis + B.random_units(rng, n) * off[:, None]).astype(np.float32)
    # also along the flat cylinder
    fo = np.array([tr.flat_origin[k] for k in range(3)], dtype=np.float64)
    fd = B.unit(np.array([tr.flat_dir[k] for k in range(3)], dtype=np.float64))
    m = n // 4
    A[:m] = (fo + fd * rng.uniform(-1.0, float(tr.extended_length) + 1.0, m)[:, None] +
             B.random_units(rng, m) * off[:m, None]).astype(np.float32)
    rlen = (off * B.log_uniform(rng, 0.3, 3.0, n)).astype(np.float32)
    rows = np.concatenate([A, np.ones((n, 1), np.float32), rlen[:, None]], axis=1)
    e, gm = w.probe.clear_tr(case, rows)
    A64 = A.astype(np.float64)

    def winners(radius):
        toward = B.unit(on_axis - A64 + 1e-30)
        toward[:m] = B.unit(fo + fd * np.clip(np.sum((A64[:m] - fo) * fd, axis=1), 0.0, float(tr.extended_length))[:, None]
                            - A64[:m] + 1e-30)
        ch, ix = ball_chords(rng, A64, radius, toward, per=3)
        H = np.concatenate([w.probe.hit_all(case, ch[s:s + MAX_LAUNCH]) for s in range(0, len(ch), MAX_LAUNCH)])
        return ch, ix, H

    ch, ix, H = winners(rlen.astype(np.float64))
    slot, seg = H[:, 0], H[:, 2] - KEY_TR_CURVED0
    curved, flat = slot == SLOT_TR_CURVED, slot == SLOT_TR_FLAT
    group_bit = (gm[ix] >> np.where(curved, seg // TR_GROUP_SEGMENTS, 0).astype(np.uint32)) & 1
    bad = curved & (group_bit == 0)
    assert not bad.any(), (int(bad.sum()), ch[bad][0].tolist(), A[ix[bad][0]].tolist(), float(rlen[ix[bad][0]]),
                           int(seg[bad][0]), hex(int(gm[ix[bad][0]])))
    bad = flat & ((gm[ix] >> 31) == 0)
    assert not bad.any(), (int(bad.sum()), ch[bad][0].tolist(), A[ix[bad][0]].tolist(), float(rlen[ix[bad][0]]))
    bad = (curved | flat) & (gm[ix] == 0) & np.isposinf(e[ix])
    assert not bad.any(), int(bad.sum())
    parts = np.uint32(((1 << w.probe.image(case)[2]["tr_num_groups"]) - 1) | (1 << 31))
    n_tr, n_clear_bits = int((curved | flat).sum()), int(((gm & parts) != parts).sum())
    pos = np.isfinite(e) & (e > 0)
    ch2, ix2, H2 = winners(np.where(pos, e.astype(np.float64) / w.probe.path_slack, 0.0))
    live = pos[ix2]
    bad = live & ((H2[:, 0] == SLOT_TR_CURVED) | (H2[:, 0] == SLOT_TR_FLAT))
    assert not bad.any(), (int(bad.sum()), ch2[bad][0].tolist(), A[ix2[bad][0]].tolist(), float(e[ix2[bad][0]]))
    print(f"{name}: {n_tr} of {len(ch)} chords within rlen won by a test-ray part, {n_clear_bits} of {n} anchors "
          f"with a cleared bit, {int(pos.sum())} positive clearances, {int(live.sum())} chords in their balls")
    assert n_tr > 500 and n_clear_bits > n // 4 and pos.sum() > n // 4


# ---- 6 -----------------------------------------------------------------------------
def test_flat_misses_finds_nothing(w):
    """Wherever flat_misses(ro, rd) holds, the unbounded exhaustive intersect
    from ro finds nothing: |ro|^2 a few floats either side of flat_miss_r2,
    ro . rd a tiny value of either sign, rays aimed past the farthest reach."""
    n_true = n_rays = n_scenes = 0
    for case in w.cases:
        view = w.probe.image(case)[2]
        r2 = view["flat_miss_r2"]
        if not np.isfinite(r2) or view["tr_visible"]:
            continue
        rng = np.random.default_rng(B.seed_of(case.name) + 6)
        n = 2048
        r = np.sqrt(np.float64(r2)) * (1.0 + rng.integers(-8, 9, n) * 2.0 ** -24)
        r[n // 2:] *= B.log_uniform(rng, 1.0, 1e2, n - n // 2)
        u = B.random_units(rng, n)
        ro = u * r[:, None]
        tiny = rng.choice([-1.0, 1.0], n) * B.log_uniform(rng, 1e-9, 1e-2, n)
        tiny[::7] = 0.0
        rd = B.unit(B.perpendicular(rng, u) + u * tiny[:, None])
        # a quarter aimed to graze the sphere of the farthest reach (half of sqrt(r2 - 1) at most)
        q = n // 4
        reach = 0.5 * np.sqrt(max(r2 - 1.0, 0.0))
        sin_a = np.clip(reach / r[:q], 0.0, 1.0) * (1.0 + rng.choice([-1.0, 1.0], q) * B.log_uniform(rng, 1e-7, 1e-1, q))
        sin_a = np.clip(sin_a, 0.0, 1.0)
        rd[:q] = B.unit(-u[:q] * np.sqrt(1.0 - sin_a ** 2)[:, None] + B.perpendicular(rng, u[:q]) * sin_a[:, None])
        rd[:q:2] *= -1.0  # half of them looking back along the same line: leaving
        rays = np.concatenate([ro, rd], axis=1).astype(np.float32)
        fm = w.probe.flat(case, rays)
        H = w.probe.hit_all(case, np.concatenate([rays, np.full((n, 1), -1.0, np.float32)], axis=1))
        bad = (fm == 1) & (H[:, 0] != SLOT_NONE)
        assert not bad.any(), (case.name, int(bad.sum()), rays[bad][0].tolist(), H[bad][0].tolist())
        assert (fm == 1).any() and (fm == 0).any(), case.name
        n_true += int((fm == 1).sum())
        n_rays += n
        n_scenes += 1
    print(f"flat_misses: true on {n_true} of {n_rays} rays in {n_scenes} scenes")
    assert n_scenes >= 20


def _nudge(x, k):
    """x moved by k floats (binary32)."""
    x = np.asarray(x, dtype=np.float32).copy()
    for _ in range(abs(int(k))):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf))
    return x


def test_certain_end_ends_the_ray(w):
    """Wherever certain_end(u, up, r2) holds, sphere_lambda_r2 on the chord
    point_at builds from (up, u) returns false (the reseed ends the ray):
    (u, up) a few floats either side of each of its five conditions, r2 from
    the u_f values of tests/view_cases.py, random orthonormal frames, the step
    angles of 100 .. 65536 steps."""
    F = np.float32
    ufs = sorted({float(V.params_of(w.pkg, c).u_f) for c in V.CASES})
    r2s = [F(F(1.0) / F(u)) * F(F(1.0) / F(u)) for u in ufs if np.isfinite(u) and u > 1e-6]  # uf_radius2
    assert len(r2s) >= 8
    rng = np.random.default_rng(66)
    delta, end_r2 = F(1.0 - 2.0 ** -10), F(1.0 - 2.0 ** -9)  # SR_END_DELTA, SR_END_R2
    rows = []
    for r2 in r2s:
        n = 256
        u_edge = F(np.sqrt(np.float64(end_r2) / np.float64(r2)))  # u^2 r2 = SR_END_R2
        for k in range(-6, 7):
            # around u^2 r2 < SR_END_R2, up well above
            u = _nudge(np.full(n, u_edge, F), k)
            up = (u.astype(np.float64) * B.log_uniform(rng, 1.0 + 2e-3, 10.0, n)).astype(F)
            rows.append((u, up, r2))
            # around u <= up SR_END_DELTA, u at and below the r2 edge
            u = (np.float64(u_edge) * rng.uniform(0.05, 1.0, n)).astype(F)
            up = _nudge((u.astype(np.float64) / np.float64(delta)).astype(F), k)
            rows.append((u, up, r2))
        # around u >= 2^-40, u < 1 and up < 1e30
        for k in range(-3, 4):
            u = _nudge(np.full(n, 2.0 ** -40, F), k)
            rows.append((u, (u.astype(np.float64) * 2.0).astype(F), r2))
            u = _nudge(np.full(n, 1.0, F), k)
            rows.append((u, (u.astype(np.float64) * 2.0).astype(F), r2))
            u = (np.float64(u_edge) * rng.uniform(0.05, 0.9, n)).astype(F)
            rows.append((u, _nudge(np.full(n, 1.0e30, F), k), r2))
    u = np.concatenate([r[0] for r in rows])
    up = np.concatenate([r[1] for r in rows])
    r2 = np.concatenate([np.full(len(r[0]), r[2], F) for r in rows])
    n = len(u)
    nv = B.random_units(rng, n)
    tv = B.perpendicular(rng, nv)
    steps = rng.choice([100, 400, 1000, 4096, 65536], n)
    dphi = 2.0 * np.pi * rng.choice([1, 2, 3], n) / steps
    k = rng.integers(0, steps - 1)
    cs = [np.cos(k * dphi), np.sin(k * dphi), np.cos((k + 1) * dphi), np.sin((k + 1) * dphi)]
    data = np.concatenate([u[:, None], up[:, None], r2[:, None], nv, tv, *[c[:, None] for c in cs]],
                          axis=1).astype(np.float32)
    out = np.concatenate([w.probe.end(w.cases[0], data[s:s + MAX_LAUNCH]) for s in range(0, n, MAX_LAUNCH)])
    certain, sphere = out[:, 0] == 1, out[:, 1] == 1
    bad = certain & sphere
    assert not bad.any(), (int(bad.sum()), data[bad][0].tolist())
    print(f"certain_end: true on {int(certain.sum())} of {n} inputs; the sphere test hit on {int(sphere.sum())}")
    assert certain.sum() > n // 10 and (~certain).sum() > n // 10
