#!/usr/bin/env python3
"""Records tests/golden/lens_reference.npz and tests/golden/lens_tolerances.json
(CPU only, about two minutes):

    python tests/golden/make_lens_reference.py

lens_reference.npz: what tests/geodesic_reference.py's exact() gives for every
ray of its ray_set(), u_f = 0.01, max_revolutions 1, 2 and 4: class, exit
tangent, end angle, sensitivity s per max_revolutions; b, phi_exit, u' at the
exit, the orbital plane's normal, the first crossings of r = 4, 20 and 60 and
their sensitivities; the rays themselves. tests/test_gpu_lens_physics.py
compares the kernel with it and needs no scipy loop.

lens_tolerances.json: the tolerances of that comparison, tol = eps + delta s.
Neither number can be derived; both are measured here, on the float32 scheme
model against the reference (level C, the finite radii) or against the
float64 model (level B), by geodesic_reference.fit's rule, never on the kernel
or the oracle, then multiplied by MARGIN: the kernel's trig and contraction
make its rounding another draw from the distribution whose one draw the model
is. Rays that start beyond r = 1 / u_f get a pair of their own: the float32
entry into that sphere costs them a relative 1e-5 of b, ten times what the
walk costs the others. The file also records the float64 model's distance from
the reference (the scheme's truncation) by step count, the float32 model's
error by |b / b_crit - 1| (DESIGN.md's CPU column) and the model error of the
flat exterior.

Both files are this project's own recorded results and regenerate byte for
byte on the same numpy and scipy.
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tests" / "golden"))

import geodesic_reference as G  # noqa: E402

COMMAND = "python tests/golden/make_lens_reference.py"
MARGIN = 4.0


def pair(err, s):
    eps, delta = G.fit(err, s)
    return {"eps_fit": eps, "delta_fit": delta, "eps": MARGIN * eps, "delta": MARGIN * delta}


def scalar(x):
    return {"fit": float(x), "tol": MARGIN * float(x)}


def by_origin(err, s, beyond):
    return {"inside": pair(err[~beyond], s[~beyond]), "beyond": pair(err[beyond], s[beyond])}


def main() -> None:
    from make_golden import write_npz

    L = G.Lens.compute()
    out = ROOT / "tests" / "golden"
    write_npz(out / "lens_reference.npz", L.ref)

    tol = {"command": COMMAND, "margin": MARGIN, "u_f": G.U_F, "rays": int(len(L.O)),
           "rule": "geodesic_reference.fit; tol = margin * fit; radians, hit_radius in length units"}
    # ---- level C: float32 model against the reference, N = 2000, max_revolutions 2
    k = L.c_sky()
    m32 = L.model(G.LEVEL_C_STEPS, 2, np.float32)
    assert (m32["class"][k] == G.SKY).all(), "the float32 model flips a class of the set"
    err = G.angle_between(m32["dir"][k], L.tangent(2)[k])
    s, beyond, x = L.s(2)[k], L.beyond[k], L.x[k]
    c = {"steps": G.LEVEL_C_STEPS, "max_revolutions": 2, "rays": int(k.sum()), "dir": by_origin(err, s, beyond),
         "plane": scalar(np.abs(np.sum(m32["dir"][k].astype(np.float64) * L.ref["plane"][k], axis=-1)).max()),
         "model_f32_error_by_offset": G.error_table(err, s, x)}
    trunc = {}
    for n in G.TRUNCATION_STEPS:
        m64 = L.model(n, 2, np.float64)
        same = k & (m64["class"] == G.SKY)
        e = G.angle_between(m64["dir"][same], L.tangent(2)[same])
        trunc[str(n)] = {"max": float(e.max()), "median": float(np.median(e)), "class_flips": int((k & ~same).sum())}
    c["truncation_f64_model"] = trunc
    tol["level_c"] = c
    # ---- level B: float32 model against the float64 model, per step count over the three max_revolutions
    tol["level_b"] = {}
    for n in G.LEVEL_B_STEPS:
        errs, ss, bs, planes, flips = [], [], [], [], {}
        for rev in G.REVOLUTIONS:
            m32, m64 = L.model(n, rev, np.float32), L.model(n, rev, np.float64)
            k = L.level_b(rev, m64) & G.ends_in_sky(m32["class"])
            errs.append(G.angle_between(m32["dir"][k], m64["dir"][k]))
            ss.append(L.s(rev)[k])
            bs.append(L.beyond[k])
            kp = k & ~L.straight
            planes.append(np.abs(np.sum(m32["dir"][kp].astype(np.float64) * L.ref["plane"][kp], axis=-1)).max())
            flips[str(rev)] = int(L.model_flips(rev, m64).sum())
        tol["level_b"][str(n)] = {"dir": by_origin(np.concatenate(errs), np.concatenate(ss), np.concatenate(bs)),
                                  "plane": scalar(max(planes)), "f64_model_class_differs_from_exact": flips}
    # ---- the finite radii: float32 model against the reference's first crossing
    tol["finite_radius"] = {}
    for j, R in enumerate(G.RADII):
        k = L.inside_radius(j)
        m32 = L.model(G.LEVEL_C_STEPS, 2, np.float32, R)
        m64 = L.model(G.LEVEL_C_STEPS, 2, np.float64, R)
        assert (m32["class"][k] == G.SURFACE).all() and (m64["class"][k] == G.SURFACE).all()
        s = L.ref["s_cross"][k, j]
        p = m32["hit_point"][k].astype(np.float64)
        tol["finite_radius"][str(int(R))] = {
            "rays": int(k.sum()),
            "angle": pair(G.angle_between(p, L.ref["cross"][k, j]), s),
            "radius": scalar(np.abs(np.linalg.norm(p, axis=-1) - R).max()),
            "view": pair(G.angle_between(m32["hit_view"][k], m64["hit_view"][k]), s)}
    # ---- the model error of the flat exterior: the reference against itself with u_f -> 0
    k = np.flatnonzero(L.c_sky() & ~L.beyond)
    far = np.stack([G.exact(L.O[i], L.V[i], 0.0, (2,), (), sensitivity=False)["tangent"][0] for i in k])
    e = G.angle_between(far, L.tangent(2)[k])
    tol["flat_exterior_model_error"] = {"rays": int(len(k)), "max": float(e.max()), "median": float(np.median(e)),
                                        "by_offset": G.error_table(e, np.ones(len(k)), L.x[k])}
    (out / "lens_tolerances.json").write_text(json.dumps(tol, indent=1, sort_keys=True) + "\n")
    print(json.dumps(tol, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
