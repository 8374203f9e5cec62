"""The picking scenes of tests/pick_cases.py on the oracle alone: every pixel's
colour decodes to exactly one code, and each code a case claims to cover
appears on at least 1 % of its frame (a condition of tests/test_gpu_pick.py:
a map that never held the code could not be told from one that did)."""
import numpy as np
import pytest

import pick_cases as P

@pytest.fixture(scope="module")
def picks(pkg, oracle, textures):
    return P.Picks(pkg, oracle, textures)


CASE_IDS = ["stress", "default", "flat", "half-width", "overlay", "noise", "translucent-front", "single-sided-behind",
            "single-sided-behind-flat", "kinds"]


def test_table_is_complete(picks):
    assert sorted(picks.cases) == sorted(CASE_IDS)


@pytest.mark.parametrize("name", CASE_IDS)
def test_case_decodes_and_covers(picks, name):
    case = picks.cases[name]
    best = {}
    for cam in case["cams"]:
        codes, ok = picks.codes(case, cam)
        assert ok.all(), f"{name} {cam}: {int((~ok).sum())} of {ok.size} pixels do not decode to exactly one code"
        assert ((codes >= P.NONE) & (codes < int(case["scene"].num_objects))).all()
        vals, counts = np.unique(codes, return_counts=True)
        share = {int(v): c / codes.size for v, c in zip(vals, counts)}
        print(f"MEASURED {name} {cam}: " + ", ".join(f"{v}: {s:.1%}" for v, s in sorted(share.items())))
        for code, v in share.items():
            best[code] = max(best.get(code, 0.0), v)
    for code in case["covers"]:  # on at least 1 % of the frame of one of the case's cameras
        assert best.get(code, 0.0) >= P.MIN_SHARE, (name, code, best.get(code, 0.0))


def test_cases_say_what_they_claim(picks):
    """The flat case is flat everywhere, the single-sided surface is seen from
    behind (it shows in no pixel, the object behind it or the sky does), and
    the translucent one is reported in front of the opaque one."""
    c = picks.cases
    behind, _ = picks.codes(c["single-sided-behind"], "rect")
    flat, _ = picks.codes(c["single-sided-behind-flat"], "rect")
    assert not (behind == 0).any() and not (flat == 0).any()
    # where the curved walk goes on to the object behind, the flat intersect does not look: more sky
    assert (flat == P.SKY).sum() > (behind == P.SKY).sum() and (flat == 1).sum() < (behind == 1).sum()
    front, _ = picks.codes(c["translucent-front"], "rect")
    cy, cx = front.shape[0] // 2, front.shape[1] // 2
    assert front[cy, cx] == 0 and (front == 1).any()
