"""tests/walk_cases.py on the CPU (the oracle and the host library only): the
walks can catch what tests/test_gpu_context_walk.py runs them for. Every
bound here is a condition on the generated inputs, not a measurement of the
library.
"""
import collections
import ctypes as C
import json

import numpy as np
import pytest

import projection_cases as P
import walk_cases as WC
from reshade_cases import changed_share

MIN_KIND = 3  # every op kind, over all walks
MIN_RULE = 2  # every drop and keep rule, with a valid frame before it
MIN_VALID, MIN_NOT_VALID = 0.30, 0.20  # of the consumer ops
MIN_CHANGED = 0.01  # of the 33x17 frame's pixels, across a setter that changes pixels


@pytest.fixture(scope="module")
def rs(pkg, oracle, textures):
    return WC.Resolver(pkg, oracle, textures)


@pytest.fixture(scope="module")
def walks():
    return WC.walks()


def test_walks_are_data_and_reproducible(walks):
    assert tuple(walks) == WC.WALK_NAMES and len(WC.RANDOM_SEEDS) == 8
    for seed in WC.RANDOM_SEEDS:
        again = WC.random_walk(seed)
        assert json.dumps(again) == json.dumps(walks[f"random-{seed}"]) and len(again) == WC.RANDOM_LENGTH
    covered = set().union(*(WC.setter_output_pairs(walks[f"random-{s}"]) for s in WC.RANDOM_SEEDS))
    assert json.dumps(WC.pair_walk(covered)) == json.dumps(walks["pairs"])
    assert json.dumps(WC.pressure_walk()) == json.dumps(walks["pressure"])


def test_every_kind_occurs(walks):
    n = collections.Counter(op["kind"] for ops in walks.values() for op in ops)
    assert set(n) == set(WC.KINDS)
    rare = {k: n[k] for k in WC.KINDS if n[k] < MIN_KIND}
    assert not rare, rare


DROPPING = ("set_scene_geo", "set_test_ray", "set_texture_array", "set_projection")


def test_every_setter_is_followed_by_every_output_kind(walks):
    """As "setter, then the next op that produces output", with an output op
    the model says succeeds (it writes, and is compared with the fresh
    context). The one exception is a consumer straight after a setter that
    just dropped the frame: SR_E_NOT_READY is all that pair can give."""
    ok, not_ready = set(), set()
    for ops in walks.values():
        m, last = WC.Model(), None
        for op in ops:
            k = op["kind"]
            had = m.retained is not None
            status, _ = m.step(op)
            if k in WC.SETTERS:
                last = (k, had and m.retained is None)
            elif k in WC.OUTPUT_KINDS:
                if last is not None and status == WC.OK:
                    ok.add((last[0], k))
                elif last is not None and status == WC.NOT_READY and k in WC.CONSUMERS and last[1]:
                    assert last[0] in DROPPING
                    not_ready.add((last[0], k))
                last = None
    missing = [(s, k) for s in WC.SETTERS for k in WC.OUTPUT_KINDS if (s, k) not in ok | not_ready]
    assert not missing, missing
    only_not_ready = not_ready - ok
    assert all(s in DROPPING and k in WC.CONSUMERS for s, k in only_not_ready), only_not_ready
    # every pair outside "dropping setter, then consumer" succeeds; the same projection said again keeps the frame
    assert len(ok) >= len(WC.SETTERS) * len(WC.OUTPUT_KINDS) - len(DROPPING) * 4 + 1
    assert ok | not_ready == set().union(*(WC.setter_output_pairs(ops) for ops in walks.values()))


def test_consumers_meet_valid_and_invalid_frames_and_every_rule_fires(walks):
    valid = total = 0
    rules = collections.Counter()
    statuses = collections.Counter()
    for ops in walks.values():
        m = WC.Model()
        for op in ops:
            if op["kind"] in WC.CONSUMERS[:4]:
                total += 1
                valid += m.retained is not None
            status, rule = m.step(op)
            statuses[(op["kind"], status)] += 1
            if rule is not None:
                rules[rule] += 1
    assert valid / total >= MIN_VALID and (total - valid) / total >= MIN_NOT_VALID, (valid, total)
    few = {r: rules[r] for r in WC.DROP_RULES + WC.KEEP_RULES if rules[r] < MIN_RULE}
    assert not few, few
    # the statuses sr.h gives the consumers of a frame that is there but of the wrong kind
    assert statuses[("reshade_debug", WC.INVALID)] >= 2 and statuses[("pick_map", WC.NOT_READY)] >= 2
    for k in WC.REJECTS:
        assert statuses[(k, WC.INVALID)] >= 1, k


def _state_frame(rs, st):
    return rs.frame(st["scene"], st["ray"], st["bg"], st["tex"])[0]


def test_a_stale_state_would_show(walks, rs):
    """Across every setter op that changes pixels, the oracle's 33x17 frames of
    the declared state before and after differ on at least 1 % of the pixels."""
    checked = collections.Counter()
    for name, ops in walks.items():
        m = WC.Model()
        for i, op in enumerate(ops):
            before = m.declared()
            m.step(op)
            after = m.declared()
            k = op["kind"]
            if k not in WC.PIXEL_SETTERS or k == "set_projection":
                continue
            assert before != after, (name, i, op)
            if k == "set_sequence":
                # frame 1 of a sequence launch; a load or a clear shows in the launch's status
                if before["seq"] is None or after["seq"] is None:
                    continue
                a = rs.frame((before["seq"], 1), before["ray"], before["bg"], before["tex"])[0]
                b = rs.frame((after["seq"], 1), after["ray"], after["bg"], after["tex"])[0]
            else:
                if before["scene"] is None or before["bg"] is None or before["tex"] is None:
                    continue  # no frame before: the launches before it were SR_E_NOT_READY
                a, b = _state_frame(rs, before), _state_frame(rs, after)
            share = changed_share(a, b)
            assert share >= MIN_CHANGED, (name, i, op, share)
            checked[k] += 1
    assert all(checked[k] >= 5 for k in WC.PIXEL_SETTERS if k != "set_projection"), checked


def test_projection_ops_use_the_cases_proven_to_differ(walks):
    """tests/test_projection_cases.py shows that the equirect and the fisheye
    frame of camera "view" at 33x17 differ from the pinhole's on a quarter of
    the pixels; the walks set those projections and launch that camera."""
    shown = {c[1] for c in P.CASES if (c[2], c[3], c[4]) == (33, 17, None)}
    assert shown == {P.EQUIRECT, P.FISHEYE}
    values = {op["projection"] for ops in walks.values() for op in ops if op["kind"] == "set_projection"}
    assert values == {P.RECTILINEAR} | shown
    assert "view" in WC.CAMS and (33, 17) in WC.SHAPES


def test_shading_only_classification_is_the_librarys(walks, rs, pkg):
    abi = pkg.abi
    lib = abi.load()
    seen = collections.Counter()
    for ops in walks.values():
        cur = None
        for op in ops:
            if op["kind"] not in ("set_scene_geo", "set_scene_shade"):
                continue
            if cur is not None:
                a, b = rs.scene(cur), rs.scene(op["scene"])
                model = op["kind"] == "set_scene_shade"
                assert model == (WC.base_of(cur) == WC.base_of(op["scene"]))
                assert model == WC.shading_only_fields(abi, a, b)
                assert int(model) == lib.sr_scene_shading_only(C.byref(a), C.byref(b))
                assert bytes(a) != bytes(b)
                seen[model] += 1
            cur = op["scene"]
    assert seen[True] >= 10 and seen[False] >= 10, seen


def test_pressure_walk_exceeds_every_cache_and_returns(walks):
    keys = WC.pressure_keys(walks["pressure"])
    for name, ks in keys.items():
        distinct, revisits = WC.lru_revisits(ks, capacity=8)
        assert distinct >= 9 and revisits >= 1, (name, distinct, revisits)
    # a block-list frame is used, and the next use comes after nine more lists: the first frame's
    # list is evicted by then, and the frame read is the last launch's (every block-list launch
    # replaces the retained frame, so no call sequence evicts a list under a frame that stays)
    ops = walks["pressure"]
    first = next(i for i, op in enumerate(ops) if op["kind"] == "render_block_list")
    uses = [i for i, op in enumerate(ops) if op["kind"] == "reshade" and i > first]
    lists_between = {tuple(op["blocks"]) for op in ops[uses[0]:uses[1]] if "blocks" in op}
    assert len(lists_between) >= 8


def test_model_statuses_of_a_fresh_context():
    m = WC.Model()
    rng = np.random.default_rng(0)
    for kind in WC.LAUNCHES + WC.CONSUMERS[:4] + WC.TRACES + ("reject_pitch", "reject_window"):
        assert m.step(WC.make_op(rng, kind, m))[0] == WC.NOT_READY, kind
    assert m.step(WC.make_op(rng, "reject_block", m))[0] == WC.INVALID
    assert m.can_reshade() == 0
