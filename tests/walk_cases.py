"""Model-checked walks over the C ABI (a helper, not a test module).

sr.h promises that a context's history never reaches the bytes: a call writes
what a fresh context in the same declared state would write. The walks are
sequences of ABI calls ("ops") on one long-lived context, generated from a
seed, with a small model of the declared state and of sr.h's rules beside
them. tests/test_walk_cases.py shows on the CPU that the walks can catch what
they are meant to catch; tests/test_gpu_context_walk.py runs them.

An op is a dict: "kind" and its arguments, all plain data (names of scenes,
cameras and textures, numbers, lists). Regenerating a walk from its seed gives
the same list. Names are resolved by Resolver from the existing case modules:
scenes, cameras and the test ray of test_gpu_launch_matrix.World, the relit
scenes of reshade_cases, the sequences of sequence_cases.

The catalogue (sr.h's entry list):
  SETTERS      set_scene_geo, set_scene_shade (sr_set_scene: another geometry /
               reshade_cases.relit of the current one, or back), set_test_ray
               (off, on, replaced), set_sequence (load, replace, clear),
               set_background, set_texture_array, set_projection, set_split,
               set_latency, set_culling
  LAUNCHES     every entry point that renders; RETAINING of them leave a
               retained frame when they render at least one row
  CONSUMERS    reshade, reshade_debug, pick_map, ray_maps, can_reshade
  UNTOUCHING   trace_rays, trace_ray_maps and one late-rejected call per launch
               family: reject_pitch (sr_render, pitch below 4 w), reject_block
               (sr_render_block_list, a block index past the frame),
               reject_window (sr_render_sequence, a window past the end)

Model: the rules of sr.h "Retained frames", "Scene sequences", "Shutter
frames", "Ray queries" and "Projections", restated here (Model.step), and the
order of a launch's rejections that tests/test_gpu_rejections.py pins: an entry
point's own arguments (the block list's indices among them), then the context
(SR_E_NOT_READY without a scene, or without a sequence for a sequence launch),
then the window, then pitch and frame stride.
"""
from __future__ import annotations

import numpy as np

OK, INVALID, NOT_READY = 0, -1, -5  # sr_status

SHAPES = ((1, 1), (33, 17), (68, 44), (40, 24), (17, 33))  # the last two: more grid shapes for the caches
STEPS = (0, 7, 64, 300)
REVS = (1, 2, 4)
UFS = (0.01, 0.02)
SCENES = ("small", "general", "large", "stacked", "empty")
# the scenes whose 33x17 frame shows the texture array / the background on 1 % of
# its pixels at least (tests/test_walk_cases.py holds every setter op to that)
TEXTURED = ("small", "general", "large")
SKY = ("small", "general", "empty")
RAYS = ("off", "on", "on2")
SEQUENCES = {"MIX": 6, "GEO8": 8, "SHADE8": 8}  # name -> scenes
BACKGROUNDS = ("bgA", "bgB", "bgC")
TEXTURES = ("texA", "texB")
SPLITS = ((0, 16, 1), (4, 16, 1), (32, 4, 1), (8, 1, 50))
CAMS = ("view", "fly1", "fly5")
BLOCK_ROWS = 8

SETTERS = ("set_scene_geo", "set_scene_shade", "set_test_ray", "set_sequence", "set_background",
           "set_texture_array", "set_projection", "set_split", "set_latency", "set_culling")
RETAINING = ("render", "render_blocks", "render_blocks_batch", "render_block_list", "render_debug", "render_phase",
             "render_ss", "render_block_list_ss")
OWN_NO_FRAME = ("render_accumulate", "render_adaptive", "wave_costs")
SEQ_LAUNCHES = ("render_sequence", "render_sequence_block_list", "render_sequence_debug")
SHUTTER_LAUNCHES = ("render_shutter", "render_shutter_block_list", "accumulate_shutter")
LAUNCHES = RETAINING + OWN_NO_FRAME + SEQ_LAUNCHES + SHUTTER_LAUNCHES
CONSUMERS = ("reshade", "reshade_debug", "pick_map", "ray_maps", "can_reshade")
TRACES = ("trace_rays", "trace_ray_maps")
REJECTS = ("reject_pitch", "reject_block", "reject_window")
UNTOUCHING = TRACES + REJECTS
KINDS = SETTERS + LAUNCHES + CONSUMERS + UNTOUCHING
# the kinds that write output when they succeed
OUTPUT_KINDS = LAUNCHES + CONSUMERS[:4] + TRACES
# the setters sr.h says change pixels, and the ones it says do not
PIXEL_SETTERS = ("set_scene_geo", "set_scene_shade", "set_test_ray", "set_sequence", "set_background",
                 "set_texture_array", "set_projection")
# the rules of the retained frame, counted where a frame was valid before the op
DROP_RULES = ("drop:set_texture_array", "drop:set_test_ray", "drop:set_scene_geo", "drop:projection_changed",
              "drop:render_adaptive", "drop:render_accumulate", "drop:wave_costs", "drop:zero_rows",
              "drop:sequence_launch", "drop:shutter_launch")
KEEP_RULES = ("keep:set_background", "keep:set_scene_shade", "keep:set_split", "keep:set_latency", "keep:set_culling",
              "keep:projection_same", "keep:set_sequence", "keep:trace", "keep:consumer", "keep:rejected",
              "replace:launch")

RANDOM_SEEDS = (101, 102, 103, 104, 105, 106, 107, 108)
RANDOM_LENGTH = 60


def base_of(scene):
    return scene.split("~")[0]


def blocks_rows(h, block_rows, first, step):
    """(rows of the packed output buffer, frame rows rendered) of sr_render_blocks"""
    nb = len(range(first, -(-h // block_rows), step))
    rows = sum(min(block_rows, h - b * block_rows) for b in range(first, -(-h // block_rows), step))
    return nb * block_rows, rows


def out_shape(op):
    """(width, output rows, frames, ss) of a retaining launch's output"""
    k, w, h = op["kind"], op["w"], op["h"]
    ss = op.get("ss", 1) if k in ("render_ss", "render_block_list_ss") else 1
    if k in ("render", "render_debug", "render_phase", "render_ss"):
        return w, op["y1"] - op["y0"], 1, ss
    if k in ("render_blocks", "render_blocks_batch"):
        return w, blocks_rows(h, BLOCK_ROWS, op["first"], op["step"])[0], len(op["cams"]), ss
    if k in ("render_block_list", "render_block_list_ss"):
        return w, len(op["blocks"]) * BLOCK_ROWS, len(op["cams"]), ss
    raise ValueError(k)


def rendered_rows(op):
    """Frame rows a launch renders (0: sr.h's "launch of zero rows")"""
    k = op["kind"]
    if "y0" in op:
        return op["y1"] - op["y0"]
    if k in ("render_blocks", "render_blocks_batch"):
        return blocks_rows(op["h"], BLOCK_ROWS, op["first"], op["step"])[1]
    if "blocks" in op:
        return len(op["blocks"]) * BLOCK_ROWS
    return op["h"]


class Model:
    """The declared state of a context and sr.h's rules for it."""

    def __init__(self):
        self.scene = None
        self.ray = "off"
        self.seq = None
        self.bg = None
        self.tex = None
        self.projection = 0
        self.split = SPLITS[0]
        self.latency = 0
        self.culling = 1
        self.retained = None  # the op of the retained call

    def declared(self):
        return {"scene": self.scene, "ray": self.ray, "seq": self.seq, "bg": self.bg, "tex": self.tex,
                "projection": self.projection}

    def can_reshade(self):
        return 1 if self.retained is not None else 0

    def _window_ok(self, first, n):
        return self.seq is not None and 0 <= first and first + n <= SEQUENCES[self.seq]

    def step(self, op):
        """(status, rule) of the op, and the state after it. rule: the name of
        the retained-frame rule that applied, None where sr.h has none."""
        k = op["kind"]
        had = self.retained is not None
        rule = None
        if k in SETTERS:
            status = OK
            if k == "set_scene_geo":
                assert self.scene is None or base_of(op["scene"]) != base_of(self.scene)
                self.scene, rule = op["scene"], "drop:set_scene_geo"
                self.retained = None
            elif k == "set_scene_shade":
                # shading-only fields at most: lights and the materials' Phong terms (reshade_cases.relit)
                assert base_of(op["scene"]) == base_of(self.scene)
                self.scene, rule = op["scene"], "keep:set_scene_shade"
            elif k == "set_test_ray":
                self.ray, rule = op["ray"], "drop:set_test_ray"
                self.retained = None
            elif k == "set_sequence":
                # the sequence and the context's own scene are independent states
                self.seq, rule = op["seq"], "keep:set_sequence"
            elif k == "set_background":
                self.bg, rule = op["bg"], "keep:set_background"
            elif k == "set_texture_array":
                self.tex, rule = op["tex"], "drop:set_texture_array"
                self.retained = None
            elif k == "set_projection":
                if op["projection"] != self.projection:
                    self.projection, rule = op["projection"], "drop:projection_changed"
                    self.retained = None
                else:
                    rule = "keep:projection_same"
            elif k == "set_split":
                self.split, rule = tuple(op["split"]), "keep:set_split"
            elif k == "set_latency":
                self.latency, rule = op["on"], "keep:set_latency"
            elif k == "set_culling":
                self.culling, rule = op["on"], "keep:set_culling"
        elif k in LAUNCHES:
            seq_launch = k in SEQ_LAUNCHES or (k in SHUTTER_LAUNCHES and op["first"] >= 0)
            if seq_launch:
                n = 1 if k == "render_sequence_debug" else len(op["cams"])
                status = NOT_READY if self.seq is None else OK if self._window_ok(op["first"], n) else INVALID
            else:
                status = NOT_READY if self.scene is None else OK
            if status == OK:
                if k in RETAINING and rendered_rows(op) > 0:
                    self.retained, rule = op, "replace:launch"
                else:
                    self.retained = None
                    rule = ("drop:zero_rows" if k in RETAINING else "drop:sequence_launch" if k in SEQ_LAUNCHES
                            else "drop:shutter_launch" if k in SHUTTER_LAUNCHES else "drop:" + k)
            else:
                rule = "keep:rejected"
        elif k in CONSUMERS:
            rule = "keep:consumer"
            r = self.retained
            if k == "can_reshade":
                status = OK
            elif r is None:
                status = NOT_READY
            else:
                _, _, frames, ss = out_shape(r)
                if k == "reshade":
                    status = OK
                elif k == "reshade_debug":
                    status = OK if frames == 1 and ss == 1 else INVALID
                else:  # the picking surface is the plain frame
                    status = OK if ss == 1 else NOT_READY
        elif k in TRACES:
            status, rule = (NOT_READY if self.scene is None else OK), "keep:trace"
        elif k in REJECTS:
            rule = "keep:rejected"
            if k == "reject_block":
                status = INVALID  # the list is the entry point's own argument: checked first
            elif k == "reject_pitch":
                status = NOT_READY if self.scene is None else INVALID
            else:
                status = NOT_READY if self.seq is None else INVALID
        else:
            raise ValueError(k)
        return status, (rule if had else None)


# ---- the generator -------------------------------------------------------------------

def _pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def _other(rng, seq, cur):
    return _pick(rng, [v for v in seq if v != cur])


def _frame(rng, shape=None):
    w, h = shape if shape is not None else _pick(rng, SHAPES)
    return {"w": int(w), "h": int(h), "steps": int(_pick(rng, STEPS)), "revs": int(_pick(rng, REVS)),
            "uf": float(_pick(rng, UFS)), "stream": int(rng.integers(2))}


def _band(rng, h, allow_zero=False):
    mode = int(rng.integers(4 if allow_zero else 3))
    if mode == 3:
        return (h // 2, h // 2)
    if mode == 0 or h < 3:
        return (0, h)
    return (h // 3, h - h // 4) if mode == 1 else (h - 1, h)


def _cams(rng, lo, hi):
    return [_pick(rng, CAMS) for _ in range(int(rng.integers(lo, hi + 1)))]


def _blocks(rng, h):
    """A list with -1 padding; its last real block may hold the frame's partial rows"""
    nb = -(-h // BLOCK_ROWS)
    real = [int(rng.integers(nb)) for _ in range(int(rng.integers(1, 3)))]
    out = real + [-1]
    if rng.integers(2):
        out = [-1] + out
    if rng.integers(2):
        out.append(nb - 1)
    return out


def _phases(rng, ss, n):
    return [[int(rng.integers(ss)), int(rng.integers(ss))] for _ in range(n)]


def make_op(rng, kind, m, shape=None):
    """An op of `kind` drawn for the model state m (its arguments are valid in
    m wherever the kind can succeed at all). None: the kind has no op in m."""
    op = {"kind": kind}
    if kind == "set_scene_geo":
        op["scene"] = _other(rng, SCENES, None if m.scene is None else base_of(m.scene))
    elif kind == "set_scene_shade":
        if m.scene is None or base_of(m.scene) == "empty":
            return None  # nothing to relight
        op["scene"] = base_of(m.scene) if "~" in m.scene else m.scene + "~relit"
    elif kind == "set_test_ray":
        op["ray"] = _other(rng, RAYS, m.ray)
    elif kind == "set_sequence":
        op["seq"] = _other(rng, tuple(SEQUENCES) + (None,), m.seq)
    elif kind == "set_background":
        if m.bg is not None and (m.scene is None or base_of(m.scene) not in SKY):
            return None  # the frame would not show it
        op["bg"] = _other(rng, BACKGROUNDS, m.bg)
    elif kind == "set_texture_array":
        if m.tex is not None and (m.scene is None or base_of(m.scene) not in TEXTURED):
            return None  # the frame would not show it
        op["tex"] = _other(rng, TEXTURES, m.tex)
    elif kind == "set_projection":
        op["projection"] = m.projection if rng.integers(4) == 0 else _other(rng, (0, 1, 2), m.projection)
    elif kind == "set_split":
        op["split"] = list(_other(rng, SPLITS, m.split))
    elif kind in ("set_latency", "set_culling"):
        op["on"] = 1 - (m.latency if kind == "set_latency" else m.culling)
    elif kind in LAUNCHES:
        op.update(_frame(rng, shape))
        h = op["h"]
        n_seq = SEQUENCES[m.seq] if m.seq is not None else 6
        if kind in ("render", "render_debug", "render_phase", "render_ss"):
            op["cams"] = _cams(rng, 1, 1)
            op["y0"], op["y1"] = _band(rng, h, allow_zero=kind == "render")
        if kind in ("render_blocks", "render_blocks_batch"):
            op["cams"] = _cams(rng, 1, 1) if kind == "render_blocks" else _cams(rng, 2, 3)
            op["first"], op["step"] = int(rng.integers(2)), int(rng.integers(1, 3))
        if kind in ("render_block_list", "render_block_list_ss"):
            op["cams"] = _cams(rng, 1, 3 if kind == "render_block_list" else 2)
            op["blocks"] = _blocks(rng, h)
        if kind in ("render_ss", "render_block_list_ss", "render_phase", "render_accumulate", "render_adaptive"):
            op["ss"] = int(rng.integers(2, 4))
        if kind == "render_phase":
            op["px"], op["py"] = _phases(rng, op["ss"], 1)[0]
        if kind == "render_accumulate":
            op["cams"] = _cams(rng, 1, 1)
            op["phases"] = _phases(rng, op["ss"], int(rng.integers(1, 4)))
        if kind == "render_adaptive":
            op["cams"] = _cams(rng, 1, 1)
            op["threshold"], op["grow"] = int(_pick(rng, (-1, 24, 255))), int(rng.integers(2))
        if kind == "wave_costs":
            op["cams"] = _cams(rng, 1, 1)
        if kind in ("render_sequence", "render_sequence_block_list"):
            op["cams"] = _cams(rng, 1, 3)
            op["first"] = int(rng.integers(n_seq - len(op["cams"]) + 1))
            op["ss"] = int(_pick(rng, (1, 1, 2)))
            if kind == "render_sequence":
                op["y0"], op["y1"] = _band(rng, h)
            else:
                op["blocks"] = _blocks(rng, h)
        if kind == "render_sequence_debug":
            op["cams"] = _cams(rng, 1, 1)
            op["first"] = int(rng.integers(n_seq))
            op["y0"], op["y1"] = _band(rng, h)
        if kind in SHUTTER_LAUNCHES:
            own = m.seq is None or rng.integers(2) == 0
            if kind == "accumulate_shutter":
                op["K"], op["M"] = int(rng.integers(1, 4)), 1
            else:
                op["K"], op["M"] = int(rng.integers(1, 3)), int(rng.integers(1, 3))
            n = op["K"] * op["M"]
            op["cams"] = [_pick(rng, CAMS) for _ in range(n)]
            op["first"] = -1 if own else int(rng.integers(n_seq - n + 1))
            op["ss"] = int(rng.integers(1, 3))
            if kind == "render_shutter_block_list":
                op["blocks"] = _blocks(rng, h)
            else:
                op["y0"], op["y1"] = _band(rng, h)
    elif kind in CONSUMERS:
        op["stream"] = int(rng.integers(2))
    elif kind in TRACES:
        op.update(_frame(rng, (8, 4)))  # the rays of an 8 x 4 frame of the camera
        op["cams"] = _cams(rng, 1, 1)
    elif kind in REJECTS:
        op.update(_frame(rng, shape))
        op["cams"] = _cams(rng, 1, 2)
        if kind == "reject_block":
            op["blocks"] = [0, -(-op["h"] // BLOCK_ROWS), -1]
        if kind == "reject_window":
            n_seq = SEQUENCES[m.seq] if m.seq is not None else 6
            op["first"] = n_seq - len(op["cams"]) + 1
    else:
        raise ValueError(kind)
    return op


def _append(ops, m, op):
    m.step(op)
    ops.append(op)


def prologue(rng, ops, m):
    """Textures, calls on a context without a scene, then a scene"""
    _append(ops, m, make_op(rng, "set_background", m))
    _append(ops, m, make_op(rng, "set_texture_array", m))
    _append(ops, m, make_op(rng, _pick(rng, RETAINING), m))
    _append(ops, m, make_op(rng, _pick(rng, CONSUMERS[:4] + UNTOUCHING), m))
    _append(ops, m, make_op(rng, "set_scene_geo", m))


def random_walk(seed, length=RANDOM_LENGTH):
    rng = np.random.default_rng(seed)
    ops, m = [], Model()
    prologue(rng, ops, m)
    while len(ops) < length:
        u = rng.random()
        if m.retained is not None and u < 0.30:
            group = CONSUMERS  # a valid frame is there to be used
        elif u < 0.55:
            group = SETTERS
        elif u < 0.85:
            group = LAUNCHES
        elif u < 0.93:
            group = CONSUMERS
        else:
            group = UNTOUCHING
        op = make_op(rng, _pick(rng, group), m)
        if op is not None:
            _append(ops, m, op)
    return ops


def setter_output_pairs(ops):
    """The ordered pairs (setter kind, kind of the next op that produces
    output) of a walk from its start. A pair counts where the model says the
    output op succeeds, so that it writes and is compared with the fresh
    context; SR_E_NOT_READY counts only for a consumer right after a setter
    that dropped the retained frame, which is the one thing that pair can do."""
    m, pairs, last = Model(), set(), None
    for op in ops:
        k = op["kind"]
        had = m.retained is not None
        status, _ = m.step(op)
        if k in SETTERS:
            last = (k, had and m.retained is None)
        elif k in OUTPUT_KINDS:
            if last is not None and (status == OK or (status == NOT_READY and k in CONSUMERS and last[1])):
                pairs.add((last[0], k))
            last = None
    return pairs


def pair_walk(covered):
    """Scripted: every retained-frame rule with a valid frame before it, then
    every (setter, output kind) pair missing from `covered`."""
    rng = np.random.default_rng(7)
    ops, m = [], Model()
    prologue(rng, ops, m)
    shape = (33, 17)

    def ready(kind):
        """The state in which an op of `kind` does what it is here for"""
        if kind in ("set_scene_shade", "set_texture_array", "set_background") and base_of(m.scene) not in (
                "small", "general"):
            _append(ops, m, {"kind": "set_scene_geo", "scene": "small"})
        if m.seq is None and (kind in SEQ_LAUNCHES or kind in SHUTTER_LAUNCHES):
            _append(ops, m, make_op(rng, "set_sequence", m))

    def frame():
        op = make_op(rng, "render", m, shape)
        op["y0"], op["y1"] = 0, op["h"]
        _append(ops, m, op)

    def use():
        _append(ops, m, make_op(rng, "reshade", m))

    # the rules, each twice: a frame, the op, a consumer
    for _ in range(2):
        for kind in SETTERS + OWN_NO_FRAME + ("render_sequence", "render_shutter", "trace_rays", "reject_pitch"):
            ready(kind)
            frame()
            _append(ops, m, make_op(rng, kind, m, shape))
            use()
        frame()  # the same projection again keeps the frame
        _append(ops, m, {"kind": "set_projection", "projection": m.projection})
        use()
        frame()  # a launch of zero rows leaves none
        op = make_op(rng, "render", m, shape)
        op["y0"] = op["y1"] = 5
        _append(ops, m, op)
        use()
    # the pairs
    have = set(covered) | setter_output_pairs(ops)
    for s in SETTERS:
        for k in OUTPUT_KINDS:
            if (s, k) in have:
                continue
            ready(s)
            if s != "set_sequence":
                ready(k)
            if k in CONSUMERS:
                frame()  # a frame for the setter to keep or to drop
            op = make_op(rng, s, m)
            if s == "set_sequence" and op["seq"] is None and k in SEQ_LAUNCHES + SHUTTER_LAUNCHES:
                op["seq"] = _other(rng, tuple(SEQUENCES), m.seq)
            if s == "set_projection" and op["projection"] == m.projection:
                op["projection"] = _other(rng, (0, 1, 2), m.projection)
            _append(ops, m, op)
            _append(ops, m, make_op(rng, k, m, _pick(rng, SHAPES[:3])))
    missing = [(s, k) for s in SETTERS for k in OUTPUT_KINDS if (s, k) not in have | setter_output_pairs(ops)]
    assert not missing, missing
    return ops


def _launch(kind, w, h, steps, revs, uf=UFS[0], stream=0, **kw):
    op = {"kind": kind, "w": w, "h": h, "steps": steps, "revs": revs, "uf": uf, "stream": stream, "cams": ["view"]}
    op.update(kw)
    return op


def pressure_walk():
    """Scripted: each of the four caches through more distinct keys than it
    holds (device_cache.h: eight), then back to an evicted key."""
    rng = np.random.default_rng(11)
    ops, m = [], Model()
    prologue(rng, ops, m)
    if base_of(m.scene) != "general":
        _append(ops, m, {"kind": "set_scene_geo", "scene": "general"})
    _append(ops, m, {"kind": "set_sequence", "seq": "MIX"})
    w, h = 33, 17
    tables = [(s, r) for s in STEPS[1:] for r in REVS] + [(0, 2)]  # ten keys
    # step tables: ten (steps, revolutions) keys, then the first ones again
    for s, r in tables + tables[:2]:
        _append(ops, m, _launch("render", w, h, s, r, y0=0, y1=h, stream=len(ops) % 2))
    _append(ops, m, make_op(rng, "reshade", m))
    # the overlay for the rest of the walk: the frame above goes with the old test ray
    _append(ops, m, {"kind": "set_test_ray", "ray": "on"})
    _append(ops, m, make_op(rng, "reshade", m))
    # launch orders: grid shapes x split x projection, then the first ones again
    orders = [(shape, split, pj) for pj in (0, 1) for split in SPLITS[:2] for shape in SHAPES[1:4]]
    for shape, split, pj in orders[:10] + orders[:2]:
        if tuple(split) != m.split:
            _append(ops, m, {"kind": "set_split", "split": list(split)})
        if pj != m.projection:
            _append(ops, m, {"kind": "set_projection", "projection": pj})
        _append(ops, m, _launch("render", shape[0], shape[1], 64, 2, y0=0, y1=shape[1]))
        _append(ops, m, _launch("render", shape[0], shape[1], 64, 2, y0=0, y1=shape[1]))  # the learned order
    _append(ops, m, {"kind": "set_split", "split": list(SPLITS[0])})
    _append(ops, m, {"kind": "set_projection", "projection": 0})
    # block lists: ten lists of a 68x44 frame. A block-list frame is used early;
    # nine lists later its list has been evicted. Every retaining block-list
    # launch replaces the retained frame, so no call sequence evicts a list under
    # a frame that stays (device_cache.h's cascade for that is the CPU test's):
    # what the walk holds is that the frames and reshades around the eviction
    # are the fresh context's
    lists = [[b, -1, (b + 1 + k) % 6] for k in range(2) for b in range(5)]
    for i, blocks in enumerate(lists + lists[:2]):
        _append(ops, m, _launch("render_block_list", 68, 44, 64, 2, blocks=blocks, cams=["view", "fly1"]))
        if i == 1:
            _append(ops, m, make_op(rng, "reshade", m))
            _append(ops, m, make_op(rng, "pick_map", m))
        if i == 9:
            # nine lists since: the retained call's list is gone, the frame is the last launch's
            _append(ops, m, make_op(rng, "reshade", m))
    _append(ops, m, _launch("render_block_list_ss", 33, 17, 64, 2, blocks=[1, -1, 2], cams=["view"], ss=2))
    _append(ops, m, make_op(rng, "reshade", m))
    # exclusion tables: ten (u_f, step angle) pairs under a loaded sequence, then the first ones again
    xtabs = [(uf, s, r) for uf in UFS for (s, r) in ((64, 1), (64, 2), (64, 4), (300, 1), (300, 2))]
    for uf, s, r in xtabs + xtabs[:2]:
        _append(ops, m, _launch("render_sequence", w, h, s, r, uf=uf, first=1, cams=["view", "fly1"], ss=1,
                                y0=0, y1=h))
    _append(ops, m, _launch("render", w, h, 300, 2, y0=0, y1=h))
    _append(ops, m, make_op(rng, "ray_maps", m))
    return ops


def pressure_keys(ops):
    """Per cache the sequence of keys the pressure walk's launches present"""
    m = Model()
    keys = {"tables": [], "orders": [], "block_lists": [], "xtabs": []}
    for op in ops:
        status, _ = m.step(op)
        if op["kind"] not in LAUNCHES or status != OK:
            continue
        keys["tables"].append((op["steps"], op["revs"]))
        blocks = tuple(op["blocks"]) if "blocks" in op else None
        if blocks is not None:
            keys["block_lists"].append(blocks)
        ss = op.get("ss", 1) if op["kind"] in ("render_ss", "render_block_list_ss", "render_sequence") else 1
        rows = (len(blocks) * BLOCK_ROWS if blocks is not None else rendered_rows(op)) * ss
        keys["orders"].append((-(-op["w"] * ss // 16), -(-rows // 16), m.split[0], m.split[1] if m.split[0] else 0,
                               blocks, m.projection))
        if op["kind"] in SEQ_LAUNCHES:
            keys["xtabs"].append((op["uf"], op["steps"], op["revs"]))
    return keys


def lru_revisits(keys, capacity=8):
    """(distinct keys, misses on a key that was cached before and evicted) of an LRU cache"""
    cache, seen, evicted_hits = [], set(), 0
    for k in keys:
        if k in cache:
            cache.remove(k)
        else:
            if k in seen:
                evicted_hits += 1
            if len(cache) >= capacity:
                cache.pop(0)
        cache.append(k)
        seen.add(k)
    return len(seen), evicted_hits


_WALKS = {}


def walks():
    """name -> ops: the eight random walks, the pair walk and the pressure walk"""
    if not _WALKS:
        covered = set()
        for seed in RANDOM_SEEDS:
            ops = random_walk(seed)
            _WALKS[f"random-{seed}"] = ops
            covered |= setter_output_pairs(ops)
        _WALKS["pairs"] = pair_walk(covered)
        _WALKS["pressure"] = pressure_walk()
    return _WALKS


WALK_NAMES = tuple(f"random-{s}" for s in RANDOM_SEEDS) + ("pairs", "pressure")


# ---- names -> structs and arrays -------------------------------------------------------

def shading_only_fields(abi, a, b):
    """sr.h's list, restated: True when b differs from a at most in num_lights,
    lights[] and, per material, color[0..2], ambient, diffuse, specular,
    shininess and normal_map_index (bytes: a NaN equals itself)."""
    import ctypes as C

    def geometry(s):
        g = abi.Scene()
        C.memmove(C.addressof(g), C.addressof(s), C.sizeof(abi.Scene))
        g.num_lights = 0
        C.memset(C.addressof(g) + abi.Scene.lights.offset, 0, abi.Scene.lights.size)
        for i in range(abi.MAX_MATERIALS):
            mt = g.materials[i]
            mt.color[0] = mt.color[1] = mt.color[2] = 0.0
            mt.ambient = mt.diffuse = mt.specular = mt.shininess = 0.0
            mt.normal_map_index = 0
        return bytes(g)

    return geometry(a) == geometry(b)


class Resolver:
    """The structs and arrays behind an op's names, and the oracle's frame of a declared state."""

    W, H, STEPS = 33, 17, 300  # the frame in which a stale state must show

    def __init__(self, pkg, oracle, textures):
        import reshade_cases
        import sequence_cases
        import shading_cases

        self.pkg, self.oracle = pkg, oracle
        self.sq = sequence_cases.Sequences(pkg, oracle, textures)
        self.wd = self.sq.wd
        self._relit = reshade_cases.relit
        sc = pkg.scenes
        self._scenes, self._rays, self._tex, self._frames = {}, {}, {}, {}
        self.bgs = {"bgA": sc.skybox(64, 32), "bgB": shading_cases.skybox(5, 7, 3), "bgC": sc.skybox(96, 40)[::-1].copy()}
        self.texs = {"texA": sc.pad_texture_array([sc.uv_checker(60), sc.cubemap(161, 121)])[0],
                     "texB": sc.feature_texture_array()[0]}

    def scene(self, key):
        if key not in self._scenes:
            base = base_of(key)
            s = self.pkg.scenes.scene_black_hole_only() if base == "empty" else self.wd.scene(base)
            self._scenes[key] = self._relit(self.pkg, s) if key.endswith("~relit") else s
        return self._scenes[key]

    def ray(self, key):
        """off: the default; on: World's press-R overlay, thick enough for a
        33x17 frame; on2: replaced (another radius, the colours exchanged)"""
        if key not in self._rays:
            sc, abi = self.pkg.scenes, self.pkg.abi
            if key == "off":
                t = self.wd.test_rays[False]
            else:
                t = sc.struct_from_bytes(abi.TestRay, sc.struct_bytes(self.wd.test_rays[True]))
                t.radius = 0.35 if key == "on" else 0.8
                if key == "on2":
                    for k in range(4):
                        t.curved_color[k], t.flat_color[k] = t.flat_color[k], t.curved_color[k]
            self._rays[key] = t
        return self._rays[key]

    def sequence(self, name):
        return self.sq.scenes(name)

    def cam(self, name):
        return self.wd.cams[name]

    def params(self, op):
        return self.wd.params(op["steps"], max_revolutions=op["revs"], u_f=op["uf"])

    def texset(self, bg, tex):
        if (bg, tex) not in self._tex:
            self._tex[(bg, tex)] = self.oracle.TextureSet(self.bgs[bg], self.texs[tex])
        return self._tex[(bg, tex)]

    def frame(self, scene, ray, bg, tex):
        """The oracle's (rgba8, float rgba, steps) of a declared state: camera
        "view", 33x17, 300 steps, the pinhole (read-only)."""
        key = (scene, ray, bg, tex)
        if key not in self._frames:
            s = self.scene(scene) if isinstance(scene, str) else self.sequence(scene[0])[scene[1]]
            out = self.oracle.render(s, self.cam("view"), self.wd.params(self.STEPS), self.W, self.H,
                                     self.texset(bg, tex), self.ray(ray))
            for a in out:
                a.setflags(write=False)
            self._frames[key] = out
        return self._frames[key]
