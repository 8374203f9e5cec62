#!/usr/bin/env python3
"""Times an animation of the scene three ways (sr.h "Scene sequences"): the
default scene with its sphere on a circular orbit, --scenes positions (16),
1920 x 1080 at 2000 steps, the app's camera. Milliseconds per frame by the
host's clock around each leg (the first leg waits on the host by its nature),
each leg after a warm-up, the legs one after the other in each of --rounds
interleaved rounds. One JSON line out.

  a  the loop without sequences: sr_set_scene + sr_render per frame. With
     --parent-lib on a library built from the parent commit (as
     tools/bench_ab.sh takes one through SR_LIB), else on this tree's.
  b  sr_render_sequence, all scenes in one launch, launches queued back to back
  c  sr_render_blocks_batch of as many cameras on the static scene: the ceiling

  python tools/sequence_time.py [--parent-lib lib/variants/libsr_parent.so --passes 6 --rounds 5]
"""
import argparse
import json
import math
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def median(v):
    s = sorted(v)
    return s[len(s) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libsr.so of the parent commit for leg a")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--scenes", type=int, default=16)
    ap.add_argument("--passes", type=int, default=6, help="times each leg runs over the animation per round")
    ap.add_argument("--warmup", type=int, default=2, help="untimed passes ahead of them")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--textures", choices=["assets", "standin"], default="assets")
    args = ap.parse_args()
    import torch

    import srpkg

    pkg = srpkg.load_package()
    abi, sc = pkg.abi, pkg.scenes
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    n, W, H = args.scenes, args.width, args.height
    scenes = []
    for k in range(n):
        s = sc.scene_default(textured=True)
        pos = s.spheres[0].transform.pos
        radius, phase = math.hypot(pos[0], pos[2]), math.atan2(pos[2], pos[0])
        pos[0] = radius * math.cos(phase + 2.0 * math.pi * k / n)
        pos[2] = radius * math.sin(phase + 2.0 * math.pi * k / n)
        scenes.append(s)
    if args.textures == "assets":
        bg = pkg.assets.skybox("2k")
        arr, _, _ = pkg.assets.texture_array()
    else:
        bg = sc.skybox(2048, 1024)
        arr, _, _ = sc.default_texture_array()

    def renderer(lib=None):
        r = pkg.Renderer(0, lib=lib)
        r.set_scene(scenes[0])
        r.set_background(bg)
        r.set_texture_array(arr)
        return r

    cur = renderer()
    old = renderer(abi.load(args.parent_lib)) if args.parent_lib else cur
    cur.set_scene_sequence(scenes)
    params = abi.default_params(max_steps=args.steps, percent_black=-1.0)
    cam = abi.default_camera()
    cams = [cam] * n
    out = torch.empty((n, H, W, 4), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def leg_a():
        for k in range(n):
            old.set_scene(scenes[k])
            old.render(cam, params, W, H, out=out[k], stream=stream)

    def leg_b():
        cur.render_sequence(0, cams, params, W, H, out=out, stream=stream)

    def leg_c():
        cur.render_blocks_batch(cams, params, W, H, H, 0, 1, out=out, stream=stream)

    legs = {"a": leg_a, "b": leg_b, "c": leg_c}
    ms = {k: [] for k in legs}
    for _ in range(args.rounds):
        for name, leg in legs.items():
            if name == "c":
                cur.set_scene(scenes[0])
            for _ in range(args.warmup):
                leg()
            stream.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.passes):
                leg()
            stream.synchronize()
            ms[name].append(round((time.perf_counter() - t0) * 1e3 / (args.passes * n), 4))
    med = {k: median(v) for k, v in ms.items()}
    print(json.dumps({
        "tool": "sequence_time", "width": W, "height": H, "steps": args.steps, "scenes": n, "passes": args.passes,
        "warmup": args.warmup, "rounds": args.rounds, "textures": args.textures,
        "leg_a_library": "parent" if args.parent_lib else "this tree",
        "ms_per_frame": ms, "ms_per_frame_median": med,
        "a_spread": round(max(ms["a"]) - min(ms["a"]), 4),
        "a_minus_b": round(med["a"] - med["b"], 4), "b_over_c": round(med["b"] / med["c"], 4),
        "diag": cur.diag_counters(),
    }))
    if old is not cur:
        old.close()
    cur.close()


if __name__ == "__main__":
    main()
