#!/usr/bin/env python3
"""Times sr_reshade against sr_render of the same frame, and sr_pick_map:
every leg runs frames back to back on one stream after a warm-up, one device
event between frames; the legs run one after the other in each of --rounds
interleaved rounds. One JSON line out (per leg: the rounds' medians and their
median).

Scenes (--scenes, comma-separated): default, ss2 (the default scene through
sr_render_ss at ss 2), stress (scenes.scene_stress, the max-capacity scene),
overlay (the default scene with scenes.test_ray_overlay visible).
Legs per scene:
  render   the scene's launch (sr_render / sr_render_ss), on --render-lib when
           given (another build of the library, e.g. the parent commit's, in a
           context of its own), else on this tree's
  reshade  sr_reshade of that launch's retained frame (this tree's library),
           after a shading-only sr_set_scene
  pick     sr_pick_map of it (not for ss2: SR_E_NOT_READY)
(run under `rocprofv3 --kernel-trace --stats` for the kernels' own durations)

  python tools/reshade_time.py [--width 1920 --height 1080 --steps 2000]
  python tools/reshade_time.py --render-lib path/to/parent/libsr.so
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def median(v):
    s = sorted(v)
    return s[len(s) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="default,ss2,stress,overlay")
    ap.add_argument("--legs", default="render,reshade,pick")
    ap.add_argument("--render-lib", default=None, help="the library of the render leg (default: this tree's)")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--textures", choices=["assets", "standin"], default="assets")
    args = ap.parse_args()
    import torch

    import srpkg

    pkg = srpkg.load_package()
    abi, sc = pkg.abi, pkg.scenes
    W, H = args.width, args.height
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    if args.textures == "assets":
        bg = pkg.assets.skybox("2k")
        arr, _, _ = pkg.assets.texture_array()
    else:
        bg = sc.skybox(2048, 1024)
        arr, _, _ = sc.default_texture_array()
    params = abi.default_params(max_steps=args.steps, percent_black=-1.0)
    cam = abi.default_camera()
    other = abi.load(args.render_lib) if args.render_lib else None

    def relit(scene):
        """A shading-only change: a light moved and dimmed, a colour's rgb."""
        s = sc.struct_from_bytes(abi.Scene, sc.struct_bytes(scene))
        s.lights[0].transform.pos[0] += 1.0
        s.lights[0].intensity *= 0.75
        s.materials[1].color[0] *= 0.5
        assert abi.scene_shading_only(scene, s)
        return s

    def context(lib, scene, overlay):
        r = pkg.Renderer(0, lib=lib)
        r.set_scene(scene)
        r.set_background(bg)
        r.set_texture_array(arr)
        if overlay:
            r.set_test_ray(sc.test_ray_overlay())
        return r

    makers = {
        "default": (lambda: sc.scene_default(textured=True), 1, False),
        "ss2": (lambda: sc.scene_default(textured=True), 2, False),
        "stress": (sc.scene_stress, 1, False),
        "overlay": (lambda: sc.scene_default(textured=True), 1, True),
    }
    out = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
    ids = torch.empty((H, W), dtype=torch.int32, device=dev)
    legs, keep = [], []
    for name in [n for n in args.scenes.split(",") if n]:
        make, ss, overlay = makers[name]
        scene = make()
        mine = context(None, scene, overlay)
        theirs = context(other, scene, overlay) if other is not None else mine
        keep += [mine, theirs]

        def render(r=theirs, ss=ss):
            if ss > 1:
                r.render_ss(cam, params, W, H, ss, out=out, stream=stream)
            else:
                r.render(cam, params, W, H, out=out, stream=stream)

        def retain(r=mine, ss=ss, scene=scene):
            """This tree's launch of the frame, then the shading-only change."""
            r.set_scene(scene)
            render(r, ss)
            r.set_scene(relit(scene))
            assert r.can_reshade()

        frames = {"render": render, "reshade": lambda r=mine: r.reshade(out=out, stream=stream),
                  "pick": lambda r=mine: r.pick_map(out=ids, stream=stream)}
        for leg in [n for n in args.legs.split(",") if n]:
            if leg == "pick" and ss > 1:
                continue
            legs.append({"scene": name, "leg": leg, "lib": "render-lib" if leg == "render" and other is not None else "this",
                         "before": None if leg == "render" else retain, "frame": frames[leg],
                         "ms_median": [], "ms_min": [], "ms_mean": []})
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for res in legs:
            if res["before"]:
                res["before"]()
            for _ in range(args.warmup):
                res["frame"]()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.frames + 1)]
            ev[0].record(stream)
            for i in range(args.frames):
                res["frame"]()
                ev[i + 1].record(stream)
            torch.cuda.synchronize()
            ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(args.frames))
            res["ms_median"].append(round(ms[len(ms) // 2], 4))
            res["ms_min"].append(round(ms[0], 4))
            res["ms_mean"].append(round(ev[0].elapsed_time(ev[-1]) / args.frames, 4))
    for res in legs:
        res["ms"] = median(res["ms_median"])
        del res["before"], res["frame"]
    diag = {}
    for r in {id(r): r for r in keep}.values():
        for k, v in r.diag_counters().items():
            diag[k] = diag.get(k, 0) + v
    print(json.dumps({
        "tool": "reshade_time", "width": W, "height": H, "steps": args.steps, "frames": args.frames,
        "warmup": args.warmup, "rounds": args.rounds, "textures": args.textures, "render_lib": args.render_lib,
        "legs": legs, "diag": diag,
    }))
    for r in {id(r): r for r in keep}.values():
        r.close()


if __name__ == "__main__":
    main()
