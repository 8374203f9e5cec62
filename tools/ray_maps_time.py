#!/usr/bin/env python3
"""Times sr_ray_maps against the calls beside it. After one sr_render of the
scene every leg runs calls back to back on one stream after a warm-up, one
device event between calls; the legs run one after the other in each of
--rounds interleaved rounds. One JSON line out (per scene and leg: the rounds'
medians, their median and their max - min).

Scenes: the default scene (the app's camera and textures) and the stacked
translucent layers, where every pixel's hit log fills and the end of its ray
comes from the resume path. Legs:
  all      sr_ray_maps, all nine maps (84 bytes written per pixel)
  lens     `end` and `sky_uv` alone (12 bytes)
  id       `id` alone
  pick     sr_pick_map
  reshade  sr_reshade
  render   sr_render (it leaves the same retained frame: the legs after it see what the legs before it saw)
The yardsticks are reshade and render of the same session; the one condition
is all < render on the default scene (otherwise tracing again would do as well).

  python tools/ray_maps_time.py [--width 1920 --height 1080 --steps 2000] [--out FILE]
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

LEGS = ("all", "lens", "id", "pick", "reshade", "render")


def median(v):
    s = sorted(v)
    return s[len(s) // 2]


def stacked_scene(abi, sc, n_translucent=4, gap=0.5):
    """Four translucent layers and an opaque one behind them across the camera's view (the suite's
    stacked-layer cell): every ray logs four translucent hits and is walked on by the resume path."""
    import ctypes as C

    s = abi.Scene()
    abi.load().sr_scene_clear(C.byref(s))
    for m, col in ((0, (0.02, 0.04, 0.06, 0.3)), (1, (0.9, 0.2, 0.2, 1.0))):
        M = s.materials[m]
        for k in range(4):
            M.color[k] = col[k]
        M.ambient, M.diffuse, M.specular, M.shininess = 0.2, 0.8, 0.3, 16.0
        M.texture_index, M.normal_map_index, M.double_sided_normals = -1, -1, 1
    axes = sc._axes_from((0.0, 0.0, 1.0))  # normal +z
    for k in range(n_translucent + 1):  # three disks, then rectangles (three of each primitive at most)
        z = 10.0 - gap * k
        if k < 3:
            t, kind, idx, pos = s.disks[k].plane.transform, abi.OBJECT_DISK, k, (0.0, 2.0, z)
            s.disks[k].radius = 12.0
        else:
            t, kind, idx, pos = s.rectangles[k - 3].plane.transform, abi.OBJECT_RECTANGLE, k - 3, (-8.0, 10.0, z)
            s.rectangles[k - 3].width = s.rectangles[k - 3].height = 16.0
        for i in range(3):
            t.pos[i] = pos[i]
        for i in range(9):
            t.axes[i] = axes[i]
        o = s.objects[k]
        o.type, o.index, o.material_index = kind, idx, int(k == n_translucent)
    s.num_objects = n_translucent + 1
    s.num_lights = 1
    L = s.lights[0]
    for i in range(3):
        L.transform.pos[i] = (0.0, 5.0, 14.0)[i]
        L.color[i] = 1.0
    L.intensity, L.attenuation_constant, L.attenuation_linear, L.attenuation_quadratic = 5.0, 1.0, 0.09, 0.032
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--calls", type=int, default=20, help="timed calls per leg and round")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--textures", choices=["assets", "standin"], default="assets")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    W, H = args.width, args.height
    import torch

    import srpkg

    pkg = srpkg.load_package()
    abi, sc = pkg.abi, pkg.scenes
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    if args.textures == "assets":
        bg = pkg.assets.skybox("2k")
        arr, _, _ = pkg.assets.texture_array()
    else:
        bg = sc.skybox(2048, 1024)
        arr, _, _ = sc.default_texture_array()
    params = abi.default_params(max_steps=args.steps, percent_black=-1.0)

    scenes = {"default": (lambda: sc.scene_default(textured=True), abi.default_camera()),
              "stacked": (lambda: stacked_scene(abi, sc), sc.camera_look((0.0, 2.0, 15.0), (0.0, -2.0, -15.0)))}
    r = pkg.Renderer(0)
    r.set_background(bg)
    r.set_texture_array(arr)
    frame = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
    ids = torch.empty((H, W), dtype=torch.int32, device=dev)
    results = {}
    for name, (make, cam) in scenes.items():
        r.set_scene(make())
        r.render(cam, params, W, H, out=frame, stream=stream)
        maps = r.ray_maps(stream=stream)  # the buffers of every leg
        torch.cuda.synchronize()
        pixels = W * H
        calls = {
            "all": lambda: r.ray_maps(out=maps, stream=stream),
            "lens": lambda: r.ray_maps(("end", "sky_uv"), out=maps, stream=stream),
            "id": lambda: r.ray_maps(("id",), out=maps, stream=stream),
            "pick": lambda: r.pick_map(out=ids, stream=stream),
            "reshade": lambda: r.reshade(out=frame, stream=stream),
            "render": lambda: r.render(cam, params, W, H, out=frame, stream=stream),
        }
        legs = [{"leg": n, "ms_median": [], "ms_min": []} for n in LEGS]
        for _ in range(args.rounds):
            for res in legs:
                call = calls[res["leg"]]
                for _ in range(args.warmup):
                    call()
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.calls + 1)]
                ev[0].record(stream)
                for i in range(args.calls):
                    call()
                    ev[i + 1].record(stream)
                torch.cuda.synchronize()
                ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(args.calls))
                res["ms_median"].append(round(ms[len(ms) // 2], 4))
                res["ms_min"].append(round(ms[0], 4))
        by = {}
        for res in legs:
            res["ms"] = median(res["ms_median"])
            res["spread_ms"] = round(max(res["ms_median"]) - min(res["ms_median"]), 4)
            by[res["leg"]] = res["ms"]
        written = sum(n * 4 for n, _ in abi.RAY_MAPS.values()) * pixels
        results[name] = {
            "legs": legs,
            "ratios": {"all/render": round(by["all"] / by["render"], 4), "all/reshade": round(by["all"] / by["reshade"], 4),
                       "lens/render": round(by["lens"] / by["render"], 4), "id/pick": round(by["id"] / by["pick"], 4)},
            "all_bytes_written": written, "all_write_gbytes_per_s": round(written / (by["all"] * 1e6), 1),
            "all_below_render": by["all"] < by["render"],
        }
    line = json.dumps({"tool": "ray_maps_time", "width": W, "height": H, "steps": args.steps, "calls": args.calls,
                       "warmup": args.warmup, "rounds": args.rounds, "textures": args.textures, "scenes": results,
                       "diag": r.diag_counters()})
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    r.close()


if __name__ == "__main__":
    main()
