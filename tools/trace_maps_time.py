#!/usr/bin/env python3
"""Times sr_trace_ray_maps beside sr_trace_rays on the same rays in the same
session, and prints one JSON line.

The rays are the headline frame's own camera rays (sr_camera_rays of the
app's camera, 1920 x 1080, default scene, the reference's textures) in
tools/trace_time.py's three orders: the frame kernels' 8x8 wave tiles,
row-major, shuffled. Legs, per order:
  trace   sr_trace_rays with all four outputs (28 bytes written per ray): the yardstick
  all     sr_trace_ray_maps, all nine maps (84 bytes per ray)
  lens    `end` and `sky_uv` alone
  id      `id` alone (a ray ends at its first surface)
  hits    the hit maps without `end` (the same early exit)
and a "stacked" row in tile order on tools/ray_maps_time.py's stacked
translucent layers, where every ray crosses four surfaces before it ends.
Each leg runs --warmup launches, then --calls launches back to back with a
device event between them; the legs run one after the other in each of
--rounds interleaved rounds. Per leg: the rounds' median launch times and their
median. Before the timing the traced maps must equal sr_ray_maps of the
rendered frame byte for byte.

The condition (tile order): all <= trace, with the spread of trace's own
rounds, (max - min) / median, as the margin.

  python tools/trace_maps_time.py [--steps 2000 --calls 20 --rounds 3 --out FILE]
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from ray_maps_time import stacked_scene  # noqa: E402
from trace_time import median, tile_order  # noqa: E402

DEFAULT_OUT = ROOT / "profiles" / "trace_maps" / "trace_maps_time.json"
HITS = ("hit_point", "hit_normal", "hit_view", "hit_base", "hit_step")
LEGS = {"trace": None, "all": None, "lens": ("end", "sky_uv"), "id": ("id",), "hits": HITS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--calls", type=int, default=20, help="timed launches per leg and round")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--textures", choices=["assets", "standin"], default="assets")
    ap.add_argument("--out", default=str(DEFAULT_OUT), help="the file the JSON line is also written to")
    args = ap.parse_args()
    import numpy as np
    import torch

    import srpkg

    pkg = srpkg.load_package()
    abi, sc = pkg.abi, pkg.scenes
    if not torch.cuda.is_available():
        sys.exit("trace_maps_time: no HIP device (a timing needs the GPU)")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    r = pkg.Renderer(0)
    if args.textures == "assets":
        r.set_background(pkg.assets.skybox("2k"))
        arr, _, _ = pkg.assets.texture_array()
    else:
        r.set_background(sc.skybox(2048, 1024))
        arr, _, _ = sc.default_texture_array()
    r.set_texture_array(arr)
    W, H = args.width, args.height
    n = W * H
    params = abi.default_params(max_steps=args.steps, percent_black=-1.0)
    maps_all = tuple(abi.RAY_MAPS)
    orders = {"tiles": tile_order(W, H), "rows": np.arange(n, dtype=np.int64),
              "shuffled": np.random.default_rng(0).permutation(n).astype(np.int64)}
    rows = [("default", lambda: sc.scene_default(textured=True), abi.default_camera(), order, tuple(LEGS))
            for order in orders]
    rows.append(("stacked", lambda: stacked_scene(abi, sc), sc.camera_look((0.0, 2.0, 15.0), (0.0, -2.0, -15.0)),
                 "tiles", ("trace", "all", "hits")))
    out_maps = {k: torch.empty((n, c), dtype=getattr(torch, d), device=dev) for k, (c, d) in abi.RAY_MAPS.items()}
    results, differing = [], {}
    for scene_name, make, cam, order, leg_names in rows:
        r.set_scene(make())
        O, V = pkg.camera_rays(cam, "rectilinear", W, H)
        idx = orders[order]
        o = torch.from_numpy(O.reshape(-1, 3)[idx]).to(dev)
        v = torch.from_numpy(V.reshape(-1, 3)[idx]).to(dev)

        def launch(leg):
            if leg == "trace":
                return r.trace_rays(o, v, params, rgba32=True, rgba8=True, steps=True, ids=True, stream=stream)
            return r.trace_ray_maps(o, v, params, LEGS[leg] or maps_all, out=out_maps, stream=stream)

        # the traced maps are the rendered frame's (the cameras have no -0 direction component)
        r.render(cam, params, W, H, stream=stream)
        want = r.ray_maps(stream=stream)
        got = launch("all")
        torch.cuda.synchronize()
        gather = torch.from_numpy(idx).to(dev)
        differing[f"{scene_name}/{order}"] = {
            k: int((got[k].view(torch.int32) != want[k].reshape(n, -1)[gather].view(torch.int32)).any(-1).sum().item())
            for k in maps_all}
        del want
        legs = [{"leg": name, "ms_median": [], "ms_min": []} for name in leg_names]
        for _ in range(args.rounds):
            for leg in legs:
                for _ in range(args.warmup):
                    launch(leg["leg"])
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.calls + 1)]
                ev[0].record(stream)
                for i in range(args.calls):
                    launch(leg["leg"])
                    ev[i + 1].record(stream)
                torch.cuda.synchronize()
                ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(args.calls))
                leg["ms_median"].append(round(ms[len(ms) // 2], 4))
                leg["ms_min"].append(round(ms[0], 4))
        by = {}
        for leg in legs:
            leg["ms"] = median(leg["ms_median"])
            leg["spread"] = round((max(leg["ms_median"]) - min(leg["ms_median"])) / leg["ms"], 4)
            leg["mrays_s"] = round(n / leg["ms"] / 1e3, 1)
            by[leg["leg"]] = leg
        row = {"scene": scene_name, "order": order, "legs": legs,
               "all/trace": round(by["all"]["ms"] / by["trace"]["ms"], 4), "trace_spread": by["trace"]["spread"],
               "all_within_trace": by["all"]["ms"] <= by["trace"]["ms"] * (1.0 + by["trace"]["spread"])}
        results.append(row)
    written = sum(c * 4 for c, _ in abi.RAY_MAPS.values())
    line = json.dumps({"tool": "trace_maps_time", "width": W, "height": H, "steps": args.steps, "calls": args.calls,
                       "warmup": args.warmup, "rounds": args.rounds, "textures": args.textures, "rays": n,
                       "bytes_per_ray": {"trace": 28, "all": written},
                       "rays_differing_from_sr_ray_maps": differing, "rows": results, "diag": r.diag_counters(),
                       "device": torch.cuda.get_device_name(0)})
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    r.close()
    if any(v for d in differing.values() for v in d.values()):
        sys.exit("trace_maps_time: the traced maps differ from sr_ray_maps of the rendered frame")


if __name__ == "__main__":
    main()
