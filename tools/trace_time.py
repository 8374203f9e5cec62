#!/usr/bin/env python3
"""Times sr_trace_rays on the headline frame's own camera rays
(sr_camera_rays) in three orders, beside sr_render of the same frame in the
same process, and prints one JSON line.

Legs (one context, one stream; every leg traces or renders the same 1920 x
1080 rays of the app's camera on the default scene):
  render     sr_render: the frame kernels, the yardstick (Mpixels/s)
  tiles      the rays in the frame kernels' order: 16x16 workgroup tiles of
             four 8x8 wave tiles, so each 64-ray wave is an 8x8 pixel tile
  rows       row-major: a wave is 64 pixels of one row
  shuffled   a seeded random permutation: a wave's rays are unrelated
Each leg runs --warmup launches, then --frames launches back to back with a
device event between them; the legs run one after the other in each of
--rounds interleaved rounds. Per leg: the rounds' median launch times, their
median, and Mrays/s (Mpixels/s) from it. The traced legs ask for RGBA8 alone,
what sr_render writes; their bytes are checked against the rendered frame
once, before the timing.

  python tools/trace_time.py [--steps 2000 --frames 20 --rounds 3 --out FILE]
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


def tile_order(w, h):
    """The pixel indices (row-major) of a w x h frame in the frame kernels'
    order: 16x16 tiles row-major, in each the four 8x8 wave tiles, in each
    8 rows of 8 (geodesic.hip pixel_of); pixels off the frame dropped."""
    import numpy as np

    gx, gy = (w + 15) // 16, (h + 15) // 16
    t = np.arange(256)
    lane, wave = t & 63, t >> 6
    px = (np.arange(gx)[None, :, None] * 16 + ((wave & 1) * 8 + (lane & 7))[None, None, :])
    py = (np.arange(gy)[:, None, None] * 16 + ((wave >> 1) * 8 + (lane >> 3))[None, None, :])
    px, py = np.broadcast_to(px, (gy, gx, 256)).reshape(-1), np.broadcast_to(py, (gy, gx, 256)).reshape(-1)
    keep = (px < w) & (py < h)
    return (py[keep] * w + px[keep]).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--textures", choices=["assets", "standin"], default="assets")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    import numpy as np
    import torch

    import srpkg

    pkg = srpkg.load_package()
    abi, sc = pkg.abi, pkg.scenes
    if not torch.cuda.is_available():
        sys.exit("trace_time: no HIP device (a timing needs the GPU)")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    r = pkg.Renderer(0)
    r.set_scene(sc.scene_default(textured=True))
    if args.textures == "assets":
        r.set_background(pkg.assets.skybox("2k"))
        arr, _, _ = pkg.assets.texture_array()
    else:
        r.set_background(sc.skybox(2048, 1024))
        arr, _, _ = sc.default_texture_array()
    r.set_texture_array(arr)
    W, H = args.width, args.height
    params = abi.default_params(max_steps=args.steps, percent_black=-1.0)
    cam = abi.default_camera()
    O, V = pkg.camera_rays(cam, "rectilinear", W, H)
    O, V = O.reshape(-1, 3), V.reshape(-1, 3)
    n = W * H
    orders = {"tiles": tile_order(W, H), "rows": np.arange(n, dtype=np.int64),
              "shuffled": np.random.default_rng(0).permutation(n).astype(np.int64)}
    assert all(len(o) == n for o in orders.values())
    frame = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
    legs = [{"leg": "render", "ms_median": [], "ms_min": [], "ms_mean": []}]
    for name, idx in orders.items():
        legs.append({"leg": name, "o": torch.from_numpy(O[idx]).to(dev), "v": torch.from_numpy(V[idx]).to(dev),
                     "idx": torch.from_numpy(idx).to(dev), "ms_median": [], "ms_min": [], "ms_mean": []})

    def launch(leg):
        if leg["leg"] == "render":
            r.render(cam, params, W, H, out=frame, stream=stream)
            return None
        return r.trace_rays(leg["o"], leg["v"], params, stream=stream)["rgba8"]

    # the traced bytes are the frame's (the app's camera has no -0 direction component)
    launch(legs[0])
    torch.cuda.synchronize()
    flat = frame.reshape(-1, 4)
    differing = {}
    for leg in legs[1:]:
        with torch.cuda.stream(stream):
            got = launch(leg)
        torch.cuda.synchronize()
        differing[leg["leg"]] = int((got != flat[leg["idx"]]).any(-1).sum().item())
    for _ in range(args.rounds):
        for leg in legs:
            with torch.cuda.stream(stream):
                for _ in range(args.warmup):
                    launch(leg)
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.frames + 1)]
                ev[0].record(stream)
                for i in range(args.frames):
                    launch(leg)
                    ev[i + 1].record(stream)
            torch.cuda.synchronize()
            ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(args.frames))
            leg["ms_median"].append(round(ms[len(ms) // 2], 4))
            leg["ms_min"].append(round(ms[0], 4))
            leg["ms_mean"].append(round(ev[0].elapsed_time(ev[-1]) / args.frames, 4))
    for leg in legs:
        leg["ms"] = median(leg["ms_median"])
        leg["mrays_s"] = round(n / leg["ms"] / 1e3, 1)
        for k in ("o", "v", "idx"):
            leg.pop(k, None)
    base = legs[0]["ms"]
    for leg in legs[1:]:
        leg["times_render"] = round(leg["ms"] / base, 3)
    line = json.dumps({
        "tool": "trace_time", "width": W, "height": H, "steps": args.steps, "frames": args.frames,
        "warmup": args.warmup, "rounds": args.rounds, "textures": args.textures, "rays": n,
        "pixels_differing_from_render": differing, "legs": legs, "diag": r.diag_counters(),
        "device": torch.cuda.get_device_name(0),
    })
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    r.close()


if __name__ == "__main__":
    main()
