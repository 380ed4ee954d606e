"""Supersampled render against its only equivalent without it, interleaved in one process:
  (a) ss       Scene.render(..., ss=k) of W x H: k x k rays per pixel, resolved in the march wave
  (b) virtual  the plain render of kW x kH (same camera, cap, format, both targets) -- the frame a caller
               would have had to render and average on the host
Same rays either way; (a) stores k^2 times fewer bytes.  HIP events on the stream around `frames` launches per
leg after a warm-up of both, legs alternating for `rounds` rounds; the shader clock of each leg's launches
(bh_set_clock_probe) is reported beside its time.  `spread_b` = (max - min) / median over the rounds of (b):
judge `a_over_b` (median a / median b) against it.
    python tools/bench_ss.py [--cases 1920x1080:2,1024x512:4] [--cap 512] [--frames 20] [--rounds 5] [--out FILE]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

import black_hole_ray_marching_amd as bh  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--cases", default="1920x1080:2,1024x512:4", help="comma list of WxH:k")
p.add_argument("--cap", type=int, default=512)
p.add_argument("--frames", type=int, default=20, help="launches per timed window")
p.add_argument("--rounds", type=int, default=5)
p.add_argument("--math", choices=["exact", "fast"], default="exact")
p.add_argument("--out", default=None, help="also append the JSON rows to this file")
args = p.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_ss: no GPU (there is no CPU timing path)")
FMTS = {"rgba16f": (bh.BH_OUT_RGBA16F, torch.float16), "bgra8": (bh.BH_OUT_BGRA8_SRGB, torch.uint8)}
math = bh.BH_MATH_EXACT if args.math == "exact" else bh.BH_MATH_FAST
sky = bh.synthetic_sky()


def window(fn, stream, acc, scene):
    """ms per launch over args.frames launches, and the shader clock during them"""
    acc.zero_()
    scene.set_clock_probe(acc, 64)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(args.frames):
        fn(stream)
    b.record(stream)
    torch.cuda.synchronize()
    scene.set_clock_probe(None)
    return a.elapsed_time(b) / args.frames, bh.clock_mhz(acc.cpu().numpy())["mhz"]


rows = []
for case in args.cases.split(","):
    size, k = case.split(":")
    W, H = (int(v) for v in size.split("x"))
    k = int(k)
    for name, (fmt, dt) in FMTS.items():
        scene = bh.Scene(W, H, sky=sky, max_iters=args.cap, math=math)
        s = torch.cuda.Stream()
        acc = torch.zeros(128, dtype=torch.int64, device="cuda")
        col, bo = (torch.empty((H, W, 4), dtype=dt, device="cuda") for _ in range(2))
        vcol, vbo = (torch.empty((k * H, k * W, 4), dtype=dt, device="cuda") for _ in range(2))

        def leg_a(st):
            scene.render(col, bo, fmt=fmt, ss=k, stream=st)

        def leg_b(st):
            scene.render(vcol, vbo, fmt=fmt, width=k * W, height=k * H, stream=st)

        for _ in range(3):  # warm-up: code objects, the order state both legs share, the learned order
            leg_a(s)
            leg_b(s)
        torch.cuda.synchronize()
        ta, tb, ca, cb = [], [], [], []
        for _ in range(args.rounds):
            t, c = window(leg_a, s, acc, scene)
            ta.append(t)
            ca.append(c)
            t, c = window(leg_b, s, acc, scene)
            tb.append(t)
            cb.append(c)
        ma, mb = statistics.median(ta), statistics.median(tb)
        row = {"width": W, "height": H, "ss": k, "max_iters": args.cap, "format": name, "math": args.math,
               "frames": args.frames, "rounds": args.rounds,
               "a_ss_ms": [round(t, 5) for t in ta], "b_virtual_ms": [round(t, 5) for t in tb],
               "a_clock_mhz": ca, "b_clock_mhz": cb,
               "a_median_ms": round(ma, 5), "b_median_ms": round(mb, 5), "a_over_b": round(ma / mb, 4),
               "spread_a": round((max(ta) - min(ta)) / ma, 4), "spread_b": round((max(tb) - min(tb)) / mb, 4),
               "samples_per_s_a": round(k * k * W * H / (ma * 1e-3) / 1e9, 3), "unit_samples": "Gsample/s"}
        print(json.dumps(row), flush=True)
        rows.append(row)
        scene.close()
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
