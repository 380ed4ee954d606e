"""Shutter render against what its march alone costs today, interleaved in one process:
  (a) shutter  Scene.render_shutter of W x H with n sub-frame cameras: n marches per tile in one workgroup,
               resolved there, one frame stored
  (b) frames   bh_render_frames of the same n cameras in one launch into n frames of the same format (both
               targets): the same rays with no averaging at all, n times the bytes stored
The cameras: camera A orbiting the hole by 0.2 degrees per frame, the step split into n sub-steps.  HIP events on
the stream around `frames` launches per leg after a warm-up of both, legs alternating for `rounds` rounds; the
shader clock of each window's launches (bh_set_clock_probe) is reported beside its time.  Round 1 is reported
and kept out of the medians and spreads.  `spread_b` = (max - min) / median over the later rounds of (b): judge
`a_over_b` (median a / median b) against it.
    python tools/bench_shutter.py [--cases 1920x1080:4,1920x1080:8] [--cap 512] [--frames 20] [--rounds 5] [--out FILE]"""
import argparse
import json
import math
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

import black_hole_ray_marching_amd as bh  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--cases", default="1920x1080:4,1920x1080:8,1920x1080:16,4096x2048:4,4096x2048:8,4096x2048:16",
               help="comma list of WxH:n")
p.add_argument("--formats", default="rgba16f,bgra8")
p.add_argument("--cap", type=int, default=512)
p.add_argument("--frames", type=int, default=20, help="launches per timed window")
p.add_argument("--rounds", type=int, default=5)
p.add_argument("--degrees", type=float, default=0.2, help="orbit angle per frame")
p.add_argument("--out", default=None, help="also append the JSON rows to this file")
args = p.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_shutter: no GPU (there is no CPU timing path)")
FMTS = {"rgba16f": (bh.BH_OUT_RGBA16F, torch.float16), "bgra8": (bh.BH_OUT_BGRA8_SRGB, torch.uint8)}
sky = bh.synthetic_sky()


def orbit_cameras(W, H, n):
    """n sub-frame cameras: camera A (0, 0, -20) turned about the y axis by degrees * t / n, looking at the hole"""
    out = []
    for t in range(n):
        a = math.radians(args.degrees * t / n)
        cu = bh.CameraUniform()
        cu.update(bh.Camera.look_at((-20.0 * math.sin(a), 0.0, -20.0 * math.cos(a)), (0.0, 0.0, 0.0), W, H))
        out.append(cu)
    return out


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
    size, n = case.split(":")
    W, H = (int(v) for v in size.split("x"))
    n = int(n)
    for name in args.formats.split(","):
        fmt, dt = FMTS[name]
        scene = bh.Scene(W, H, sky=sky, max_iters=args.cap, math=bh.BH_MATH_EXACT)
        s = torch.cuda.Stream()
        acc = torch.zeros(128, dtype=torch.int64, device="cuda")
        cams = orbit_cameras(W, H, n)
        col, bo = (torch.empty((H, W, 4), dtype=dt, device="cuda") for _ in range(2))
        fcol = [torch.empty((H, W, 4), dtype=dt, device="cuda") for _ in range(n)]
        fbo = [torch.empty((H, W, 4), dtype=dt, device="cuda") for _ in range(n)]
        batch = scene.prepare_frames(fcol, fbo, fmt=fmt)

        def leg_a(st):
            scene.render_shutter(col, bo, cameras=cams, fmt=fmt, stream=st)

        def leg_b(st):
            batch.render(cameras=cams, stream=st)

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
        ka, kb = (ta[1:], tb[1:]) if args.rounds > 1 else (ta, tb)  # round 1 stays out of the statistics
        ma, mb = statistics.median(ka), statistics.median(kb)
        row = {"width": W, "height": H, "n_sub": n, "max_iters": args.cap, "format": name, "math": "exact",
               "frames": args.frames, "rounds": args.rounds,
               "a_shutter_ms": [round(t, 5) for t in ta], "b_frames_ms": [round(t, 5) for t in tb],
               "a_clock_mhz": ca, "b_clock_mhz": cb,
               "a_median_ms": round(ma, 5), "b_median_ms": round(mb, 5), "a_over_b": round(ma / mb, 4),
               "spread_a": round((max(ka) - min(ka)) / ma, 4), "spread_b": round((max(kb) - min(kb)) / mb, 4),
               "rays_per_s_a": round(n * W * H / (ma * 1e-3) / 1e9, 3), "unit_rays": "Gray/s"}
        print(json.dumps(row), flush=True)
        rows.append(row)
        scene.close()
        del fcol, fbo, batch
        torch.cuda.empty_cache()
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
