"""Adaptive supersampling against its two neighbours, interleaved in one process on one build:
  plain     Scene.render of W x H: one ray per pixel (what every pixel of the adaptive frame starts as)
  ss        Scene.render(..., ss=k): k x k rays through every pixel
  adaptive  Scene.render(..., ss=k, adaptive=T) for each T: the plain frame, a detect pass, and k x k rays
            through the pixels of the 8x8 tiles that show an edge above T
  fixed     the adaptive render at T = 3e38: nothing refined -- its time minus the plain render's is the fixed
            overhead (two memsets, the detect kernel, a march launch over an empty list)
tools/bench_ss.py's method: HIP events on the stream around `frames` launches per leg after a warm-up of every
leg, legs alternating for `rounds` rounds, medians; the shader clock of each leg's march launches
(bh_set_clock_probe) beside its time.  `share` = refined tiles / tiles (read back after the timing), `model_ms`
= plain + share * ss, the simple ray-count model; `adaptive_over_ss` and `adaptive_over_model` are median
ratios.  Exact math, both targets.
    python tools/bench_ss_adaptive.py [--cases 1920x1080:2,1920x1080:4,1024x512:4] [--cameras A,B]
        [--thresholds 0.05,0.1,0.25] [--cap 512] [--frames 20] [--rounds 5] [--schedule-flag latency] [--out FILE]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

import black_hole_ray_marching_amd as bh  # noqa: E402
from bench import CAMERAS  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--cases", default="1920x1080:2,1920x1080:4,1024x512:4", help="comma list of WxH:k")
p.add_argument("--cameras", default="A,B")
p.add_argument("--thresholds", default="0.05,0.1,0.25")
p.add_argument("--formats", default="rgba16f,bgra8")
p.add_argument("--cap", type=int, default=512)
p.add_argument("--frames", type=int, default=20, help="launches per timed window")
p.add_argument("--rounds", type=int, default=5)
p.add_argument("--schedule-flag", choices=["none", "issue", "latency"], default="none",
               help="force one build of the exact kernels in every leg (BH_SCHED_FLAG_ISSUE_ORDER / _LATENCY)")
p.add_argument("--out", default=None, help="also append the JSON rows to this file")
args = p.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_ss_adaptive: no GPU (there is no CPU timing path)")
FMTS = {"rgba16f": (bh.BH_OUT_RGBA16F, torch.float16), "bgra8": (bh.BH_OUT_BGRA8_SRGB, torch.uint8)}
NOTHING = 3e38
sched = bh.BH_SCHED_TILE | {"none": 0, "issue": bh.BH_SCHED_FLAG_ISSUE_ORDER, "latency": bh.BH_SCHED_FLAG_LATENCY}[args.schedule_flag]
thresholds = [float(t) for t in args.thresholds.split(",")]
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
    n_tiles = ((W + 7) // 8) * ((H + 7) // 8)
    for cam in args.cameras.split(","):
        for name in args.formats.split(","):
            fmt, dt = FMTS[name]
            scene = bh.Scene(W, H, sky=sky, max_iters=args.cap, math=bh.BH_MATH_EXACT)
            scene.update(bh.Camera.look_at(*CAMERAS[cam], W, H))
            s = torch.cuda.Stream()
            acc = torch.zeros(128, dtype=torch.int64, device="cuda")
            col, bo = (torch.empty((H, W, 4), dtype=dt, device="cuda") for _ in range(2))
            count = torch.zeros(1, dtype=torch.int32, device="cuda")
            legs = {"plain": lambda st: scene.render(col, bo, fmt=fmt, schedule=sched, stream=st),
                    "ss": lambda st: scene.render(col, bo, fmt=fmt, ss=k, schedule=sched, stream=st)}
            for t in thresholds + [NOTHING]:
                legs[f"adaptive_{t:g}"] = (lambda st, t=t: scene.render(col, bo, fmt=fmt, ss=k, adaptive=t, schedule=sched,
                                                                       refined_tiles=count, stream=st))
            for _ in range(3):  # warm-up: code objects, both geometries' order states, the work list, the learned orders
                for fn in legs.values():
                    fn(s)
            torch.cuda.synchronize()
            ms = {n: [] for n in legs}
            clk = {n: [] for n in legs}
            for _ in range(args.rounds):
                for n, fn in legs.items():
                    t_ms, c = window(fn, s, acc, scene)
                    ms[n].append(t_ms)
                    clk[n].append(c)
            share = {}
            for t in thresholds + [NOTHING]:
                legs[f"adaptive_{t:g}"](s)
                torch.cuda.synchronize()
                share[t] = int(count.item()) / n_tiles
            med = {n: statistics.median(v) for n, v in ms.items()}
            base = {"width": W, "height": H, "ss": k, "camera": cam, "max_iters": args.cap, "format": name, "math": "exact",
                    "schedule_flag": args.schedule_flag, "frames": args.frames, "rounds": args.rounds, "tiles": n_tiles,
                    "plain_ms": [round(v, 5) for v in ms["plain"]], "ss_ms": [round(v, 5) for v in ms["ss"]],
                    "plain_median_ms": round(med["plain"], 5), "ss_median_ms": round(med["ss"], 5),
                    "plain_clock_mhz": clk["plain"], "ss_clock_mhz": clk["ss"],
                    "spread_plain": round((max(ms["plain"]) - min(ms["plain"])) / med["plain"], 4),
                    "spread_ss": round((max(ms["ss"]) - min(ms["ss"])) / med["ss"], 4),
                    "fixed_overhead_ms": round(med[f"adaptive_{NOTHING:g}"] - med["plain"], 5),
                    "nothing_refined_ms": [round(v, 5) for v in ms[f"adaptive_{NOTHING:g}"]]}
            assert share[NOTHING] == 0.0
            for t in thresholds:
                n = f"adaptive_{t:g}"
                model = med["plain"] + share[t] * med["ss"]
                row = dict(base, threshold=t, share=round(share[t], 4), adaptive_ms=[round(v, 5) for v in ms[n]],
                           adaptive_median_ms=round(med[n], 5), adaptive_clock_mhz=clk[n],
                           spread_adaptive=round((max(ms[n]) - min(ms[n])) / med[n], 4), model_ms=round(model, 5),
                           adaptive_over_ss=round(med[n] / med["ss"], 4), adaptive_over_model=round(med[n] / model, 4),
                           rays_per_pixel=round(1 + share[t] * k * k, 3))
                print(json.dumps(row), flush=True)
                rows.append(row)
            scene.close()
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
