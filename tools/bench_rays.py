"""Ray-map renders, measured (JSON lines, HIP events on one stream, camera A, exact math).  Per case and leg pair,
the two legs alternate for `rounds` rounds of `frames` launches after a warm-up of both, the shader clock of each
leg's launches (bh_set_clock_probe) beside its time:
  rays      (a) Scene.render_rays over raymap.pinhole -- bh_render's own rays, read from the map -- against
            (b) Scene.render of the same geometry, for RGBA16F and BGRA8, both targets.  (b)'s kernels are the parent
            commit's byte for byte, so (b) in the same session is the yardstick and its own spread over the rounds
            the margin: judge a_over_b against spread_b = (max - min) / median of (b).
  equirect  (c) Scene.render_rays over raymap.equirect from camera A's position, RGBA16F: informational, no
            yardstick (other rays, another frame).
  lens      (d) Scene.render_lens(dirs=pinhole map) against Scene.render_lens.
    python tools/bench_rays.py [--cases 1920x1080:256,4096x2048:512] [--frames 20] [--rounds 5] [--out FILE]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

import black_hole_ray_marching_amd as bh  # noqa: E402
from black_hole_ray_marching_amd import raymap  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--cases", default="1920x1080:256,4096x2048:512", help="comma list of WxH:cap")
p.add_argument("--frames", type=int, default=20, help="launches per timed window")
p.add_argument("--rounds", type=int, default=5)
p.add_argument("--warm-ms", type=float, default=400.0, help="warm-up of both legs before a pair's first window")
p.add_argument("--out", default=None, help="also append the JSON rows to this file")
args = p.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_rays: no GPU (there is no CPU timing path)")
FMTS = {"rgba16f": (bh.BH_OUT_RGBA16F, torch.float16), "bgra8": (bh.BH_OUT_BGRA8_SRGB, torch.uint8)}
sky = bh.synthetic_sky()
rows = []


def window(fn, stream, scene, acc):
    """(ms per launch over args.frames launches, the shader clock during them)"""
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


def spread(ts):
    return round((max(ts) - min(ts)) / statistics.median(ts), 4)


def pair(what, scene, s, acc, leg_a, leg_b, **tags):
    """legs alternating; leg_b None: one leg alone"""
    legs = [leg for leg in (leg_a, leg_b) if leg]
    # warm-up: code objects, each leg's order state, the learned orders -- and the clock, which takes some hundred
    # milliseconds of load to settle after an idle stretch (the host work between two cases is one)
    t_end = time.perf_counter() + args.warm_ms * 1e-3
    n = 0
    while n < 3 or time.perf_counter() < t_end:
        for leg in legs:
            for _ in range(args.frames):
                leg(s)
        torch.cuda.synchronize()
        n += 1
    t, c = [[] for _ in legs], [[] for _ in legs]
    for _ in range(args.rounds):
        for i, leg in enumerate(legs):
            ms, mhz = window(leg, s, scene, acc)
            t[i].append(ms)
            c[i].append(mhz)
    row = {"what": what, **tags, "camera": "A", "math": "exact", "frames": args.frames, "rounds": args.rounds,
           "a_ms": [round(v, 5) for v in t[0]], "a_clock_mhz": c[0], "a_median_ms": round(statistics.median(t[0]), 5),
           "spread_a": spread(t[0])}
    if leg_b:
        row.update({"b_ms": [round(v, 5) for v in t[1]], "b_clock_mhz": c[1], "b_median_ms": round(statistics.median(t[1]), 5),
                    "spread_b": spread(t[1]), "a_over_b": round(statistics.median(t[0]) / statistics.median(t[1]), 4)})
    print(json.dumps(row), flush=True)
    rows.append(row)


for case in args.cases.split(","):
    size, cap = case.split(":")
    W, H = (int(v) for v in size.split("x"))
    cap = int(cap)
    scene = bh.Scene(W, H, sky=sky, max_iters=cap, math=bh.BH_MATH_EXACT)
    s = torch.cuda.Stream()
    acc = torch.zeros(128, dtype=torch.int64, device="cuda")
    tags = dict(width=W, height=H, max_iters=cap)
    pin = torch.from_numpy(raymap.pinhole(scene.camera_uniform, W, H)).cuda()
    for name, (fmt, dt) in FMTS.items():
        col, bo = (torch.empty((H, W, 4), dtype=dt, device="cuda") for _ in range(2))
        pair("rays", scene, s, acc, lambda st: scene.render_rays(pin, col, bo, fmt=fmt, stream=st),
             lambda st: scene.render(col, bo, fmt=fmt, stream=st), format=name, targets=2, map="pinhole", **tags)
    eq = torch.from_numpy(raymap.equirect(W, H, scene.camera.dir, scene.camera.up)).cuda()
    fmt, dt = FMTS["rgba16f"]
    col, bo = (torch.empty((H, W, 4), dtype=dt, device="cuda") for _ in range(2))
    pair("equirect", scene, s, acc, lambda st: scene.render_rays(eq, col, bo, fmt=fmt, stream=st), None,
         format="rgba16f", targets=2, map="equirect", **tags)
    lens = torch.empty((H, W, 2), dtype=torch.float32, device="cuda")
    pair("lens", scene, s, acc, lambda st: scene.render_lens(lens, dirs=pin, stream=st),
         lambda st: scene.render_lens(lens, stream=st), map="pinhole", **tags)
    del pin, eq, col, bo, lens
    scene.close()
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
