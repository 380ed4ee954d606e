"""Hit maps and disc shades, measured (JSON lines, HIP events on one stream, camera A, exact math):
  march   (a) Scene.render_lens(hits=) against (b) Scene.render_lens of the same frame, windows alternating for
          `rounds` rounds of `frames` launches after a warm-up of both, the shader clock of each leg's launches
          (bh_set_clock_probe) beside its time.  Same rays, same order state; (a) stores 12 more bytes per pixel.
          Judge a_over_b against spread_b = (max - min) / median over the rounds of (b).
  shade   (a) Scene.shade(hits=, disc=) against (b) Scene.shade of the same lens, RGBA16F, both targets, at every ss
          of --ss (the lens and the hit map are the virtual frame's), windows alternating.  surface_frac and
          disc_frac: the part of the records that are surface records, and of those on the disc (the only records
          the two kernels treat differently).  The shade kernels carry no clock probe; march_clock_mhz is the clock
          the probe saw during the case's render_lens windows.
The share of the f64 angle in (a): run the shade leg again with a variant build whose angle is the fp32 library call,
    python -m black_hole_ray_marching_amd.build --out DIR --extra bh_disc.hip="-DBH_DISC_ANGLE_F32"
    BH_LIB=DIR/libbh_render.so python tools/bench_disc.py --legs shade --tag f32angle
and compare a_median_ms of the two runs (the variant does not render the rule's bits).
    python tools/bench_disc.py [--cases 4096x2048:512,1920x1080:256] [--ss 1,2,4] [--frames 20] [--rounds 5] [--out FILE]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

import black_hole_ray_marching_amd as bh  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--cases", default="4096x2048:512,1920x1080:256", help="comma list of WxH:cap")
p.add_argument("--ss", default="1,2,4", help="comma list of ss for the shade leg")
p.add_argument("--legs", default="march,shade")
p.add_argument("--shade-case", default="1920x1080:256", help="the output frame of the shade leg")
p.add_argument("--frames", type=int, default=20, help="launches per timed window")
p.add_argument("--rounds", type=int, default=5)
p.add_argument("--tag", default="", help="a word copied into every row (which build ran)")
p.add_argument("--out", default=None, help="also append the JSON rows to this file")
args = p.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_disc: no GPU (there is no CPU timing path)")
sky = bh.synthetic_sky()
rows = []


def window(fn, stream, scene=None, acc=None):
    """ms per launch over args.frames launches (and, with a scene, the shader clock during them)"""
    if scene is not None:
        acc.zero_()
        scene.set_clock_probe(acc, 64)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(args.frames):
        fn(stream)
    b.record(stream)
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / args.frames
    if scene is None:
        return ms, None
    scene.set_clock_probe(None)
    return ms, bh.clock_mhz(acc.cpu().numpy())["mhz"]


def emit(row):
    if args.tag:
        row["tag"] = args.tag
    print(json.dumps(row), flush=True)
    rows.append(row)


def spread(ts):
    return round((max(ts) - min(ts)) / statistics.median(ts), 4)


def alternate(leg_a, leg_b, s, scene=None, acc=None):
    for _ in range(3):
        leg_a(s)
        leg_b(s)
    torch.cuda.synchronize()
    ta, tb, ca, cb = [], [], [], []
    for _ in range(args.rounds):
        t, c = window(leg_a, s, scene, acc)
        ta.append(t), ca.append(c)
        t, c = window(leg_b, s, scene, acc)
        tb.append(t), cb.append(c)
    return ta, tb, ca, cb


def size_cap(case):
    size, cap = case.split(":")
    W, H = (int(v) for v in size.split("x"))
    return W, H, int(cap)


legs = args.legs.split(",")
if "march" in legs:
    for case in args.cases.split(","):
        W, H, cap = size_cap(case)
        scene = bh.Scene(W, H, sky=sky, max_iters=cap, math=bh.BH_MATH_EXACT)
        s = torch.cuda.Stream()
        acc = torch.zeros(128, dtype=torch.int64, device="cuda")
        lens = torch.empty((H, W, 2), dtype=torch.float32, device="cuda")
        lens_b = torch.empty_like(lens)
        hits = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        ta, tb, ca, cb = alternate(lambda st: scene.render_lens(lens, hits=hits, stream=st),
                                   lambda st: scene.render_lens(lens_b, stream=st), s, scene, acc)
        ma, mb = statistics.median(ta), statistics.median(tb)
        emit({"what": "march", "width": W, "height": H, "max_iters": cap, "camera": "A", "frames": args.frames,
              "rounds": args.rounds, "a_lens_hits_ms": [round(t, 5) for t in ta], "b_lens_ms": [round(t, 5) for t in tb],
              "a_median_ms": round(ma, 5), "b_median_ms": round(mb, 5), "a_over_b": round(ma / mb, 4),
              "spread_a": spread(ta), "spread_b": spread(tb), "a_clock_mhz": statistics.median(ca),
              "b_clock_mhz": statistics.median(cb), "same_lens_bytes": bool(torch.equal(lens, lens_b))})
        scene.close()
if "shade" in legs:
    W, H, cap = size_cap(args.shade_case)
    scene = bh.Scene(W, H, sky=sky, max_iters=cap, math=bh.BH_MATH_EXACT)
    disc = bh.Disc(scene, bh.synthetic_disc())
    s = torch.cuda.Stream()
    acc = torch.zeros(128, dtype=torch.int64, device="cuda")
    for k in (int(v) for v in args.ss.split(",")):
        lens = torch.empty((k * H, k * W, 2), dtype=torch.float32, device="cuda")
        hits = torch.empty((k * H, k * W, 3), dtype=torch.float32, device="cuda")
        clocks = [window(lambda st: scene.render_lens(lens, width=k * W, height=k * H, hits=hits, stream=st), s, scene, acc)[1]
                  for _ in range(3)]
        surf = lens[..., 0] == bh.BH_LENS_SURFACE
        n_surf = int(surf.sum())
        rho = torch.sqrt(hits[..., 0] ** 2 + hits[..., 2] ** 2)
        rs = scene.uniforms.rs
        n_disc = int((surf & (rho > 3 * rs - 0.001) & (rho < 6 * rs + 0.001) & (hits[..., 1].abs() < 0.021)).sum())
        col, bo = (torch.empty((H, W, 4), dtype=torch.float16, device="cuda") for _ in range(2))
        ta, tb, _, _ = alternate(
            lambda st: scene.shade(lens, col, bo, fmt=bh.BH_OUT_RGBA16F, ss=k, hits=hits, disc=disc, spin=0.37, stream=st),
            lambda st: scene.shade(lens, col, bo, fmt=bh.BH_OUT_RGBA16F, ss=k, stream=st), s)
        ma, mb = statistics.median(ta), statistics.median(tb)
        emit({"what": "shade", "width": W, "height": H, "ss": k, "format": "rgba16f", "targets": 2, "camera": "A",
              "view_max_iters": cap, "disc": "synthetic 1024x128", "frames": args.frames, "rounds": args.rounds,
              "surface_frac": round(n_surf / surf.numel(), 5), "disc_frac_of_surface": round(n_disc / max(n_surf, 1), 5),
              "a_disc_ms": [round(t, 5) for t in ta], "b_plain_ms": [round(t, 5) for t in tb],
              "a_median_ms": round(ma, 5), "b_median_ms": round(mb, 5), "a_over_b": round(ma / mb, 4),
              "a_minus_b_ms": round(ma - mb, 5), "spread_a": spread(ta), "spread_b": spread(tb),
              "march_clock_mhz": statistics.median(clocks)})
        del lens, hits, col, bo
    scene.close()
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
