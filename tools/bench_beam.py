"""Arrival maps and beamed disc shades, measured (JSON lines, HIP events on one stream, camera A, exact math), in
tools/bench_disc.py's scheme: the legs' windows alternate for `rounds` rounds of `frames` launches after a warm-up of
each, and a ratio is judged against the yardstick leg's own run-to-run spread, (max - min) / median over its rounds.
  march   (a) Scene.render_lens(hits=, arrivals=) against (b) Scene.render_lens(hits=) of the same frame -- the
          parent's kernel, byte for byte -- with the shader clock of each leg's launches (bh_set_clock_probe) beside
          its time.  Same rays, same order state; (a) stores 12 more bytes per pixel.
  shade   (a) Scene.shade(hits=, disc=, arrivals=) against (b) Scene.shade(hits=, disc=) -- the parent's kernel -- and
          (c) the plain Scene.shade of the same lens, RGBA16F, both targets, at every ss of --ss.  a - b is what the
          beam adds to b - c, the disc shade's extra over the plain shade (its divergent surface branch).
          surface_frac and disc_frac_of_surface: the part of the records that are surface records, and of those on
          the disc -- the only records (a) and (b) treat differently.  The shade kernels carry no clock probe;
          march_clock_mhz is the clock the probe saw during the case's render_lens windows.
    python tools/bench_beam.py [--cases 4096x2048:512,1920x1080:256] [--ss 1,2,4] [--frames 20] [--rounds 5] [--out FILE]"""
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
    sys.exit("bench_beam: no GPU (there is no CPU timing path)")
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


def alternate(legs, s, scene=None, acc=None):
    """per leg, its rounds' (ms, clock): one window of each leg per round, in the legs' order"""
    for _ in range(3):
        for leg in legs:
            leg(s)
    torch.cuda.synchronize()
    out = [[] for _ in legs]
    for _ in range(args.rounds):
        for o, leg in zip(out, legs):
            o.append(window(leg, s, scene, acc))
    return [([t for t, _ in o], [c for _, c in o]) for o in out]


def size_cap(case):
    size, cap = case.split(":")
    W, H = (int(v) for v in size.split("x"))
    return W, H, int(cap)


def r5(ts):
    return [round(t, 5) for t in ts]


legs = args.legs.split(",")
if "march" in legs:
    for case in args.cases.split(","):
        W, H, cap = size_cap(case)
        scene = bh.Scene(W, H, sky=sky, max_iters=cap, math=bh.BH_MATH_EXACT)
        s = torch.cuda.Stream()
        acc = torch.zeros(128, dtype=torch.int64, device="cuda")
        lens, lens_b = (torch.empty((H, W, 2), dtype=torch.float32, device="cuda") for _ in range(2))
        hits, hits_b, arrs = (torch.empty((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(3))
        (ta, ca), (tb, cb) = alternate([lambda st: scene.render_lens(lens, hits=hits, arrivals=arrs, stream=st),
                                        lambda st: scene.render_lens(lens_b, hits=hits_b, stream=st)], s, scene, acc)
        ma, mb = statistics.median(ta), statistics.median(tb)
        emit({"what": "march", "width": W, "height": H, "max_iters": cap, "camera": "A", "frames": args.frames,
              "rounds": args.rounds, "a_lens_arrivals_ms": r5(ta), "b_lens_hits_ms": r5(tb),
              "a_median_ms": round(ma, 5), "b_median_ms": round(mb, 5), "a_over_b": round(ma / mb, 4),
              "spread_a": spread(ta), "spread_b": spread(tb), "a_clock_mhz": statistics.median(ca),
              "b_clock_mhz": statistics.median(cb),
              "same_lens_and_hit_bytes": bool(torch.equal(lens, lens_b) and torch.equal(hits, hits_b))})
        scene.close()
if "shade" in legs:
    W, H, cap = size_cap(args.shade_case)
    scene = bh.Scene(W, H, sky=sky, max_iters=cap, math=bh.BH_MATH_EXACT)
    disc = bh.Disc(scene, bh.synthetic_disc())
    s = torch.cuda.Stream()
    acc = torch.zeros(128, dtype=torch.int64, device="cuda")
    for k in (int(v) for v in args.ss.split(",")):
        lens = torch.empty((k * H, k * W, 2), dtype=torch.float32, device="cuda")
        hits, arrs = (torch.empty((k * H, k * W, 3), dtype=torch.float32, device="cuda") for _ in range(2))
        clocks = [window(lambda st: scene.render_lens(lens, width=k * W, height=k * H, hits=hits, arrivals=arrs, stream=st),
                         s, scene, acc)[1] for _ in range(3)]
        surf = lens[..., 0] == bh.BH_LENS_SURFACE
        n_surf = int(surf.sum())
        rho = torch.sqrt(hits[..., 0] ** 2 + hits[..., 2] ** 2)
        rs = scene.uniforms.rs
        n_disc = int((surf & (rho > 3 * rs - 0.001) & (rho < 6 * rs + 0.001) & (hits[..., 1].abs() < 0.021)).sum())
        col, bo = (torch.empty((H, W, 4), dtype=torch.float16, device="cuda") for _ in range(2))
        kw = dict(fmt=bh.BH_OUT_RGBA16F, ss=k)
        (ta, _), (tb, _), (tc, _) = alternate(
            [lambda st: scene.shade(lens, col, bo, hits=hits, disc=disc, arrivals=arrs, spin=0.37, stream=st, **kw),
             lambda st: scene.shade(lens, col, bo, hits=hits, disc=disc, spin=0.37, stream=st, **kw),
             lambda st: scene.shade(lens, col, bo, stream=st, **kw)], s)
        ma, mb, mc = (statistics.median(t) for t in (ta, tb, tc))
        emit({"what": "shade", "width": W, "height": H, "ss": k, "format": "rgba16f", "targets": 2, "camera": "A",
              "view_max_iters": cap, "disc": "synthetic 1024x128", "frames": args.frames, "rounds": args.rounds,
              "surface_frac": round(n_surf / surf.numel(), 5), "disc_frac_of_surface": round(n_disc / max(n_surf, 1), 5),
              "a_beamed_ms": r5(ta), "b_disc_ms": r5(tb), "c_plain_ms": r5(tc),
              "a_median_ms": round(ma, 5), "b_median_ms": round(mb, 5), "c_median_ms": round(mc, 5),
              "a_over_b": round(ma / mb, 4), "a_minus_b_ms": round(ma - mb, 5), "b_minus_c_ms": round(mb - mc, 5),
              "spread_a": spread(ta), "spread_b": spread(tb), "spread_c": spread(tc),
              "march_clock_mhz": statistics.median(clocks)})
        del lens, hits, arrs, col, bo
    scene.close()
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
