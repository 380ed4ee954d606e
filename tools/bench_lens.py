"""Lens maps, measured (JSON lines, HIP events on one stream, camera A, exact math):
  march   (a) Scene.render_lens against (b) Scene.render (RGBA16F, both targets) of the same frame, legs
          alternating for `rounds` rounds of `frames` launches after a warm-up of both; the shader clock of each
          leg's launches (bh_set_clock_probe) beside its time.  Same rays, same order state; (a) stores 8 bytes per
          pixel where (b) stores 16.  Judge a_over_b against spread_b = (max - min) / median over the rounds of (b).
  shade   Scene.shade of a lens for the three formats at ss 1, 2 and 4 (the lens is the virtual frame's:
          ss*W x ss*H records), both targets, against a device-to-device copy as the bandwidth yardstick: the
          shade's compulsory traffic is lens bytes in + two targets out (the sky gathers hit the L2); the copy
          moves as many bytes (half of them read, half written).  frac_of_copy = the shade's compulsory bytes per
          second over the copy's.  The shade kernel carries no clock probe; `march_clock_mhz` is the clock the
          probe saw during this case's render_lens windows.
  --mip   instead of the above: (a) Scene.shade(mip=True) against (b) Scene.shade of the same lens and sky, RGBA16F,
          both targets, at every ss of --ss that the filter has, windows alternating; once per sky of --mip-skies
          (4096x2048: mostly the plain path, so a - b is the cost of the footprint; 16384x8192: minified).  Beside
          them the chain build (bh_sky_create_mips less bh_sky_create of the same texels, wall clock, upload included
          in both) and the clock the probe saw during the case's render_lens windows.
    python tools/bench_lens.py [--cases 4096x2048:512,1920x1080:256] [--frames 20] [--rounds 5] [--out FILE]
    python tools/bench_lens.py --mip --cases 1920x1080:256,4096x2048:512 --ss 1,2"""
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
p.add_argument("--ss", default="1,2,4", help="comma list of ss for the shade legs")
p.add_argument("--frames", type=int, default=20, help="launches per timed window")
p.add_argument("--rounds", type=int, default=5)
p.add_argument("--out", default=None, help="also append the JSON rows to this file")
p.add_argument("--mip", action="store_true", help="measure the filtered shade against the plain one")
p.add_argument("--mip-skies", default="4096x2048,16384x8192", help="with --mip: comma list of synthetic sky sizes")
args = p.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_lens: no GPU (there is no CPU timing path)")
FMTS = {"rgba32f": (bh.BH_OUT_RGBA32F, torch.float32), "rgba16f": (bh.BH_OUT_RGBA16F, torch.float16),
        "bgra8": (bh.BH_OUT_BGRA8_SRGB, torch.uint8)}
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
    print(json.dumps(row), flush=True)
    rows.append(row)


def spread(ts):
    return round((max(ts) - min(ts)) / statistics.median(ts), 4)


def write_out():
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def bench_mip():
    import time
    skies = {}
    for name in args.mip_skies.split(","):
        skies[name] = bh.synthetic_sky(*(int(v) for v in name.split("x")), seed=11)
    for case in args.cases.split(","):
        size, cap = case.split(":")
        W, H = (int(v) for v in size.split("x"))
        scene = bh.Scene(W, H, sky=sky, max_iters=int(cap), math=bh.BH_MATH_EXACT)
        s = torch.cuda.Stream()
        acc = torch.zeros(128, dtype=torch.int64, device="cuda")
        for name, texels in skies.items():
            walls = {}
            for mips in (False, True, False, True):  # the second pair is the one reported (allocator warm)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                k_sky = bh.Sky(scene, texels, mips=mips)
                walls[mips] = (time.perf_counter() - t0) * 1e3
                if mips:
                    mip_sky = k_sky
                else:
                    k_sky.close()
            emit({"what": "chain", "sky": name, "levels": mip_sky.levels, "create_ms": round(walls[False], 3),
                  "create_mips_ms": round(walls[True], 3), "chain_ms": round(walls[True] - walls[False], 3)})
            for k in (int(v) for v in args.ss.split(",") if int(v) in (1, 2, 4)):
                vlens = torch.empty((k * H, k * W, 2), dtype=torch.float32, device="cuda")
                clocks = []
                for _ in range(3):
                    clocks.append(window(lambda st: scene.render_lens(vlens, width=k * W, height=k * H, stream=st), s, scene, acc)[1])
                col, bo = (torch.empty((H, W, 4), dtype=torch.float16, device="cuda") for _ in range(2))

                def leg_a(st):
                    scene.shade(vlens, col, bo, fmt=bh.BH_OUT_RGBA16F, sky=mip_sky, ss=k, stream=st, mip=True)

                def leg_b(st):
                    scene.shade(vlens, col, bo, fmt=bh.BH_OUT_RGBA16F, sky=mip_sky, ss=k, stream=st)

                for _ in range(3):
                    leg_a(s)
                    leg_b(s)
                torch.cuda.synchronize()
                ta, tb = [], []
                for _ in range(args.rounds):
                    ta.append(window(leg_a, s)[0])
                    tb.append(window(leg_b, s)[0])
                ma, mb = statistics.median(ta), statistics.median(tb)
                emit({"what": "shade_mip", "width": W, "height": H, "ss": k, "format": "rgba16f", "targets": 2, "sky": name,
                      "camera": "A", "view_max_iters": int(cap), "frames": args.frames, "rounds": args.rounds,
                      "a_mip_ms": [round(t, 5) for t in ta], "b_plain_ms": [round(t, 5) for t in tb],
                      "a_median_ms": round(ma, 5), "b_median_ms": round(mb, 5), "a_over_b": round(ma / mb, 4),
                      "spread_a": spread(ta), "spread_b": spread(tb), "march_clock_mhz": statistics.median(clocks)})
                del vlens, col, bo
            mip_sky.close()
        scene.close()


if args.mip:
    bench_mip()
    write_out()
    sys.exit(0)
for case in args.cases.split(","):
    size, cap = case.split(":")
    W, H = (int(v) for v in size.split("x"))
    cap = int(cap)
    scene = bh.Scene(W, H, sky=sky, max_iters=cap, math=bh.BH_MATH_EXACT)
    s = torch.cuda.Stream()
    acc = torch.zeros(128, dtype=torch.int64, device="cuda")

    # ---- the lens march against the plain render --------------------------------------------------------
    lens = torch.empty((H, W, 2), dtype=torch.float32, device="cuda")
    col, bo = (torch.empty((H, W, 4), dtype=torch.float16, device="cuda") for _ in range(2))

    def leg_a(st):
        scene.render_lens(lens, stream=st)

    def leg_b(st):
        scene.render(col, bo, fmt=bh.BH_OUT_RGBA16F, stream=st)

    with torch.cuda.stream(s):
        for _ in range(3):  # warm-up: code objects, the order state both legs share, the learned order
            leg_a(s)
            leg_b(s)
    torch.cuda.synchronize()
    ta, tb, ca, cb = [], [], [], []
    for _ in range(args.rounds):
        t, c = window(leg_a, s, scene, acc)
        ta.append(t)
        ca.append(c)
        t, c = window(leg_b, s, scene, acc)
        tb.append(t)
        cb.append(c)
    ma, mb = statistics.median(ta), statistics.median(tb)
    emit({"what": "march", "width": W, "height": H, "max_iters": cap, "camera": "A", "math": "exact",
          "frames": args.frames, "rounds": args.rounds,
          "a_render_lens_ms": [round(t, 5) for t in ta], "b_render_rgba16f_ms": [round(t, 5) for t in tb],
          "a_clock_mhz": ca, "b_clock_mhz": cb, "a_median_ms": round(ma, 5), "b_median_ms": round(mb, 5),
          "a_over_b": round(ma / mb, 4), "spread_a": spread(ta), "spread_b": spread(tb)})
    march_clock = statistics.median(ca)
    del lens, col, bo

    # ---- the shade against a copy of its compulsory bytes -------------------------------------------------
    for k in (int(v) for v in args.ss.split(",")):
        vlens = torch.empty((k * H, k * W, 2), dtype=torch.float32, device="cuda")
        scene.render_lens(vlens, width=k * W, height=k * H, stream=s)
        torch.cuda.synchronize()
        for name, (fmt, dt) in FMTS.items():
            col, bo = (torch.empty((H, W, 4), dtype=dt, device="cuda") for _ in range(2))
            traffic = vlens.numel() * 4 + 2 * col.numel() * col.element_size()
            src = torch.empty(traffic // 2, dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)

            def leg_shade(st):
                scene.shade(vlens, col, bo, fmt=fmt, ss=k, stream=st)

            def leg_copy(st):
                with torch.cuda.stream(st):
                    dst.copy_(src, non_blocking=True)

            for _ in range(3):
                leg_shade(s)
                leg_copy(s)
            torch.cuda.synchronize()
            ts, tc = [], []
            for _ in range(args.rounds):
                ts.append(window(leg_shade, s)[0])
                tc.append(window(leg_copy, s)[0])
            ms, mc = statistics.median(ts), statistics.median(tc)
            emit({"what": "shade", "width": W, "height": H, "ss": k, "format": name, "targets": 2,
                  "sky": f"{sky.shape[1]}x{sky.shape[0]}", "view_max_iters": cap, "frames": args.frames,
                  "rounds": args.rounds, "compulsory_bytes": traffic,
                  "shade_ms": [round(t, 5) for t in ts], "copy_ms": [round(t, 5) for t in tc],
                  "shade_median_ms": round(ms, 5), "copy_median_ms": round(mc, 5),
                  "shade_gb_per_s": round(traffic / (ms * 1e-3) / 1e9, 1),
                  "copy_gb_per_s": round(traffic / (mc * 1e-3) / 1e9, 1), "frac_of_copy": round(mc / ms, 4),
                  "spread_shade": spread(ts), "spread_copy": spread(tc),
                  "gsamples_per_s": round(k * k * W * H / (ms * 1e-3) / 1e9, 3), "march_clock_mhz": march_clock})
            del col, bo, src, dst
        del vlens
    scene.close()
write_out()
