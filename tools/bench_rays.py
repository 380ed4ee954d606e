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
Posed ray maps (one raymap.perspective map of camera A's field of view in camera space, camera A orbiting the hole by
0.2 degrees per frame; RGBA16F and BGRA8, both targets):
  pose1     one posed frame (Scene.render_frames_rays, n = 1) against Scene.render_rays over the map turned beforehand
            (raymap.apply_pose): what five multiply-adds per component and nine scalars cost.
  pose32    32 posed frames per launch against Scene.render_frames of the same 32 cameras (the rays agree to about
            1e-5): the yardstick of a form's cost.
  path32    the same 32 posed frames against the per-frame path they replace -- a torch matrix product that turns the
            map, then Scene.render_rays, 32 times -- and torch32: that path alone (it needs no posed entry point, so
            it also runs against an older library through BH_LIB).
  shutter   Scene.render_shutter_rays of n = 4, 8, 16 sub-frame poses against Scene.render_frames_rays of the same poses
            into n frames.
Origin maps (--legs origins, not in the default list; camera A's orbit as above, RGBA16F and BGRA8, both targets).  The
yardstick is always the existing posed form, interleaved in the same process:
  origins1   Scene.render_frames_rays(origins = an all-zero map), n = 1, against the same call without origins: the same
             rays and output bytes, so the ratio is the cost of the form alone (per-lane ro0 and cps, 12 more bytes per ray).
  origins32  the same with 32 frames per launch.
  thinlens   (1920x1080 only) raymap.thin_lens at ss = 4 against the posed ss = 4 render of raymap.perspective.
  ods        (4096x2048 only) raymap.ods against the posed render of raymap.equirect.
    python tools/bench_rays.py [--cases 1920x1080:256,4096x2048:512] [--frames 20] [--rounds 5] [--legs LIST] [--out FILE]"""
import argparse
import json
import math
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import black_hole_ray_marching_amd as bh  # noqa: E402
from black_hole_ray_marching_amd import raymap  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--cases", default="1920x1080:256,4096x2048:512", help="comma list of WxH:cap")
p.add_argument("--frames", type=int, default=20, help="launches per timed window")
p.add_argument("--rounds", type=int, default=5)
p.add_argument("--warm-ms", type=float, default=400.0, help="warm-up of both legs before a pair's first window")
p.add_argument("--out", default=None, help="also append the JSON rows to this file")
UNPOSED, POSED = {"rays", "equirect", "lens"}, {"pose1", "pose32", "path32", "torch32", "shutter"}
ORIGINS = {"origins"}
p.add_argument("--legs", default=",".join(sorted(UNPOSED | POSED)), help="comma list of the leg pairs to run (and: origins)")
args = p.parse_args()
LEGS = set(args.legs.split(","))
if LEGS - UNPOSED - POSED - ORIGINS:
    p.error(f"--legs: no such leg pair: {sorted(LEGS - UNPOSED - POSED - ORIGINS)}")
DEGREES, N_BATCH = 0.2, 32
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


for case in args.cases.split(",") if UNPOSED & LEGS else []:
    size, cap = case.split(":")
    W, H = (int(v) for v in size.split("x"))
    cap = int(cap)
    scene = bh.Scene(W, H, sky=sky, max_iters=cap, math=bh.BH_MATH_EXACT)
    s = torch.cuda.Stream()
    acc = torch.zeros(128, dtype=torch.int64, device="cuda")
    tags = dict(width=W, height=H, max_iters=cap)
    pin = torch.from_numpy(raymap.pinhole(scene.camera_uniform, W, H)).cuda()
    for name, (fmt, dt) in FMTS.items() if "rays" in LEGS else ():
        col, bo = (torch.empty((H, W, 4), dtype=dt, device="cuda") for _ in range(2))
        pair("rays", scene, s, acc, lambda st: scene.render_rays(pin, col, bo, fmt=fmt, stream=st),
             lambda st: scene.render(col, bo, fmt=fmt, stream=st), format=name, targets=2, map="pinhole", **tags)
    eq = torch.from_numpy(raymap.equirect(W, H, scene.camera.dir, scene.camera.up)).cuda()
    fmt, dt = FMTS["rgba16f"]
    col, bo = (torch.empty((H, W, 4), dtype=dt, device="cuda") for _ in range(2))
    if "equirect" in LEGS:
        pair("equirect", scene, s, acc, lambda st: scene.render_rays(eq, col, bo, fmt=fmt, stream=st), None,
             format="rgba16f", targets=2, map="equirect", **tags)
    lens = torch.empty((H, W, 2), dtype=torch.float32, device="cuda")
    if "lens" in LEGS:
        pair("lens", scene, s, acc, lambda st: scene.render_lens(lens, dirs=pin, stream=st),
             lambda st: scene.render_lens(lens, stream=st), map="pinhole", **tags)
    del pin, eq, col, bo, lens
    scene.close()
    torch.cuda.empty_cache()


def orbit_poses(scene, W, H, n, per_frame):
    """n cameras and their poses: camera A turned about the y axis by DEGREES * t / per_frame, looking at the hole"""
    cams, poses = [], []
    for t in range(n):
        a = math.radians(DEGREES * t / per_frame)
        c = bh.Camera.look_at((-20.0 * math.sin(a), 0.0, -20.0 * math.cos(a)), (0.0, 0.0, 0.0), W, H)
        cu = bh.CameraUniform()
        cu.update(c)
        cams.append(cu)
        poses.append(raymap.pose_of(c))
    return cams, poses


# ---- posed ray maps (bh_render_frames_rays, bh_render_frames_shutter_rays): one camera-space map, camera A's orbit ----
for case in args.cases.split(",") if POSED & LEGS else []:
    size, cap = case.split(":")
    W, H = (int(v) for v in size.split("x"))
    cap = int(cap)
    scene = bh.Scene(W, H, sky=sky, max_iters=cap, math=bh.BH_MATH_EXACT)
    s = torch.cuda.Stream()
    acc = torch.zeros(128, dtype=torch.int64, device="cuda")
    tags = dict(width=W, height=H, max_iters=cap)
    local_np = raymap.perspective(W, H, scene.camera.fovy)  # camera space: camera A's field of view
    local = torch.from_numpy(local_np).cuda()
    cams, poses = orbit_poses(scene, W, H, N_BATCH, 1)
    pose_rows = [np.frombuffer(bytes(q), np.float32).reshape(4, 3).copy() for q in poses]
    for name, (fmt, dt) in FMTS.items():
        fcol = [torch.empty((H, W, 4), dtype=dt, device="cuda") for _ in range(N_BATCH)]
        fbo = [torch.empty((H, W, 4), dtype=dt, device="cuda") for _ in range(N_BATCH)]
        if "pose1" in LEGS:  # (a) one posed frame against (b) render_rays over the map turned beforehand
            world = torch.from_numpy(raymap.apply_pose(poses[0], local_np)).cuda()
            pos = pose_rows[0][0]
            pair("pose1", scene, s, acc,
                 lambda st: scene.render_frames_rays(local, fcol[:1], fbo[:1], poses=poses[:1], fmt=fmt, stream=st),
                 lambda st: scene.render_rays(world, fcol[0], fbo[0], pos=pos, fmt=fmt, stream=st),
                 format=name, targets=2, map="perspective", a="render_frames_rays n=1", b="render_rays, world map", **tags)
            del world
        if "pose32" in LEGS:  # (c) 32 posed frames per launch against (d) render_frames of the same 32 cameras
            batch = scene.prepare_frames(fcol, fbo, fmt=fmt, math=bh.BH_MATH_EXACT)
            pair("pose32", scene, s, acc,
                 lambda st: scene.render_frames_rays(local, fcol, fbo, poses=poses, fmt=fmt, stream=st),
                 lambda st: batch.render(cameras=cams, stream=st),
                 format=name, targets=2, map="perspective", n_frames=N_BATCH, a="render_frames_rays", b="render_frames", **tags)
        if {"path32", "torch32"} & LEGS:  # (c) against (e): the torch product and render_rays per frame, 32 frames per "launch"
            turns = [torch.from_numpy(np.asarray(q_rows[1:], np.float32)).cuda() for q_rows in pose_rows]
            origins = [q_rows[0] for q_rows in pose_rows]

            def per_frame(st):
                with torch.cuda.stream(st):
                    for i in range(N_BATCH):
                        m = (local.reshape(-1, 3) @ turns[i]).reshape(local.shape)
                        scene.render_rays(m, fcol[i], fbo[i], pos=origins[i], fmt=fmt, stream=st)

            if "path32" in LEGS:
                pair("path32", scene, s, acc,
                     lambda st: scene.render_frames_rays(local, fcol, fbo, poses=poses, fmt=fmt, stream=st), per_frame,
                     format=name, targets=2, map="perspective", n_frames=N_BATCH, a="render_frames_rays",
                     b="torch product + render_rays per frame", **tags)
            if "torch32" in LEGS:
                pair("torch32", scene, s, acc, per_frame, None, format=name, targets=2, map="perspective",
                     n_frames=N_BATCH, a="torch product + render_rays per frame", **tags)
            del turns
        for n in (4, 8, 16) if "shutter" in LEGS else ():  # (f) a shutter over the map against its poses' n frames
            _, sub = orbit_poses(scene, W, H, n, n)
            pair("shutter", scene, s, acc,
                 lambda st: scene.render_shutter_rays(local, fcol[0], fbo[0], poses=sub, fmt=fmt, stream=st),
                 lambda st: scene.render_frames_rays(local, fcol[:n], fbo[:n], poses=sub, fmt=fmt, stream=st),
                 format=name, targets=2, map="perspective", n_sub=n, a="render_shutter_rays", b="render_frames_rays", **tags)
        del fcol, fbo
        torch.cuda.empty_cache()
    scene.close()

# ---- origin maps (bh_render_frames_rays_origins): the posed form of the same maps is the yardstick ---------------------
for case in args.cases.split(",") if ORIGINS & LEGS else []:
    size, cap = case.split(":")
    W, H = (int(v) for v in size.split("x"))
    cap = int(cap)
    scene = bh.Scene(W, H, sky=sky, max_iters=cap, math=bh.BH_MATH_EXACT)
    s = torch.cuda.Stream()
    acc = torch.zeros(128, dtype=torch.int64, device="cuda")
    tags = dict(width=W, height=H, max_iters=cap)
    local = torch.from_numpy(raymap.perspective(W, H, scene.camera.fovy)).cuda()
    zero = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    cams, poses = orbit_poses(scene, W, H, N_BATCH, 1)
    special = []  # (what, dirs of the new form, its origins, the yardstick's dirs, ss)
    if (W, H) == (1920, 1080):
        d, o = raymap.thin_lens(W, H, scene.camera.fovy, 0.05, 20.0, k=4)
        special.append(("thinlens", torch.from_numpy(d).cuda(), torch.from_numpy(o).cuda(),
                        torch.from_numpy(raymap.perspective(4 * W, 4 * H, scene.camera.fovy)).cuda(), 4))
        del d, o
    if (W, H) == (4096, 2048):
        d, o = raymap.ods(W, H, 0.065, "left")
        dd = torch.from_numpy(d).cuda()
        special.append(("ods", dd, torch.from_numpy(o).cuda(), dd, 1))
        del d, o
    for name, (fmt, dt) in FMTS.items():
        fcol = [torch.empty((H, W, 4), dtype=dt, device="cuda") for _ in range(N_BATCH)]
        fbo = [torch.empty((H, W, 4), dtype=dt, device="cuda") for _ in range(N_BATCH)]
        for n in (1, N_BATCH):
            pair(f"origins{n}", scene, s, acc,
                 lambda st: scene.render_frames_rays(local, fcol[:n], fbo[:n], poses=poses[:n], origins=zero, fmt=fmt, stream=st),
                 lambda st: scene.render_frames_rays(local, fcol[:n], fbo[:n], poses=poses[:n], fmt=fmt, stream=st),
                 format=name, targets=2, map="perspective", n_frames=n, a="render_frames_rays, zero origins",
                 b="render_frames_rays", **tags)
        for what, da, oa, db, k in special:
            pair(what, scene, s, acc,
                 lambda st: scene.render_frames_rays(da, fcol[:1], fbo[:1], poses=poses[:1], origins=oa, fmt=fmt, ss=k, stream=st),
                 lambda st: scene.render_frames_rays(db, fcol[:1], fbo[:1], poses=poses[:1], fmt=fmt, ss=k, stream=st),
                 format=name, targets=2, ss=k, n_frames=1, a=f"render_frames_rays, raymap.{what.replace('thinlens', 'thin_lens')}",
                 b="render_frames_rays, " + ("raymap.perspective" if what == "thinlens" else "raymap.equirect"), **tags)
        del fcol, fbo
        torch.cuda.empty_cache()
    del special, local, zero
    scene.close()
    torch.cuda.empty_cache()
if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    with open(args.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
