"""Offline multi-frame render along a scripted camera path: the reference's
frame (Scene::render into the two Bgra8UnormSrgb targets, then Bloom::render) per frame, the camera
driven by CameraController with a key script, PNG frames out.

    python tools/render_path.py --width 1024 --height 512 --frames 24 --dt 0.05 \\
        --script "W:0-12,ArrowLeft:6-24,P:12-18" --out gpurun_out/path
Script: comma-separated KEY:first-last frame ranges (keys held down), reference key names (W A S D
Space F ArrowUp/Down/Left/Right P O).

    python tools/render_path.py --shutter 8 --ss 2 --frames 4
Every frame integrated over a shutter interval: 8 sub-frame cameras per frame, averaged before the encode.

    python tools/render_path.py --sky-frames DIR --out frames/sky
A moving sky behind a still camera instead: one frame per image in DIR, the view marched once into a lens map.

    python tools/render_path.py --sky-filter mip --sky stars_16k.jpg --width 1920 --height 1080
The sky filtered through its mip chain: per frame a lens render and a filtered shade (bh_shade_lens_mip).

    python tools/render_path.py --projection equirect --ss 2 --width 2048 --height 1024
Another projection than the reference's pinhole: the frames march one ray map in camera space, uploaded once, each
with its camera's pose (bh_render_frames_rays, several frames per launch) -- a 360-degree equirectangular frame, a
fisheye:DEG dome frame, a perspective:DEG lens of another field of view.  With --shutter N every frame averages N
sub-frame poses over the same map (bh_render_frames_shutter_rays).

    python tools/render_path.py --projection ods:0.065 --width 4096 --height 2048
Omnidirectional stereo, the 360-degree format of VR players: two frame sets, OUT/left and OUT/right, each column's eye
on the viewing circle of diameter IPD (raymap.ods; an origin per ray beside the equirect map:
bh_render_frames_rays_origins).

    python tools/render_path.py --projection perspective:60 --ss 4 --aperture 0.05 --focus 20
Depth of field: the ss x ss samples of a pixel start on a thin lens of radius A and meet at distance D
(raymap.thin_lens).  The direction and origin maps are uploaded once per path.

    python tools/render_path.py --disc synthetic --disc-spin 0.01 --script "" --frames 120
A textured, turning accretion disc: each view is marched into a lens map and a hit map (bh_render_lens_hits) and
shaded with the disc texture turned by TURNS_PER_FRAME * frame turns of its inner edge (bh_shade_lens_disc).  A frame
whose camera did not move re-uses the last march: with a still camera (an empty --script) the path is one march and
one shade per frame.

    python tools/render_path.py --disc synthetic --disc-spin 0.01 --disc-beam 1 --script "" --frames 120
The same with Doppler beaming and gravitational redshift: the march also writes an arrival map
(bh_march_lens_arrivals) and the shade scales every disc hit by the fourth power of a Keplerian emitter's frequency
ratio (bh_shade_lens_disc_beamed) -- the approaching side bright, the receding side dim, the inner edge darkened.
--disc-sense -1 turns the matter the other way (a negative --disc-spin carries the texture that way)."""
import argparse
import dataclasses
import json
import sys
import time
from pathlib import Path

import numpy as np

p = argparse.ArgumentParser()
p.add_argument("--width", type=int, default=1024)
p.add_argument("--height", type=int, default=512)
p.add_argument("--frames", type=int, default=24)
p.add_argument("--dt", type=float, default=0.05)
p.add_argument("--max-iters", type=int, default=512)
p.add_argument("--script", default="W:0-12,ArrowLeft:6-24,P:12-18")
p.add_argument("--out", default="gpurun_out/path")
p.add_argument("--no-png", action="store_true")
p.add_argument("--ss", type=int, choices=[1, 2, 4, 8], default=1,
               help="rays per pixel side: ss x ss samples averaged in linear fp32 before the sRGB encode (bh_render_ss)")
p.add_argument("--adaptive", type=float, default=None, metavar="T",
               help="with --ss > 1: supersample only the 8x8 tiles that show an edge above T (bh_render_adaptive)")
p.add_argument("--sky", default=None, help="image file for the sky (e.g. the reference's space_4096x2048.jpg); "
                                            "default: the synthetic sky")
p.add_argument("--sky-frames", default=None, metavar="DIR",
               help="a moving sky behind a still camera: one output frame per image file in DIR (sorted by name), "
                    "the default camera marched once into a lens map (bh_render_lens) and shaded with each image "
                    "(bh_shade_lens); --script, --frames and --dt are not used")
p.add_argument("--shutter", type=int, choices=[1, 2, 4, 8, 16], default=1, metavar="N",
               help="N sub-frame cameras per frame, averaged in linear fp32 before the sRGB encode (bh_render_shutter): "
                    "camera t of a frame is where a copy of the controller takes the frame's camera in dt * S * t / N")
p.add_argument("--shutter-frac", type=float, default=0.5, metavar="S",
               help="with --shutter: the part of a frame's dt the shutter stays open (default 0.5)")
p.add_argument("--sky-filter", choices=["none", "mip"], default="none",
               help="mip: every frame is a lens render (bh_render_lens) shaded through the sky's mip chain, the level "
                    "taken from the lens (bh_shade_lens_mip); with --ss 1, 2 or 4 and with --sky-frames")
p.add_argument("--aperture", type=float, default=None, metavar="A",
               help="with --projection perspective:DEG: a thin lens of radius A (world units) focused at --focus; the "
                    "--ss x --ss samples of a pixel are its lens samples")
p.add_argument("--focus", type=float, default=None, metavar="D", help="with --aperture: the distance of the plane in focus")
p.add_argument("--projection", default=None, metavar="{pinhole,equirect,fisheye:DEG,perspective:DEG,ods:IPD}",
               help="march a ray map instead of the camera's own rays: the map of the (ss x) frame is built and uploaded "
                    "once, in the camera's frame, and every frame passes its camera's pose (bh_render_frames_rays; "
                    "with --shutter, bh_render_frames_shutter_rays); pinhole is the camera's own projection through a "
                    "per-frame map of the library's helper (bh_render_rays: the same bytes); DEG: the full field of "
                    "view of a fisheye (up to 360), the vertical one of a perspective lens (below 180); ods:IPD: "
                    "omnidirectional stereo, two frame sets (left, right) with the eyes IPD apart (world units)")
p.add_argument("--disc", default=None, metavar="{synthetic,IMAGE}",
               help="texture the accretion disc: bh.synthetic_disc(), or an image file whose columns run around the disc "
                    "and whose rows run from its inner to its outer edge; every frame is a lens march with a hit map "
                    "(only when the camera moved) and a disc shade")
p.add_argument("--disc-spin", type=float, default=0.0, metavar="TURNS_PER_FRAME",
               help="with --disc: turns of the disc's inner edge per frame (Keplerian: slower further out)")
p.add_argument("--disc-gain", type=float, default=1.0, metavar="G", help="with --disc: the disc colour's multiplier")
p.add_argument("--disc-beam", type=float, default=None, metavar="B",
               help="with --disc: beam the disc -- 0..1, 0 the unbeamed colours, 1 the full Doppler and redshift factor g^4")
p.add_argument("--disc-sense", type=int, default=1, choices=(1, -1),
               help="with --disc-beam: +1 the matter moves the way a growing --disc-spin carries the texture, -1 the other way")
args = p.parse_args()
if args.disc and (args.projection or args.shutter > 1 or args.adaptive is not None or args.sky_frames
                  or args.sky_filter != "none" or args.aperture is not None):
    sys.exit("render_path: --disc takes the camera's own rays and --ss only (no --projection, --shutter, --adaptive, "
             "--sky-frames, --sky-filter or --aperture)")
if not args.disc and (args.disc_spin != 0.0 or args.disc_gain != 1.0):
    p.error("--disc-spin and --disc-gain go with --disc")
if not (abs(args.disc_spin) < float("inf") and 0.0 <= args.disc_gain < float("inf")):
    p.error("--disc-spin must be finite and --disc-gain finite and 0 or more")
if args.disc_beam is None and args.disc_sense != 1:
    p.error("--disc-sense goes with --disc-beam")
if args.disc_beam is not None and not (args.disc and 0.0 <= args.disc_beam <= 1.0):
    p.error("--disc-beam goes with --disc and lies in 0..1")
mip = args.sky_filter == "mip"
proj, proj_deg = None, None
if args.projection is not None:
    proj, _, deg = args.projection.partition(":")
    if proj not in ("pinhole", "equirect", "fisheye", "perspective", "ods") or bool(deg) != (proj in ("fisheye", "perspective", "ods")):
        p.error("--projection is one of pinhole, equirect, fisheye:DEG, perspective:DEG, ods:IPD")
    try:
        proj_deg = float(deg) if deg else None
    except ValueError:
        p.error(f"--projection {proj}:{'IPD' if proj == 'ods' else 'DEG'} needs a number, got {deg!r}")
    if proj == "ods" and not 0.0 <= proj_deg < float("inf"):
        p.error("--projection ods: IPD must be a finite distance, 0 or more")
    if proj != "ods" and proj_deg is not None and not 0.0 < proj_deg <= (360.0 if proj == "fisheye" else 179.9):
        p.error(f"--projection {proj}: DEG must lie in (0, {360 if proj == 'fisheye' else 179.9}]")
    if args.adaptive is not None:
        sys.exit("render_path: --projection does not combine with --adaptive (ray maps are not built for adaptive renders)")
    if args.shutter > 1 and proj == "pinhole":
        sys.exit("render_path: --projection pinhole does not combine with --shutter (its map is per camera; the plain "
                 "--shutter is the same picture)")
thin = args.aperture is not None
if thin or args.focus is not None:
    if not thin or args.focus is None or proj != "perspective":
        p.error("--aperture A and --focus D go together, with --projection perspective:DEG (and --ss k: the lens samples)")
    if not (0.0 <= args.aperture < float("inf") and 0.0 < args.focus < float("inf")):
        p.error("--aperture must be 0 or more and --focus positive")
if thin or proj == "ods":  # a ray origin per pixel: what the origin-map kernels are not built for
    if args.shutter > 1 or args.adaptive is not None:
        sys.exit("render_path: --projection ods and --aperture do not combine with --shutter or --adaptive (an origin "
                 "map has no shutter or adaptive form)")
    if args.sky_filter == "mip" or args.sky_frames:
        sys.exit("render_path: --projection ods and --aperture do not combine with --sky-filter mip or --sky-frames")
if mip and (args.shutter > 1 or args.adaptive is not None):
    sys.exit("render_path: --sky-filter mip does not combine with --shutter or --adaptive (the filter is a lens shade)")
if mip and args.ss == 8:
    sys.exit("render_path: --sky-filter mip takes --ss 1, 2 or 4 (bh_shade_lens_mip has no ss = 8)")
if args.shutter > 1 and (args.adaptive is not None or args.sky_frames):
    sys.exit("render_path: --shutter does not combine with --adaptive or --sky-frames (no adaptive or lens shutter)")
if args.adaptive is not None and args.ss == 1:
    p.error("--adaptive needs --ss 2, 4 or 8")
if args.sky_frames and args.adaptive is not None:
    p.error("--sky-frames shades a lens map: there is no adaptive lens")
# the arguments are good: now the imports that take seconds
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

import black_hole_ray_marching_amd as bh  # noqa: E402
from black_hole_ray_marching_amd import raymap  # noqa: E402
from black_hole_ray_marching_amd.png import write_png  # noqa: E402
W, H = args.width, args.height
keys = []
for item in filter(None, args.script.split(",")):
    k, rng = item.split(":")
    a, b = (int(v) for v in rng.split("-"))
    keys.append((k, a, b))
out_dir = Path(args.out)
out_dir.mkdir(parents=True, exist_ok=True)
sky = bh.load_sky(args.sky) if args.sky else bh.synthetic_sky()
scene = bh.Scene(W, H, sky=sky, max_iters=args.max_iters, math=bh.BH_MATH_EXACT)
ctrl = bh.CameraController()
cam = bh.Camera.default(W, H)
col = torch.empty((H, W, 4), dtype=torch.uint8, device="cuda")
bo = torch.empty_like(col)
surf = torch.empty_like(col)
log = []


def shutter_subcameras(frame_cam):
    """The N sub-frame cameras of a frame: a copy of the controller's state moves a copy of the frame's camera
    by dt * S * t / N (t = 0: the frame's own camera); the path itself is untouched."""
    out = []
    for t in range(args.shutter):
        c2 = bh.CameraController()
        c2.c = type(ctrl.c).from_buffer_copy(ctrl.c)
        sub, _ = c2.update_camera(dataclasses.replace(frame_cam), args.dt * args.shutter_frac * t / args.shutter)
        out.append(sub)
    return out


def shutter_cameras(frame_cam):
    """... as the CameraUniforms bh_render_shutter takes."""
    out = []
    for sub in shutter_subcameras(frame_cam):
        cu = bh.CameraUniform()
        cu.update(sub)
        out.append(cu)
    return out


local_map, map_uploads = None, 0
views = None  # with an origin per ray: [(frame set's sub-directory, the origin map)] over local_map
if proj == "ods":  # one equirect map, one origin map per eye
    d, left = raymap.ods(W * args.ss, H * args.ss, proj_deg, "left")
    local_map = torch.from_numpy(d).cuda()
    views = [("left", torch.from_numpy(left).cuda()),
             ("right", torch.from_numpy(raymap.ods(W * args.ss, H * args.ss, proj_deg, "right")[1]).cuda())]
    map_uploads += 3
elif thin:  # the virtual frame's directions and lens points
    d, o = raymap.thin_lens(W, H, np.radians(proj_deg), args.aperture, args.focus, k=args.ss)
    local_map, views = torch.from_numpy(d).cuda(), [("", torch.from_numpy(o).cuda())]
    map_uploads += 2
elif proj in ("equirect", "fisheye", "perspective"):  # once per frame size, in the camera's own frame (r, u, f)
    kw, kh = args.ss * W, args.ss * H
    m = (raymap.equirect(kw, kh) if proj == "equirect" else raymap.fisheye(kw, kh, np.radians(proj_deg))
         if proj == "fisheye" else raymap.perspective(kw, kh, np.radians(proj_deg)))
    local_map = torch.from_numpy(m).cuda()  # the run's only map: every frame passes a pose with it
    map_uploads += 1


def pinhole_map(frame_cam):
    """--projection pinhole: the camera's own map in world space, from the library's helper, per frame."""
    global map_uploads
    cu = bh.CameraUniform()
    cu.update(frame_cam)
    map_uploads += 1
    return torch.from_numpy(raymap.pinhole(cu, args.ss * W, args.ss * H)).cuda()


def lens_of(lens, frame_cam):
    """The frame's view into `lens`: the camera's own rays, its pinhole map, or the local map under its pose."""
    k = args.ss
    if not proj:
        scene.render_lens(lens, width=k * W, height=k * H)
    elif local_map is None:
        scene.render_lens(lens, width=k * W, height=k * H, dirs=pinhole_map(frame_cam))
    else:
        scene.render_lens(lens, width=k * W, height=k * H, dirs=local_map, pose=raymap.pose_of(frame_cam))


t0 = time.perf_counter()
if args.sky_frames:
    images = sorted(q for q in Path(args.sky_frames).iterdir() if q.is_file())
    if not images:
        sys.exit(f"render_path: no image files in {args.sky_frames}")
    k = args.ss
    scene.update(cam)
    lens = torch.empty((k * H, k * W, 2), dtype=torch.float32, device="cuda")
    lens_of(lens, cam)  # the only march of the run
    for f, path in enumerate(images):
        frame_sky = bh.Sky(scene, bh.load_sky(path), mips=mip)
        scene.shade(lens, col, bo, fmt=bh.BH_OUT_BGRA8_SRGB, sky=frame_sky, ss=k, mip=mip)
        scene.bloom(col, bo, surf)
        if not args.no_png:
            write_png(out_dir / f"frame_{f:04d}.png", surf.cpu().numpy())
        torch.cuda.synchronize()  # the shade has read the sky
        frame_sky.close()
        log.append({"frame": f, "sky": path.name, "pos": cam.pos, "dir": cam.dir, "moved": False})
    args.frames = len(images)
marches = None
if args.disc:  # a lens and a hit map per view, a disc shade per frame
    disc = bh.Disc(scene, bh.synthetic_disc() if args.disc == "synthetic" else bh.load_sky(args.disc))
    k, marches = args.ss, 0
    lens = torch.empty((k * H, k * W, 2), dtype=torch.float32, device="cuda")
    hits = torch.empty((k * H, k * W, 3), dtype=torch.float32, device="cuda")
    beam = {}  # --disc-beam: the arrival map beside the hit map, for the march and for the shade
    if args.disc_beam is not None:
        beam = dict(arrivals=torch.empty((k * H, k * W, 3), dtype=torch.float32, device="cuda"))
    for f in range(args.frames):
        for key, a, b in keys:
            ctrl.process_key(key, a <= f <= b)
        cam, moved = ctrl.update_camera(cam, args.dt)
        if f == 0 or moved:
            scene.update(cam)
            scene.render_lens(lens, width=k * W, height=k * H, hits=hits, **beam)
            marches += 1
        scene.shade(lens, col, bo, fmt=bh.BH_OUT_BGRA8_SRGB, ss=k, hits=hits, disc=disc, spin=args.disc_spin * f,
                    gain=args.disc_gain, **beam, **(dict(beam=args.disc_beam, sense=args.disc_sense) if beam else {}))
        scene.bloom(col, bo, surf)
        if not args.no_png:
            write_png(out_dir / f"frame_{f:04d}.png", surf.cpu().numpy())
        log.append({"frame": f, "pos": cam.pos, "dir": cam.dir, "moved": moved})
if mip and not args.sky_frames:  # the path's own sky with its chain, and the lens every frame marches into
    path_sky = bh.Sky(scene, sky, mips=True)
    path_lens = torch.empty((args.ss * H, args.ss * W, 2), dtype=torch.float32, device="cuda")
# a projection's frames in batches: one launch marches the batch's frames (with --shutter: their sub-frame poses)
posed = local_map is not None and not mip and not args.sky_frames
batch = max(1, min(8, 256 // args.shutter))
targets = [(torch.empty_like(col), torch.empty_like(bo)) for _ in range(min(batch, args.frames))] if posed else []
f0 = 0
while posed and f0 < args.frames:
    nb = min(batch, args.frames - f0)
    poses = []
    for f in range(f0, f0 + nb):
        for k, a, b in keys:
            ctrl.process_key(k, a <= f <= b)
        cam, moved = ctrl.update_camera(cam, args.dt)
        poses.append([raymap.pose_of(c) for c in (shutter_subcameras(cam) if args.shutter > 1 else [cam])])
        log.append({"frame": f, "pos": cam.pos, "dir": cam.dir, "moved": moved})
    cols, bos = [t[0] for t in targets[:nb]], [t[1] for t in targets[:nb]]
    for sub, origin_map in views or [("", None)]:
        if args.shutter > 1:
            scene.render_frames_shutter_rays(local_map, cols, bos, poses=poses, fmt=bh.BH_OUT_BGRA8_SRGB, ss=args.ss)
        else:
            scene.render_frames_rays(local_map, cols, bos, poses=[g[0] for g in poses], origins=origin_map,
                                     fmt=bh.BH_OUT_BGRA8_SRGB, ss=args.ss)
        for i in range(nb):
            scene.bloom(cols[i], bos[i], surf)
            if not args.no_png:
                (out_dir / sub).mkdir(parents=True, exist_ok=True)
                write_png(out_dir / sub / f"frame_{f0 + i:04d}.png", surf.cpu().numpy())
    f0 += nb
for f in range(0 if args.sky_frames or posed or args.disc else args.frames):
    for k, a, b in keys:
        ctrl.process_key(k, a <= f <= b)
    cam, moved = ctrl.update_camera(cam, args.dt)
    scene.update(cam)
    if mip:
        lens_of(path_lens, cam)
        scene.shade(path_lens, col, bo, fmt=bh.BH_OUT_BGRA8_SRGB, sky=path_sky, ss=args.ss, mip=True)
    elif proj:
        scene.render_rays(pinhole_map(cam), col, bo, fmt=bh.BH_OUT_BGRA8_SRGB, ss=args.ss)  # pinhole (the others: above)
    elif args.shutter > 1:
        scene.render_shutter(col, bo, cameras=shutter_cameras(cam), fmt=bh.BH_OUT_BGRA8_SRGB, ss=args.ss)
    else:
        scene.render(col, bo, fmt=bh.BH_OUT_BGRA8_SRGB, ss=args.ss, adaptive=args.adaptive)
    scene.bloom(col, bo, surf)
    if not args.no_png:
        write_png(out_dir / f"frame_{f:04d}.png", surf.cpu().numpy())
    log.append({"frame": f, "pos": cam.pos, "dir": cam.dir, "moved": moved})
torch.cuda.synchronize()
dt = time.perf_counter() - t0
(out_dir / "path.json").write_text(json.dumps(log, indent=0))
print(json.dumps({"frames": args.frames, "width": W, "height": H, "ss": args.ss, "adaptive": args.adaptive, "shutter": args.shutter, "sky_filter": args.sky_filter, "projection": args.projection, "map_uploads": map_uploads, "disc": args.disc, "disc_beam": args.disc_beam, "marches": marches, "seconds": round(dt, 3),
                  "frames_per_s_incl_png": round(args.frames / dt, 2), "out": str(out_dir)}))
