"""Ray maps for Scene.render_rays / Scene.render_lens(dirs=...): host-side builders, numpy arrays (H, W, 3) float32.
thin_lens, ods, orthographic and stereo return a pair (dirs, origins) for Scene.render_frames_rays(origins=...).

A ray map holds one direction per pixel (include/bh_render.h, "Ray maps"); the kernel normalises it, so a builder
may return any positive multiple of the direction it means.  Upload a map with `torch.from_numpy(m).cuda()`.

`pinhole` goes through the C helper and is defined to the bit: render_rays over it is render().  The other
builders compute in float64 and round once to float32; they promise their formula (each docstring states it), not
bits.  Conventions shared by them: pixel (x, y) has its centre at ((x + 0.5) / W, (y + 0.5) / H), y grows downwards;
the view's frame is right-handed from `forward` and `up` as the scene's camera builds it -- f = forward / |forward|,
r = normalize(cross(up, f)), u = cross(f, r) -- so +x on the image is r and +y on the image is -u.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._abi import BhError, check, load

FACES = ("+x", "-x", "+y", "-y", "+z", "-z")


def _size(W, H) -> tuple[int, int]:
    ok = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) and 1 <= int(v) <= 65536 for v in (W, H))
    if not ok:
        raise BhError(_abi.BH_ERR_INVALID_ARG, f"raymap: width and height must be integers in 1..65536, got {W!r} x {H!r}")
    return int(W), int(H)


def _angle(a, what: str, hi: float) -> float:
    try:
        v = float(a)
    except (TypeError, ValueError):
        v = float("nan")
    if not 0.0 < v <= hi:
        raise BhError(_abi.BH_ERR_INVALID_ARG, f"raymap: {what} must be an angle in (0, {hi:.6g}] radians, got {a!r}")
    return v


def basis(forward, up) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(r, u, f) in float64 from a view direction and an up hint (neither zero nor parallel)."""
    try:
        f = np.asarray(forward, np.float64).reshape(3)
        v = np.asarray(up, np.float64).reshape(3)
    except (TypeError, ValueError):
        raise BhError(_abi.BH_ERR_INVALID_ARG, "raymap: forward and up must be three numbers each")
    nf = np.linalg.norm(f)
    r = np.cross(v, f)
    nr = np.linalg.norm(r)
    if not (np.isfinite(nf) and nf > 0.0 and np.isfinite(nr) and nr > 1e-12 * nf * max(np.linalg.norm(v), 1e-300)):
        raise BhError(_abi.BH_ERR_INVALID_ARG, "raymap: forward and up must be finite, non-zero and not parallel")
    f = f / nf
    r = r / nr
    return r, np.cross(f, r), f


def _centres(W: int, H: int) -> tuple[np.ndarray, np.ndarray]:
    """The pixel centres as fractions of the image, sx (1, W) and sy (H, 1), float64."""
    return ((np.arange(W, dtype=np.float64) + 0.5) / W)[None, :], ((np.arange(H, dtype=np.float64) + 0.5) / H)[:, None]


def _compose(a, b, c, r, u, f) -> np.ndarray:
    """a r + b u + c f per pixel, rounded once to float32."""
    d = a[..., None] * r + b[..., None] * u + c[..., None] * f
    return np.ascontiguousarray(d, dtype=np.float32)


def pinhole(camera_uniform, W: int, H: int) -> np.ndarray:
    """bh_ray_map_pinhole_host: the scene's own projection -- the unnormalised interpolated vector of
    `camera_uniform`'s screen triangle at every pixel centre, in the kernel's fp32 operations.  render_rays over it,
    from camera_uniform.pos, is render() bit for bit."""
    W, H = _size(W, H)
    out = np.empty((H, W, 3), np.float32)
    cu = getattr(camera_uniform, "c", camera_uniform)
    check(load().bh_ray_map_pinhole_host(C.byref(cu), W, H, out.ctypes.data), "bh_ray_map_pinhole_host")
    return out


def perspective(W: int, H: int, fovy: float, forward=(0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0)) -> np.ndarray:
    """A pinhole lens of vertical field of view `fovy` (radians, below pi), square pixels:
    d = f + (2 sx - 1) t (W / H) r + (1 - 2 sy) t u,  t = tan(fovy / 2)."""
    W, H = _size(W, H)
    t = np.tan(0.5 * _angle(fovy, "fovy", np.nextafter(np.pi, 0.0)))
    r, u, f = basis(forward, up)
    sx, sy = _centres(W, H)
    a = np.broadcast_to((2.0 * sx - 1.0) * (t * W / H), (H, W))
    b = np.broadcast_to((1.0 - 2.0 * sy) * t, (H, W))
    return _compose(a, b, np.ones((H, W)), r, u, f)


def equirect(W: int, H: int, forward=(0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0)) -> np.ndarray:
    """The full sphere, longitude along x and latitude along y:
    lon = (2 sx - 1) pi, lat = (0.5 - sy) pi,  d = cos(lat) sin(lon) r + sin(lat) u + cos(lat) cos(lon) f.
    The image's centre looks along `forward`, its top row towards `up`."""
    W, H = _size(W, H)
    r, u, f = basis(forward, up)
    sx, sy = _centres(W, H)
    lon, lat = (2.0 * sx - 1.0) * np.pi, (0.5 - sy) * np.pi
    return _compose(np.cos(lat) * np.sin(lon), np.broadcast_to(np.sin(lat), (H, W)), np.cos(lat) * np.cos(lon), r, u, f)


def fisheye(W: int, H: int, fov: float, forward=(0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0)) -> np.ndarray:
    """An equidistant fisheye of full field of view `fov` (radians, up to 2 pi) across the image circle, the circle
    inscribed in the image: with (X, Y) = ((2 sx - 1) W, (1 - 2 sy) H) / min(W, H) and rho = min(|(X, Y)|, 1),
    theta = rho fov / 2,  d = sin(theta) (X r + Y u) / |(X, Y)| + cos(theta) f.
    A pixel outside the circle holds the direction of the nearest rim point, so every pixel has a finite ray."""
    W, H = _size(W, H)
    half = 0.5 * _angle(fov, "fov", 2.0 * np.pi)
    r, u, f = basis(forward, up)
    sx, sy = _centres(W, H)
    m = float(min(W, H))
    X = np.broadcast_to((2.0 * sx - 1.0) * (W / m), (H, W))
    Y = np.broadcast_to((1.0 - 2.0 * sy) * (H / m), (H, W))
    rad = np.hypot(X, Y)
    theta = np.minimum(rad, 1.0) * half
    safe = np.where(rad > 0.0, rad, 1.0)
    s = np.sin(theta)
    return _compose(s * X / safe, s * Y / safe, np.cos(theta), r, u, f)


def cube_face(N: int, face: str, forward=(0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0)) -> np.ndarray:
    """One N x N face of a cube map in the frame (r, u, f): face "+z" looks along f, "-z" against it, "+x" along r,
    "+y" along u.  With a = 2 sx - 1 and b = 1 - 2 sy the direction is, in (r, u, f) coordinates,
    +x: (1, b, -a)  -x: (-1, b, a)  +y: (a, 1, -b)  -y: (a, -1, b)  +z: (a, b, 1)  -z: (-a, b, -1)."""
    N, _ = _size(N, N)
    if face not in FACES:
        raise BhError(_abi.BH_ERR_INVALID_ARG, f"raymap: face must be one of {FACES}, got {face!r}")
    r, u, f = basis(forward, up)
    sx, sy = _centres(N, N)
    a = np.broadcast_to(2.0 * sx - 1.0, (N, N))
    b = np.broadcast_to(1.0 - 2.0 * sy, (N, N))
    one = np.ones((N, N))
    x, y, z = {"+x": (one, b, -a), "-x": (-one, b, a), "+y": (a, one, -b), "-y": (a, -one, b),
               "+z": (a, b, one), "-z": (-a, b, -one)}[face]
    return _compose(x, y, z, r, u, f)


def pose(pos, forward=(0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0)) -> _abi.bh_ray_pose:
    """A camera for a map in camera space (bh_ray_pose; Scene.render_frames_rays): the position and the rows
    (r, u, f) of `basis(forward, up)`, each rounded once to float32.  A map built with the default forward and up
    (its x along r, y along u, z along f) and turned by this pose looks along `forward`."""
    try:
        p = np.asarray(pos, np.float64).reshape(3)
    except (TypeError, ValueError):
        raise BhError(_abi.BH_ERR_INVALID_ARG, f"raymap: pos must be three numbers, got {pos!r}")
    r, u, f = basis(forward, up)
    out = _abi.bh_ray_pose()
    for name, v in (("pos", p), ("r", r), ("u", u), ("f", f)):
        setattr(out, name, (C.c_float * 3)(*np.asarray(v, np.float32).tolist()))
    return out


def pose_of(camera) -> _abi.bh_ray_pose:
    """pose() of a scene camera (its pos, dir and up; a Camera or anything with those three attributes)."""
    try:
        return pose(camera.pos, camera.dir, camera.up)
    except AttributeError:
        raise BhError(_abi.BH_ERR_INVALID_ARG, f"raymap: pose_of takes a camera with pos, dir and up, got {type(camera).__name__}")


def pose_rows(p) -> np.ndarray:
    """The 12 floats of a pose as a (4, 3) float32 array: pos, r, u, f."""
    return np.frombuffer(bytes(p), np.float32).reshape(4, 3).copy()


def apply_pose(p, dirs) -> np.ndarray:
    """bh_ray_pose_apply_host: the camera-space map `dirs` (H, W, 3) turned by pose `p` -- (mx r + my u) + mz f per
    pixel, in the kernels' fp32 operations -- the world-space map whose render_rays from the pose's position is the
    posed render, bit for bit."""
    d = np.ascontiguousarray(dirs, dtype=np.float32)
    if d.ndim != 3 or d.shape[2] != 3:
        raise BhError(_abi.BH_ERR_INVALID_ARG, f"raymap: dirs must be (H, W, 3), got {d.shape}")
    if not isinstance(p, _abi.bh_ray_pose):
        rows = np.ascontiguousarray(p, dtype=np.float32)
        if rows.shape != (4, 3):
            raise BhError(_abi.BH_ERR_INVALID_ARG, "raymap: a pose is a raymap.pose or four rows of three floats (pos, r, u, f)")
        p = _abi.bh_ray_pose.from_buffer_copy(rows.tobytes())
    H, W = _size(d.shape[1], d.shape[0])[::-1]
    out = np.empty((H, W, 3), np.float32)
    check(load().bh_ray_pose_apply_host(C.byref(p), d.ctypes.data, W, H, out.ctypes.data), "bh_ray_pose_apply_host")
    return out


def _pose_c(p) -> _abi.bh_ray_pose:
    if isinstance(p, _abi.bh_ray_pose):
        return p
    rows = np.ascontiguousarray(p, dtype=np.float32)
    if rows.shape != (4, 3):
        raise BhError(_abi.BH_ERR_INVALID_ARG, "raymap: a pose is a raymap.pose or four rows of three floats (pos, r, u, f)")
    return _abi.bh_ray_pose.from_buffer_copy(rows.tobytes())


def apply_origins(p, origins) -> np.ndarray:
    """bh_ray_origins_apply_host: the camera-space origin map `origins` (H, W, 3) under pose `p` --
    pos + ((ox r + oy u) + oz f) per pixel, in the kernels' fp32 operations -- the world-space origin of every ray
    of Scene.render_frames_rays(origins=...), bit for bit."""
    o = np.ascontiguousarray(origins, dtype=np.float32)
    if o.ndim != 3 or o.shape[2] != 3:
        raise BhError(_abi.BH_ERR_INVALID_ARG, f"raymap: origins must be (H, W, 3), got {o.shape}")
    p = _pose_c(p)
    H, W = _size(o.shape[1], o.shape[0])[::-1]
    out = np.empty((H, W, 3), np.float32)
    check(load().bh_ray_origins_apply_host(C.byref(p), o.ctypes.data, W, H, out.ctypes.data), "bh_ray_origins_apply_host")
    return out


# ---- pairs (dirs, origins) for Scene.render_frames_rays(origins=...): both in camera space (x right, y up, z forward;
# the pose places them), both (H, W, 3) float32, computed in float64 and rounded once ---------------------------------

def _length(v, what: str, zero_ok: bool = False) -> float:
    try:
        x = float(v)
    except (TypeError, ValueError):
        x = float("nan")
    if not (np.isfinite(x) and (x > 0.0 or (zero_ok and x == 0.0))):
        raise BhError(_abi.BH_ERR_INVALID_ARG, f"raymap: {what} must be a finite {'non-negative' if zero_ok else 'positive'} "
                                               f"number, got {v!r}")
    return x


def _hash01(counter: np.ndarray, seed: int, stream: int) -> np.ndarray:
    """A counter-based hash to [0, 1): splitmix64's finaliser over counter, seed and stream, the top 53 bits."""
    with np.errstate(over="ignore"):
        z = counter.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64((int(seed) * 0xD1B54A32D192ED03 + stream * 0x8CB92BA72F3D8DD7 + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def _concentric(a: np.ndarray, b: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """Shirley and Chiu's concentric map of the square [-1, 1]^2 onto the unit disc (area-preserving)."""
    wide = np.abs(a) > np.abs(b)
    with np.errstate(divide="ignore", invalid="ignore"):
        rad = np.where(wide, a, b)
        phi = np.where(wide, (np.pi / 4.0) * (b / a), (np.pi / 2.0) - (np.pi / 4.0) * (a / b))
    phi = np.where((a == 0.0) & (b == 0.0), 0.0, phi)
    return rad * np.cos(phi), rad * np.sin(phi)


def thin_lens(W: int, H: int, fovy: float, aperture: float, focus: float, k: int = 1, seed: int = 0):
    """A thin lens of radius `aperture` focused at distance `focus` along z, for a render with ss = k: the maps of the
    virtual frame (k H, k W, 3), whose k x k samples per pixel are the lens samples.  Sample (i, j) of pixel (x, y)
    takes the point ((i + jx) / k, (j + jy) / k) of the unit square -- stratum (i, j), with (jx, jy) in [0, 1)^2 a
    counter-based hash of (the pixel's index y W + x, seed) -- which the concentric map takes to (lx, ly) on the unit
    disc.  With p = ((2 sx - 1) t W / H, (1 - 2 sy) t, 1), t = tan(fovy / 2), the `perspective` direction of the pixel's
    CENTRE:
        origin = (aperture lx, aperture ly, 0),    d = p - origin / focus   (a positive multiple of focus p - origin)
    so every sample of a pixel passes through focus p, on the plane z = focus.  aperture = 0 gives zero origins and
    `perspective(W, H, fovy)` with each pixel repeated k x k."""
    W, H = _size(W, H)
    if k not in (1, 2, 4, 8):
        raise BhError(_abi.BH_ERR_INVALID_ARG, f"raymap: k must be 1, 2, 4 or 8 (the render's ss), got {k!r}")
    _size(W * k, H * k)
    if not isinstance(seed, (int, np.integer)) or isinstance(seed, bool) or seed < 0:
        raise BhError(_abi.BH_ERR_INVALID_ARG, f"raymap: seed must be a non-negative integer, got {seed!r}")
    t = np.tan(0.5 * _angle(fovy, "fovy", np.nextafter(np.pi, 0.0)))
    A, D = _length(aperture, "aperture", zero_ok=True), _length(focus, "focus")
    sx, sy = _centres(W, H)
    px = np.repeat(np.repeat(np.broadcast_to((2.0 * sx - 1.0) * (t * W / H), (H, W)), k, 0), k, 1)
    py = np.repeat(np.repeat(np.broadcast_to((1.0 - 2.0 * sy) * t, (H, W)), k, 0), k, 1)
    vy, vx = np.meshgrid(np.arange(H * k), np.arange(W * k), indexing="ij")
    pixel = (vy // k) * W + (vx // k)
    u0 = ((vx % k) + _hash01(pixel, seed, 0)) / k
    u1 = ((vy % k) + _hash01(pixel, seed, 1)) / k
    lx, ly = _concentric(2.0 * u0 - 1.0, 2.0 * u1 - 1.0)
    ox, oy = A * lx + 0.0, A * ly + 0.0  # (+ 0.0: a -0 becomes +0, so aperture 0 gives the all +0 map of the identity)
    z = np.zeros_like(ox)
    dirs = np.stack([px - ox / D, py - oy / D, np.ones_like(ox)], -1)
    return np.ascontiguousarray(dirs, np.float32), np.ascontiguousarray(np.stack([ox, oy, z], -1), np.float32)


def ods(W: int, H: int, ipd: float, eye: str):
    """Omnidirectional stereo, one eye of the 360 degree pair: dirs = equirect(W, H), and with lon = (2 sx - 1) pi
        origin = +-(ipd / 2) (cos lon, 0, -sin lon)      (eye "right": +, "left": -)
    -- the eye sits on the viewing circle of diameter `ipd`, on the tangent perpendicular to its column's horizontal
    direction (sin lon, 0, cos lon)."""
    W, H = _size(W, H)
    if eye not in ("left", "right"):
        raise BhError(_abi.BH_ERR_INVALID_ARG, f'raymap: eye must be "left" or "right", got {eye!r}')
    h = 0.5 * _length(ipd, "ipd", zero_ok=True) * (1.0 if eye == "right" else -1.0)
    sx, _ = _centres(W, H)
    lon = np.broadcast_to((2.0 * sx - 1.0) * np.pi, (H, W))
    o = np.stack([h * np.cos(lon), np.zeros((H, W)), -h * np.sin(lon)], -1)
    return equirect(W, H), np.ascontiguousarray(o, np.float32)


def orthographic(W: int, H: int, half_height: float):
    """Parallel rays along z: every direction (0, 0, 1),
        origin = ((2 sx - 1) half_height W / H, (1 - 2 sy) half_height, 0)."""
    W, H = _size(W, H)
    hh = _length(half_height, "half_height")
    sx, sy = _centres(W, H)
    o = np.stack([np.broadcast_to((2.0 * sx - 1.0) * (hh * W / H), (H, W)), np.broadcast_to((1.0 - 2.0 * sy) * hh, (H, W)),
                  np.zeros((H, W))], -1)
    d = np.zeros((H, W, 3), np.float32)
    d[..., 2] = 1.0
    return d, np.ascontiguousarray(o, np.float32)


def stereo(W: int, H: int, fovy: float, ipd: float):
    """A side-by-side pair in one frame (W even): the left half is perspective(W / 2, H, fovy) from (-ipd / 2, 0, 0),
    the right half the same map from (+ipd / 2, 0, 0)."""
    W, H = _size(W, H)
    if W % 2:
        raise BhError(_abi.BH_ERR_INVALID_ARG, f"raymap: a side-by-side pair needs an even width, got {W}")
    h = 0.5 * _length(ipd, "ipd", zero_ok=True)
    half = perspective(W // 2, H, fovy)
    o = np.zeros((H, W, 3), np.float64)
    o[:, :W // 2, 0], o[:, W // 2:, 0] = -h, h
    return np.ascontiguousarray(np.concatenate([half, half], 1)), np.ascontiguousarray(o, np.float32)


__all__ = ["FACES", "basis", "pinhole", "perspective", "equirect", "fisheye", "cube_face", "pose", "pose_of",
           "pose_rows", "apply_pose", "apply_origins", "thin_lens", "ods", "orthographic", "stereo"]
