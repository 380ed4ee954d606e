"""Host-side mirror of the reference's render-to-texture interface, over the C ABI.

Reference (jonathandw743/black_hole_ray_marching):
  Camera            src/camera.rs:11-20, 56-112
  CameraUniform     src/uniforms.rs:98-133
  OtherUniforms     src/otheruniforms.rs:105-118, defaults src/scene.rs:89-137
  Scene             src/scene.rs:28-522  (new :53, resize :370, update :444, render :470)

`Scene.render(output, blackout_output=None)` mirrors `Scene::render(encoder, output_view,
blackout_output_view)`: the caller owns the output images (device tensors here, texture views
there); `None` for the blackout target mirrors `Option::None`.  Errors raise `BhError` (the
reference panics on wgpu validation errors).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _abi
from ._abi import (BH_LAYOUT_ROWMAJOR, BH_LAYOUT_TILES, BH_LAYOUT_TILES_RGB, BH_LAYOUT_TILES_RGBM, BH_LAYOUT_TILES_RGBM14, BH_UNPACK_RGBM14, BH_MATH_EXACT, BH_MATH_FAST, BH_OUT_RGBA16F,
                   BH_OUT_RGBA32F, BH_OUT_BGRA8_SRGB, BH_SCENE_DEFAULT, BYTES_PER_PIXEL, BhError, check, load)

MAX_ITERATIONS = 1000  # src/black_hole_maybe.wgsl:85


@dataclass
class Camera:
    """src/camera.rs:11-20."""
    pos: tuple = (0.0, 0.0, -20.0)
    dir: tuple = (0.0, 0.0, 1.0)
    up: tuple = (0.0, 1.0, 0.0)
    aspect: float = 1.0
    fovy: float = float(np.float32(np.pi) * np.float32(0.5))
    znear: float = 0.1
    zfar: float = 100.0

    @classmethod
    def default(cls, width: int, height: int) -> "Camera":
        """The camera of Scene::new (src/scene.rs:68-76)."""
        c = _abi.bh_camera()
        check(load().bh_camera_default(width, height, C.byref(c)), "bh_camera_default")
        return cls._from_c(c)

    @classmethod
    def look_at(cls, pos, target, width: int, height: int) -> "Camera":
        c = _abi.bh_camera()
        check(load().bh_camera_look_at((C.c_float * 3)(*pos), (C.c_float * 3)(*target), width, height,
                                       C.byref(c)), "bh_camera_look_at")
        return cls._from_c(c)

    @classmethod
    def _from_c(cls, c) -> "Camera":
        return cls(tuple(c.pos), tuple(c.dir), tuple(c.up), c.aspect, c.fovy, c.znear, c.zfar)

    def to_c(self) -> _abi.bh_camera:
        return _abi.bh_camera((C.c_float * 3)(*self.pos), (C.c_float * 3)(*self.dir),
                              (C.c_float * 3)(*self.up), self.aspect, self.fovy, self.znear, self.zfar)


class CameraController:
    """CameraController (src/camera.rs:115-366): key state, speeds and cursor -> camera motion.
    `process_key` takes the reference's key names (process_event :186-261); `update_camera` is
    update_camera (:280-366) through the C ABI (glam f32 arithmetic).  Driving it with a scripted key
    sequence gives the camera paths of an offline, multi-frame render (tools/render_path.py)."""

    KEYS = {"W": "forward", "S": "backward", "A": "left", "D": "right", "Space": "up", "F": "down",
            "ArrowUp": "pan_up", "ArrowDown": "pan_down", "ArrowLeft": "pan_left", "ArrowRight": "pan_right",
            "P": "exp_towards_origin", "O": "exp_away_origin"}

    def __init__(self, speed: float = 5.0, pan_speed: float = 0.5) -> None:  # src/scene.rs:78
        self.c = _abi.bh_controller()
        self.c.speed, self.c.pan_speed = speed, pan_speed

    def process_key(self, key: str, pressed: bool) -> bool:
        if key == "Q":
            if pressed:
                self.c.speed = float(np.float32(self.c.speed) / np.float32(1.5))
            return True
        if key == "E":
            if pressed:
                self.c.speed = float(np.float32(self.c.speed) * np.float32(1.5))
            return True
        if key not in self.KEYS:
            return False
        setattr(self.c, self.KEYS[key], 1 if pressed else 0)
        return True

    def process_mouse(self, pressed: bool) -> None:
        self.c.mouse_pressed = 1 if pressed else 0

    def process_cursor(self, x: float, y: float) -> None:
        """CursorMoved: prev <- curr, curr <- (x, y) (as f32)."""
        self.c.prev_cursor[0], self.c.prev_cursor[1] = self.c.curr_cursor[0], self.c.curr_cursor[1]
        self.c.has_prev_cursor = self.c.has_curr_cursor
        self.c.curr_cursor[0], self.c.curr_cursor[1] = float(np.float32(x)), float(np.float32(y))
        self.c.has_curr_cursor = 1

    def update_camera(self, camera: "Camera", dt: float, do_pan: bool = False) -> tuple["Camera", bool]:
        cc = camera.to_c()
        moved = C.c_int(0)
        check(load().bh_controller_update(C.byref(self.c), C.byref(cc), float(np.float32(dt)), int(do_pan),
                                          C.byref(moved)), "bh_controller_update")
        return Camera._from_c(cc), bool(moved.value)


class CameraUniform:
    """src/uniforms.rs:98-133 — the 112-byte WGSL `Camera` uniform."""

    def __init__(self) -> None:
        self.c = _abi.bh_camera_uniform()
        for i, (x, y) in enumerate(((3.0, 1.0), (-1.0, 1.0), (-1.0, -3.0))):  # ::new
            self.c.screen_tri[i][0], self.c.screen_tri[i][1] = x, y

    def update(self, camera: Camera) -> None:
        check(load().bh_camera_uniform_update(C.byref(camera.to_c()), C.byref(self.c)),
              "bh_camera_uniform_update")

    @property
    def pos(self) -> np.ndarray:
        return np.array(self.c.pos, dtype=np.float32)

    @property
    def world_tri(self) -> np.ndarray:
        return np.array([[self.c.world_tri[i][k] for k in range(3)] for i in range(3)], dtype=np.float32)

    def to_bytes(self) -> bytes:
        return bytes(self.c)


@dataclass
class Uniforms:
    """The 32-byte WGSL `Uniforms` block (src/black_hole_maybe.wgsl:58-69) with Scene::new defaults."""
    rs: float = 1.0
    delta_time_mult: float = 0.5
    bg_brightness: float = 0.5
    blackout_eh: int = 1   # PodBool::r#false() stores inner = 1 (src/podbool.rs:24-26) => on
    max_dist: float = 250.0
    distortion_power: float = 1.0

    @classmethod
    def default(cls) -> "Uniforms":
        u = _abi.bh_uniforms()
        check(load().bh_uniforms_default(C.byref(u)), "bh_uniforms_default")
        return cls(u.rs, u.delta_time_mult, u.bg_brightness, u.blackout_eh, u.max_dist, u.distortion_power)

    def to_c(self) -> _abi.bh_uniforms:
        return _abi.bh_uniforms(self.rs, self.delta_time_mult, self.bg_brightness, int(self.blackout_eh),
                                self.max_dist, self.distortion_power)

    def as_dict(self) -> dict:
        return dict(rs=self.rs, delta_time_mult=self.delta_time_mult, blackout_eh=self.blackout_eh,
                    max_dist=self.max_dist, distortion_power=self.distortion_power)


def synthetic_sky(width: int = 4096, height: int = 2048, seed: int = 0x5EED_B1AC_401E) -> np.ndarray:
    """Deterministic RGBA8 sRGB equirectangular sky, (height, width, 4) uint8."""
    out = np.empty((height, width, 4), dtype=np.uint8)
    check(load().bh_synthetic_sky(out.ctypes.data, width, height, seed), "bh_synthetic_sky")
    return out


def load_sky(path) -> np.ndarray:
    """Texture::from_bytes / from_image (src/texture.rs:11-27, src/scene.rs:186-194): decode an image
    file (the reference ships src/space_4096x2048.jpg) to (H, W, 4) RGBA8 with alpha 255, the bytes
    bh_create uploads as the Rgba8UnormSrgb sky.  Decoded with Pillow (libjpeg-turbo); the reference
    uses the jpeg-decoder crate 0.3.1, and JPEG decoders legitimately differ by +-1 LSB, so the
    texels -- an input to both renderers -- are not part of kernel parity."""
    from PIL import Image
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGBA"), dtype=np.uint8))


def srgb_encode_table() -> np.ndarray:
    """The 257 thresholds of the BGRA8 sRGB encoder (bh_srgb.hpp): code(x) = max k with x >= T[k]."""
    out = np.empty(257, np.float32)
    check(load().bh_srgb_encode_table(out.ctypes.data), "bh_srgb_encode_table")
    return out


def first_step_host(camera_uniform: "CameraUniform", uniforms: "Uniforms", scene_flags: int = BH_SCENE_DEFAULT,
                    max_iters: int = 512) -> tuple[bool, np.float32, np.float32, np.float32]:
    """bh_first_step_host: (valid, dt0, Q0, rq0) -- iteration 0 of the march as the host forms it once per frame for
    the exact tile-schedule kernels; an invalid record is (False, 0, 0, 0) and the waves run iteration 0 themselves."""
    dt0, q0, rq0 = C.c_float(), C.c_float(), C.c_float()
    ok = load().bh_first_step_host(C.byref(camera_uniform.c), C.byref(uniforms.to_c()), scene_flags, max_iters,
                                   C.byref(dt0), C.byref(q0), C.byref(rq0))
    return bool(ok), np.float32(dt0.value), np.float32(q0.value), np.float32(rq0.value)


def shard_tile_count(width: int, height: int, shard_index: int, shard_count: int) -> int:
    n = load().bh_shard_tile_count(width, height, shard_index, shard_count)
    if n < 0:
        raise BhError(int(n), "bh_shard_tile_count")
    return int(n)


def bloom_check(width: int, height: int, levels: int = 3, schedule: int = 0) -> list[tuple]:
    """bh_bloom_check (host only, no device): plan bh_bloom's chain for this frame size and check every
    launch's index arithmetic on the host (DESIGN.md §7b "Bound checks"); raises BhError on a violation.
    Returns the chain's launches as (form, ow, oh, tw, th, rx, ry) tuples, in launch order."""
    lib = load()
    n = C.c_uint64()
    buf = C.create_string_buffer(1 << 16)
    check(lib.bh_bloom_check(width, height, levels, schedule, C.byref(n), buf, len(buf)), "bh_bloom_check")
    out = []
    for line in buf.value.decode().splitlines():
        f = line.split()
        out.append((f[0], *map(int, f[1:])))
    return out


def bloom_plan_failures() -> tuple[int, str]:
    """bh_bloom_plan_failures: (plans real bh_bloom calls built whose host check refused them -- each such pass
    ran its general kernel, same bytes, slower -- process-wide, the last refusal's message)."""
    buf = C.create_string_buffer(512)
    n = load().bh_bloom_plan_failures(buf, len(buf))
    return int(n), buf.value.decode()


def _ptr(t) -> int | None:
    if t is None:
        return None
    if isinstance(t, int):
        return t
    return t.data_ptr()


def _ss_arg(ss) -> int:
    """`ss` as the C ABI takes it (a uint32); what is no such integer is refused as the library refuses a bad ss."""
    if isinstance(ss, bool) or not isinstance(ss, (int, np.integer)) or not 0 <= int(ss) <= 0xFFFFFFFF:
        raise BhError(_abi.BH_ERR_INVALID_ARG, f"render: ss must be 1, 2, 4 or 8, got {ss!r}")
    return int(ss)


def ss_resolve_host(samples: np.ndarray, ss: int) -> np.ndarray:
    """bh_ss_resolve_host (host only): the supersampled kernel's lane code over an fp32 RGBA virtual frame
    (ss*H, ss*W, 4) -> its (H, W, 4) resolve."""
    s = np.ascontiguousarray(samples, np.float32)
    k = _ss_arg(ss)
    if s.ndim != 3 or s.shape[2] != 4 or k == 0 or s.shape[0] % k or s.shape[1] % k:
        raise BhError(_abi.BH_ERR_INVALID_ARG, "ss_resolve_host: samples must be (ss*H, ss*W, 4)")
    out = np.empty((s.shape[0] // k, s.shape[1] // k, 4), np.float32)
    check(load().bh_ss_resolve_host(s.ctypes.data, out.shape[1], out.shape[0], k, out.ctypes.data),
          "bh_ss_resolve_host")
    return out


def shutter_resolve_host(samples: np.ndarray, n_sub: int, ss: int = 1) -> np.ndarray:
    """bh_shutter_resolve_host (host only): the shutter kernel's mapping and tree over fp32 RGBA sample frames
    (n_frames * n_sub, ss*H, ss*W, 4), camera after camera -> the (n_frames, H, W, 4) resolve."""
    s = np.ascontiguousarray(samples, np.float32)
    k, n = _ss_arg(ss), _ss_arg(n_sub)
    if s.ndim != 4 or s.shape[3] != 4 or k == 0 or n == 0 or s.shape[0] % n or s.shape[1] % k or s.shape[2] % k:
        raise BhError(_abi.BH_ERR_INVALID_ARG, "shutter_resolve_host: samples must be (n_frames*n_sub, ss*H, ss*W, 4)")
    out = np.empty((s.shape[0] // n, s.shape[1] // k, s.shape[2] // k, 4), np.float32)
    check(load().bh_shutter_resolve_host(s.ctypes.data, out.shape[0], n, out.shape[2], out.shape[1], k,
                                         out.ctypes.data), "bh_shutter_resolve_host")
    return out


def lens_shade_host(lens: np.ndarray, sky: np.ndarray, ss: int = 1, mip: bool = False):
    """bh_lens_shade_host (host only): what the lens shade kernel runs, on the CPU.  `lens`: (ss*H, ss*W, 2)
    float32 records (u, v); `sky`: (h, w, 4) uint8 RGBA8 sRGB -> (col, blackout_col), fp32 (H, W, 4).
    mip=True: bh_lens_shade_mip_host, the filtered shade over the sky's mip chain (ss 1, 2 or 4)."""
    ln = np.ascontiguousarray(lens, np.float32)
    s = np.ascontiguousarray(sky, np.uint8)
    k = _ss_arg(ss)
    if ln.ndim != 3 or ln.shape[2] != 2 or s.ndim != 3 or s.shape[2] != 4:
        raise BhError(_abi.BH_ERR_INVALID_ARG, "lens_shade_host: lens must be (ss*H, ss*W, 2), sky (h, w, 4)")
    if k == 0 or ln.shape[0] % k or ln.shape[1] % k:
        raise BhError(_abi.BH_ERR_INVALID_ARG, "lens_shade_host: the lens sides must be multiples of ss")
    h, w = ln.shape[0] // k, ln.shape[1] // k
    col, bo = np.empty((h, w, 4), np.float32), np.empty((h, w, 4), np.float32)
    name = "bh_lens_shade_mip_host" if mip else "bh_lens_shade_host"
    check(getattr(load(), name)(ln.ctypes.data, w, h, k, s.ctypes.data, s.shape[1], s.shape[0], col.ctypes.data,
                                bo.ctypes.data), name)
    return col, bo


def lens_shade_disc_host(lens: np.ndarray, hits: np.ndarray, sky: np.ndarray, disc: np.ndarray, *, rs: float,
                         scene_flags: int = BH_SCENE_DEFAULT, spin: float = 0.0, gain: float = 1.0, ss: int = 1):
    """bh_lens_shade_disc_host (host only): what the disc shade kernel runs, on the CPU.  `lens`: (ss*H, ss*W, 2)
    float32 records; `hits`: (ss*H, ss*W, 3) float32, the lens's hit map; `sky`: (h, w, 4) and `disc`: (n_r, n_phi, 4)
    uint8 RGBA8 sRGB -> (col, blackout_col), fp32 (H, W, 4)."""
    ln = np.ascontiguousarray(lens, np.float32)
    ht = np.ascontiguousarray(hits, np.float32)
    s = np.ascontiguousarray(sky, np.uint8)
    dc = np.ascontiguousarray(disc, np.uint8)
    k = _ss_arg(ss)
    if ln.ndim != 3 or ln.shape[2] != 2 or ht.shape != ln.shape[:2] + (3,):
        raise BhError(_abi.BH_ERR_INVALID_ARG, "lens_shade_disc_host: lens must be (ss*H, ss*W, 2), hits (ss*H, ss*W, 3)")
    if s.ndim != 3 or s.shape[2] != 4 or dc.ndim != 3 or dc.shape[2] != 4:
        raise BhError(_abi.BH_ERR_INVALID_ARG, "lens_shade_disc_host: sky must be (h, w, 4), disc (n_r, n_phi, 4)")
    if k == 0 or ln.shape[0] % k or ln.shape[1] % k:
        raise BhError(_abi.BH_ERR_INVALID_ARG, "lens_shade_disc_host: the lens sides must be multiples of ss")
    h, w = ln.shape[0] // k, ln.shape[1] // k
    col, bo = np.empty((h, w, 4), np.float32), np.empty((h, w, 4), np.float32)
    check(load().bh_lens_shade_disc_host(ln.ctypes.data, ht.ctypes.data, w, h, k, s.ctypes.data, s.shape[1], s.shape[0],
                                         dc.ctypes.data, dc.shape[1], dc.shape[0], rs, scene_flags, spin, gain,
                                         col.ctypes.data, bo.ctypes.data), "bh_lens_shade_disc_host")
    return col, bo


def lens_shade_disc_beamed_host(lens: np.ndarray, hits: np.ndarray, arrivals: np.ndarray, sky: np.ndarray,
                                disc: np.ndarray, *, rs: float, scene_flags: int = BH_SCENE_DEFAULT, spin: float = 0.0,
                                gain: float = 1.0, ss: int = 1, beam: float = 1.0, sense: int = 1,
                                distortion_power: float = 1.0):
    """bh_lens_shade_disc_beamed_host (host only): what the beamed disc shade kernel runs, on the CPU.
    lens_shade_disc_host's arguments and `arrivals`: (ss*H, ss*W, 3) float32, the lens's arrival map -> (col,
    blackout_col), fp32 (H, W, 4)."""
    ln = np.ascontiguousarray(lens, np.float32)
    ht = np.ascontiguousarray(hits, np.float32)
    ar = np.ascontiguousarray(arrivals, np.float32)
    s = np.ascontiguousarray(sky, np.uint8)
    dc = np.ascontiguousarray(disc, np.uint8)
    k = _ss_arg(ss)
    if ln.ndim != 3 or ln.shape[2] != 2 or ht.shape != ln.shape[:2] + (3,) or ar.shape != ht.shape:
        raise BhError(_abi.BH_ERR_INVALID_ARG, "lens_shade_disc_beamed_host: lens must be (ss*H, ss*W, 2), hits and arrivals (ss*H, ss*W, 3)")
    if s.ndim != 3 or s.shape[2] != 4 or dc.ndim != 3 or dc.shape[2] != 4:
        raise BhError(_abi.BH_ERR_INVALID_ARG, "lens_shade_disc_beamed_host: sky must be (h, w, 4), disc (n_r, n_phi, 4)")
    if k == 0 or ln.shape[0] % k or ln.shape[1] % k:
        raise BhError(_abi.BH_ERR_INVALID_ARG, "lens_shade_disc_beamed_host: the lens sides must be multiples of ss")
    h, w = ln.shape[0] // k, ln.shape[1] // k
    col, bo = np.empty((h, w, 4), np.float32), np.empty((h, w, 4), np.float32)
    check(load().bh_lens_shade_disc_beamed_host(ln.ctypes.data, ht.ctypes.data, w, h, k, s.ctypes.data, s.shape[1],
                                                s.shape[0], dc.ctypes.data, dc.shape[1], dc.shape[0], rs, scene_flags, spin,
                                                gain, col.ctypes.data, bo.ctypes.data, ar.ctypes.data, beam, sense,
                                                distortion_power), "bh_lens_shade_disc_beamed_host")
    return col, bo


def synthetic_disc(n_phi: int = 1024, n_r: int = 128, seed: int = 0x0D15C) -> np.ndarray:
    """A deterministic disc texture for Disc(): (n_r, n_phi, 4) uint8 RGBA8 sRGB.  A radial temperature ramp --
    white-hot and bright at the inner edge (row 0), dim red at the outer edge -- multiplied by seeded azimuthal
    streaks: a sum of a few sinusoids around the disc whose phases drift with the radius, so the streaks shear as a
    Keplerian flow would have left them.  The same (n_phi, n_r, seed) gives the same bytes."""
    if not (1 <= n_phi <= 32768 and 1 <= n_r <= 32768):
        raise ValueError("synthetic_disc: each side must be in 1..32768")
    rng = np.random.Generator(np.random.PCG64(seed))
    r = ((np.arange(n_r, dtype=np.float64) + 0.5) / n_r)[:, None]        # 0 inner .. 1 outer
    phi = ((np.arange(n_phi, dtype=np.float64) + 0.5) / n_phi)[None, :]  # turns
    heat = (1.0 + r) ** -3.0                                             # ~ r^-3 between 3 rs and 6 rs
    streaks = np.zeros((n_r, n_phi))
    for m in (3, 7, 13, 29, 61):
        amp, phase, shear = rng.uniform(0.5, 1.0) / np.sqrt(m), rng.uniform(0.0, 1.0), rng.uniform(0.5, 2.0)
        streaks += amp * np.cos(2.0 * np.pi * (m * phi + phase + shear * m * r))
    lum = heat * (0.65 + 0.35 * streaks / np.abs(streaks).max())
    rgb = np.stack([lum ** 0.45, lum ** 0.9 * (1.0 - 0.35 * r), lum ** 1.6 * (1.0 - 0.7 * r)], axis=2)
    out = np.empty((n_r, n_phi, 4), np.uint8)
    out[..., :3] = np.clip(np.rint(rgb * 255.0), 0, 255).astype(np.uint8)
    out[..., 3] = 255
    return out


def sky_mips_host(sky: np.ndarray, level: int) -> np.ndarray:
    """bh_sky_mips_host (host only): level `level` >= 1 of the mip chain of `sky` ((h, w, 4) uint8 RGBA8 sRGB), by
    the chain kernels' own functions -> float16 (h_l, w_l, 4)."""
    s = np.ascontiguousarray(sky, np.uint8)
    if s.ndim != 3 or s.shape[2] != 4:
        raise BhError(_abi.BH_ERR_INVALID_ARG, "sky_mips_host: sky must be (h, w, 4)")
    lv = _ss_arg(level)
    out = np.empty((max(1, s.shape[0] >> min(lv, 31)), max(1, s.shape[1] >> min(lv, 31)), 4), np.float16)
    check(load().bh_sky_mips_host(s.ctypes.data, s.shape[1], s.shape[0], lv, out.ctypes.data), "bh_sky_mips_host")
    return out


def _adaptive_desc(ss, adaptive, tile_mask, refined_tiles, n_frames: int, width: int, height: int):
    """The bh_adaptive_desc of a render call (adaptive = T, not None); the optional device buffers are size-checked."""
    try:
        t = float(adaptive)
    except (TypeError, ValueError):
        raise BhError(_abi.BH_ERR_INVALID_ARG, f"render: adaptive must be a threshold (a float), got {adaptive!r}")
    a = _abi.bh_adaptive_desc()
    a.ss, a.threshold = _ss_arg(ss), t
    _check_size(tile_mask, n_frames * ((width + 7) // 8) * ((height + 7) // 8), "tile_mask")
    _check_size(refined_tiles, 4 * n_frames, "refined_tiles")
    a.tile_mask, a.refined_tiles = _ptr(tile_mask), _ptr(refined_tiles)
    return a


def refine_mask_host(col: np.ndarray, blackout: np.ndarray | None, fmt: int, threshold: float) -> np.ndarray:
    """bh_refine_mask_host (host only): the adaptive render's detect rule over one frame's stored target(s),
    (H, W, 4) arrays of float32 / float16 / uint8 for RGBA32F / RGBA16F / BGRA8 -> the (tiles_y, tiles_x) mask."""
    dt = {BH_OUT_RGBA32F: np.float32, _abi.BH_OUT_RGBA16F: np.float16, _abi.BH_OUT_BGRA8_SRGB: np.uint8}.get(fmt)
    if dt is None:
        raise BhError(_abi.BH_ERR_INVALID_ARG, f"refine_mask_host: unknown format {fmt!r}")
    c = np.ascontiguousarray(col, dt)
    b = None if blackout is None else np.ascontiguousarray(blackout, dt)
    if c.ndim != 3 or c.shape[2] != 4 or (b is not None and b.shape != c.shape):
        raise BhError(_abi.BH_ERR_INVALID_ARG, "refine_mask_host: targets must be (H, W, 4) and of one shape")
    h, w = c.shape[:2]
    mask = np.empty(((h + 7) // 8, (w + 7) // 8), np.uint8)
    check(load().bh_refine_mask_host(c.ctypes.data, None if b is None else b.ctypes.data, w, h, fmt, float(threshold),
                                     mask.ctypes.data), "bh_refine_mask_host")
    return mask


def refine_cover_host(width: int, height: int, ss: int, tile_mask: np.ndarray) -> np.ndarray:
    """bh_refine_cover_host (host only): the number of stores each output pixel receives from the adaptive
    render's second pass over `tile_mask` ((tiles_y, tiles_x) uint8) -> (height, width) uint8."""
    m = np.ascontiguousarray(tile_mask, np.uint8)
    if m.shape != ((height + 7) // 8, (width + 7) // 8):
        raise BhError(_abi.BH_ERR_INVALID_ARG, "refine_cover_host: tile_mask must be (ceil(H / 8), ceil(W / 8))")
    out = np.empty((height, width), np.uint8)
    check(load().bh_refine_cover_host(width, height, _ss_arg(ss), m.ctypes.data, out.ctypes.data), "bh_refine_cover_host")
    return out


def tile_bytes(layout: int, fmt: int) -> int:
    """Bytes of one 8x8 tile of a BH_LAYOUT_TILES* layout in format `fmt` (bh_tile_bytes)."""
    n = load().bh_tile_bytes(layout, fmt)
    if n < 0:
        raise BhError(int(n), "bh_tile_bytes")
    return int(n)


def _check_size(t, need: int, name: str, what: str = "render") -> None:
    """Host-side bounds check of a caller buffer (tensor-like objects; raw pointers are trusted)."""
    if t is None or isinstance(t, int) or not hasattr(t, "element_size"):
        return
    have = t.numel() * t.element_size()
    if have < need:
        raise BhError(_abi.BH_ERR_INVALID_ARG, f"{what}: {name} holds {have} bytes, needs {need}")
    if hasattr(t, "is_contiguous") and not t.is_contiguous():
        raise BhError(_abi.BH_ERR_INVALID_ARG, f"{what}: {name} must be contiguous")


def _check_dirs(dirs, height: int, width: int, what: str, name: str = "dirs") -> None:
    """A ray map as bh_render_rays takes it: a contiguous float32 device tensor of shape (height, width, 3) (raw
    pointers are trusted).  `name`: the argument checked ("origins": an origin map, the same checks)."""
    if dirs is None:
        raise BhError(_abi.BH_ERR_INVALID_ARG, f"{what}: {name} is required")
    if isinstance(dirs, int):
        return
    if not hasattr(dirs, "data_ptr") or not hasattr(dirs, "is_cuda"):
        raise BhError(_abi.BH_ERR_INVALID_ARG, f"{what}: {name} must be a device tensor (upload a raymap.* array first), "
                                               f"got {type(dirs).__name__}")
    if tuple(dirs.shape) != (height, width, 3):
        raise BhError(_abi.BH_ERR_INVALID_ARG, f"{what}: {name} must be ({height}, {width}, 3), got {tuple(dirs.shape)}")
    if dirs.element_size() != 4 or not dirs.dtype.is_floating_point:
        raise BhError(_abi.BH_ERR_INVALID_ARG, f"{what}: {name} must be float32, got {dirs.dtype}")
    if not dirs.is_contiguous():
        raise BhError(_abi.BH_ERR_INVALID_ARG, f"{what}: {name} must be contiguous")
    if not dirs.is_cuda:
        raise BhError(_abi.BH_ERR_INVALID_ARG, f"{what}: {name} must be in device memory")


def _pos_arg(pos, what: str):
    """The origin of a ray-map render as the C ABI takes it: three floats."""
    try:
        p = [float(v) for v in pos]
    except (TypeError, ValueError):
        p = []
    if len(p) != 3:
        raise BhError(_abi.BH_ERR_INVALID_ARG, f"{what}: pos must be three floats, got {pos!r}")
    return (C.c_float * 3)(*p)


def _poses_arg(poses, n: int, what: str):
    """n poses as the C ABI takes them: each a _abi.bh_ray_pose (raymap.pose, raymap.pose_of) or four rows of three
    floats (pos, r, u, f)."""
    try:
        ps = list(poses)
    except TypeError:
        ps = None
    if ps is None or not 1 <= n <= _abi.BH_MAX_FRAMES or len(ps) != n:
        raise BhError(_abi.BH_ERR_INVALID_ARG, f"{what}: poses must hold one pose per camera (1..{_abi.BH_MAX_FRAMES}), "
                                               f"{n} here")
    out = (_abi.bh_ray_pose * n)()
    for i, p in enumerate(ps):
        if isinstance(p, _abi.bh_ray_pose):
            out[i] = p
            continue
        try:
            rows = np.ascontiguousarray(p, dtype=np.float32)
        except (TypeError, ValueError):
            rows = np.zeros(0, np.float32)
        if rows.shape != (4, 3):
            raise BhError(_abi.BH_ERR_INVALID_ARG, f"{what}: pose {i} must be a raymap.pose or four rows of three floats "
                                                   "(pos, r, u, f)")
        C.memmove(C.byref(out[i]), rows.ctypes.data, 48)
    return out


class FrameBatch:
    """A prepared bh_render_frames call (Scene.prepare_frames): its targets stay referenced, so the
    device pointers in its descriptors stay valid while the batch lives."""

    def __init__(self, scene: "Scene", descs, keep, ss: int = 1, adaptive=None) -> None:
        self.scene, self.descs, self._keep, self.ss = scene, descs, keep, ss
        self.adaptive = adaptive  # a bh_adaptive_desc (bh_render_frames_adaptive), or None
        self.n = len(descs)
        self._cams = (_abi.bh_camera_uniform * self.n)()

    def render(self, n: int | None = None, cameras=None, stream=None) -> None:
        """Render the first `n` frames (default all) with cameras[i] (default: the scene's camera) and
        the scene's current uniforms."""
        n = self.n if n is None else n
        if not 1 <= n <= self.n:
            raise BhError(_abi.BH_ERR_INVALID_ARG, f"FrameBatch.render: 1..{self.n} frames, got {n}")
        sc = self.scene
        if cameras is None:
            cameras = [sc.camera_uniform] * n
        elif len(cameras) != n:
            raise BhError(_abi.BH_ERR_INVALID_ARG, "render_frames: per-frame lists must have one entry per frame")
        for i, c in enumerate(cameras):
            self._cams[i] = c.c
        if self.adaptive is not None:
            check(sc.lib.bh_render_frames_adaptive(sc._ctx, n, self._cams, C.byref(sc.uniforms.to_c()), self.descs,
                                                   C.byref(self.adaptive), _stream_handle(stream)),
                  "bh_render_frames_adaptive")
            return
        if self.ss != 1:
            check(sc.lib.bh_render_frames_ss(sc._ctx, n, self._cams, C.byref(sc.uniforms.to_c()), self.descs,
                                             self.ss, _stream_handle(stream)), "bh_render_frames_ss")
            return
        check(sc.lib.bh_render_frames(sc._ctx, n, self._cams, C.byref(sc.uniforms.to_c()), self.descs,
                                      _stream_handle(stream)), "bh_render_frames")


class Scene:
    """src/scene.rs `Scene`: owns the sky texture (on `device`), camera, uniforms; renders frames."""

    def __init__(self, width: int, height: int, sky: np.ndarray | None = None, device: int = 0,
                 render_blackout: bool = True, max_iters: int = MAX_ITERATIONS,
                 scene_flags: int = BH_SCENE_DEFAULT, math: int = BH_MATH_FAST) -> None:
        self.lib = load()
        self.width, self.height = width, height
        self.render_blackout = render_blackout
        self.max_iters, self.scene_flags, self.math = max_iters, scene_flags, math
        self.camera = Camera.default(width, height)
        self.camera_uniform = CameraUniform()
        self.camera_uniform.update(self.camera)
        self.uniforms = Uniforms.default()
        if sky is None:
            sky = synthetic_sky()
        sky = np.ascontiguousarray(sky, dtype=np.uint8)
        if sky.ndim != 3 or sky.shape[2] != 4:
            raise ValueError("sky must be (H, W, 4) uint8 RGBA (Rgba8UnormSrgb texels)")
        self.sky = sky
        ctx = C.c_void_p()
        check(self.lib.bh_create(sky.ctypes.data, sky.shape[1], sky.shape[0], device, C.byref(ctx)), "bh_create")
        self._ctx = ctx
        self.device = device
        self._skies = []  # the live Sky objects of this scene (closed with it)

    def close(self) -> None:
        for s in list(getattr(self, "_skies", [])):
            s.close()
        if getattr(self, "_ctx", None):
            self.lib.bh_destroy(self._ctx)
            self._ctx = None
        self._clock_acc = None

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:
            pass

    def resize(self, width: int, height: int) -> None:
        """src/scene.rs:370-382: only the aspect changes; corners are re-derived by update()."""
        self.width, self.height = width, height
        self.camera.aspect = float(np.float32(width) / np.float32(height))

    def update(self, camera: Camera | None = None) -> None:
        """src/scene.rs:444-466 (minus the interactive controller): re-derive the camera uniform."""
        if camera is not None:
            self.camera = camera
        self.camera_uniform.update(self.camera)

    def _desc(self, output, blackout_output, fmt, dbg_n_rk, dbg_fate, math, layout, shard_index, shard_count,
              width, height, schedule, dbg_steps, partition=None) -> _abi.bh_render_desc:
        if output is None:
            raise BhError(_abi.BH_ERR_INVALID_ARG, "render: output is required")
        if not self.render_blackout and blackout_output is not None:
            raise BhError(_abi.BH_ERR_INVALID_ARG, "render: scene built without a blackout target")
        d = _abi.bh_render_desc()
        d.width, d.height = width or self.width, height or self.height
        d.max_iters, d.scene_flags = self.max_iters, self.scene_flags
        d.format = fmt
        d.math = self.math if math is None else math
        d.layout, d.shard_index, d.shard_count = layout, shard_index, shard_count
        d.schedule = schedule
        bpp = _abi.BYTES_PER_PIXEL.get(fmt, 0)
        if layout == BH_LAYOUT_ROWMAJOR:
            px = d.width * d.height
            col_bytes = px * bpp
        else:
            if partition is not None:
                if (partition.width, partition.height, partition.shard_count) != (d.width, d.height, shard_count):
                    raise BhError(_abi.BH_ERR_INVALID_ARG, "render: the partition's frame size / shard count differ")
                d.partition = partition.handle
                nt = partition.tile_count(shard_index)
            else:
                nt = shard_tile_count(d.width, d.height, shard_index, shard_count)
            px = nt * 64
            col_bytes = nt * tile_bytes(layout, fmt) if bpp and layout <= BH_LAYOUT_TILES_RGBM14 else px * bpp
        _check_size(output, col_bytes, "output")
        _check_size(blackout_output, col_bytes, "blackout_output")
        _check_size(dbg_n_rk, px * 2, "dbg_n_rk")
        _check_size(dbg_fate, px, "dbg_fate")
        _check_size(dbg_steps, px * 2, "dbg_steps")
        d.out_col, d.out_blackout = _ptr(output), _ptr(blackout_output)
        d.dbg_n_rk, d.dbg_fate, d.dbg_steps = _ptr(dbg_n_rk), _ptr(dbg_fate), _ptr(dbg_steps)
        return d

    def render(self, output, blackout_output=None, *, fmt: int = BH_OUT_RGBA32F, stream=None,
               dbg_n_rk=None, dbg_fate=None, math: int | None = None, layout: int = BH_LAYOUT_ROWMAJOR,
               shard_index: int = 0, shard_count: int = 1, width: int | None = None,
               height: int | None = None, schedule: int = 0, dbg_steps=None, partition=None, ss: int = 1,
               adaptive: float | None = None, tile_mask=None, refined_tiles=None) -> None:
        """Scene::render (src/scene.rs:470-522): one pass writing `col` and optionally `blackout_col`.

        `output`/`blackout_output`: caller-owned device buffers (torch tensors or raw pointers).
        Asynchronous on `stream` (a torch.cuda.Stream, a raw hipStream_t int, or None = current).
        `ss` = k in {1, 2, 4, 8}: k x k rays per pixel, averaged in linear fp32 before the output encode
        (bh_render_ss; width x height stays the output size).
        `adaptive` = T (with ss = k > 1): the plain frame, then only the 8x8 tiles that show an edge above T
        are marched again with k x k rays and overwritten (bh_render_adaptive); `tile_mask` (uint8 device
        buffer, one byte per tile) and `refined_tiles` (one uint32) optionally receive which and how many.
        """
        d = self._desc(output, blackout_output, fmt, dbg_n_rk, dbg_fate, math, layout, shard_index, shard_count,
                       width, height, schedule, dbg_steps, partition)
        if adaptive is not None:
            a = _adaptive_desc(ss, adaptive, tile_mask, refined_tiles, 1, d.width, d.height)
            check(self.lib.bh_render_adaptive(self._ctx, C.byref(self.camera_uniform.c), C.byref(self.uniforms.to_c()),
                                              C.byref(d), C.byref(a), _stream_handle(stream)), "bh_render_adaptive")
            return
        if tile_mask is not None or refined_tiles is not None:
            raise BhError(_abi.BH_ERR_INVALID_ARG, "render: tile_mask and refined_tiles belong to an adaptive render")
        if ss != 1:
            check(self.lib.bh_render_ss(self._ctx, C.byref(self.camera_uniform.c), C.byref(self.uniforms.to_c()),
                                        C.byref(d), _ss_arg(ss), _stream_handle(stream)), "bh_render_ss")
            return
        check(self.lib.bh_render(self._ctx, C.byref(self.camera_uniform.c), C.byref(self.uniforms.to_c()),
                                 C.byref(d), _stream_handle(stream)), "bh_render")

    def render_frames(self, outputs, blackout_outputs=None, *, cameras=None, fmt: int = BH_OUT_RGBA32F, stream=None,
                      dbg_n_rk=None, dbg_fate=None, dbg_steps=None, math: int | None = None,
                      layout: int = BH_LAYOUT_ROWMAJOR, shard_index: int = 0, shard_count: int = 1,
                      width: int | None = None, height: int | None = None, schedule: int = 0,
                      partition=None, ss: int = 1, adaptive: float | None = None, tile_mask=None,
                      refined_tiles=None) -> None:
        """Several frames in one launch (bh_render_frames, up to BH_MAX_FRAMES): frame i renders with
        cameras[i] (CameraUniform; default: this scene's camera for every frame) into outputs[i] /
        blackout_outputs[i]; each frame's result is exactly render()'s (`ss`, `adaptive` as render's;
        `tile_mask` holds n masks frame after frame, `refined_tiles` n counts)."""
        self.prepare_frames(outputs, blackout_outputs, fmt=fmt, dbg_n_rk=dbg_n_rk, dbg_fate=dbg_fate,
                            dbg_steps=dbg_steps, math=math, layout=layout, shard_index=shard_index,
                            shard_count=shard_count, width=width, height=height, schedule=schedule,
                            partition=partition, ss=ss, adaptive=adaptive, tile_mask=tile_mask,
                            refined_tiles=refined_tiles).render(cameras=cameras, stream=stream)

    def prepare_frames(self, outputs, blackout_outputs=None, *, fmt: int = BH_OUT_RGBA32F, dbg_n_rk=None,
                       dbg_fate=None, dbg_steps=None, math: int | None = None, layout: int = BH_LAYOUT_ROWMAJOR,
                       shard_index: int = 0, shard_count: int = 1, width: int | None = None,
                       height: int | None = None, schedule: int = 0, partition=None, ss: int = 1,
                       adaptive: float | None = None, tile_mask=None, refined_tiles=None) -> "FrameBatch":
        """A render_frames call prepared once for targets that are rendered into again and again (an
        offline camera path, the bench): the descriptors are validated and built here, and each
        FrameBatch.render is one bh_render_frames call -- at 256x256 a launch of 32 frames takes ~0.2
        ms on the GPU, less than building 32 descriptors in Python."""
        n = len(outputs)
        if not 1 <= n <= _abi.BH_MAX_FRAMES:
            raise BhError(_abi.BH_ERR_INVALID_ARG, f"render_frames: 1..{_abi.BH_MAX_FRAMES} frames, got {n}")
        per = lambda v: v if v is not None else [None] * n  # noqa: E731
        bos, nrks, fates, steps = per(blackout_outputs), per(dbg_n_rk), per(dbg_fate), per(dbg_steps)
        if not (len(bos) == len(nrks) == len(fates) == len(steps) == n):
            raise BhError(_abi.BH_ERR_INVALID_ARG, "render_frames: per-frame lists must have one entry per frame")
        descs = (_abi.bh_render_desc * n)(*[self._desc(outputs[i], bos[i], fmt, nrks[i], fates[i], math, layout,
                                                       shard_index, shard_count, width, height, schedule, steps[i],
                                                       partition)
                                            for i in range(n)])
        keep = (outputs, blackout_outputs, dbg_n_rk, dbg_fate, dbg_steps, partition, tile_mask, refined_tiles)
        if adaptive is None:
            if tile_mask is not None or refined_tiles is not None:
                raise BhError(_abi.BH_ERR_INVALID_ARG, "render_frames: tile_mask and refined_tiles belong to an adaptive render")
            return FrameBatch(self, descs, keep, _ss_arg(ss))
        a = _adaptive_desc(ss, adaptive, tile_mask, refined_tiles, n, descs[0].width, descs[0].height)
        return FrameBatch(self, descs, keep, _ss_arg(ss), a)

    def render_shutter(self, output, blackout_output=None, *, cameras, fmt: int = BH_OUT_RGBA32F, ss: int = 1,
                       stream=None, schedule: int = 0, math: int | None = None, width: int | None = None,
                       height: int | None = None) -> None:
        """bh_render_shutter: one frame that averages the frames of `cameras` (n in {1, 2, 4, 8, 16}
        CameraUniforms: the sub-frame cameras of its exposure) in linear fp32 before the output encode; `ss` as
        render's.  Uses the scene's uniforms, not its camera."""
        self.render_frames_shutter([output], None if blackout_output is None else [blackout_output], cameras=[cameras],
                                   fmt=fmt, ss=ss, stream=stream, schedule=schedule, math=math, width=width, height=height)

    def render_frames_shutter(self, outputs, blackout_outputs=None, *, cameras, fmt: int = BH_OUT_RGBA32F, ss: int = 1,
                              stream=None, schedule: int = 0, math: int | None = None, width: int | None = None,
                              height: int | None = None) -> None:
        """bh_render_frames_shutter: several shutter frames in one launch; `cameras` is a list of n-lists, one per
        output frame, all of one length n, with len(outputs) * n at most BH_MAX_FRAMES."""
        n = len(outputs)
        if n < 1 or len(cameras) != n or not cameras[0] or any(len(g) != len(cameras[0]) for g in cameras):
            raise BhError(_abi.BH_ERR_INVALID_ARG, "render_frames_shutter: one list of n cameras per output frame")
        n_sub = len(cameras[0])
        if n * n_sub > _abi.BH_MAX_FRAMES:
            raise BhError(_abi.BH_ERR_INVALID_ARG, f"render_frames_shutter: at most {_abi.BH_MAX_FRAMES} cameras per call, got {n * n_sub}")
        bos = blackout_outputs if blackout_outputs is not None else [None] * n
        if len(bos) != n:
            raise BhError(_abi.BH_ERR_INVALID_ARG, "render_frames_shutter: per-frame lists must have one entry per frame")
        descs = (_abi.bh_render_desc * n)(*[self._desc(outputs[i], bos[i], fmt, None, None, math, BH_LAYOUT_ROWMAJOR,
                                                       0, 1, width, height, schedule, None) for i in range(n)])
        cams = (_abi.bh_camera_uniform * (n * n_sub))(*[c.c for g in cameras for c in g])
        check(self.lib.bh_render_frames_shutter(self._ctx, n, n_sub, cams, C.byref(self.uniforms.to_c()), descs,
                                                _ss_arg(ss), _stream_handle(stream)), "bh_render_frames_shutter")

    def render_rays(self, dirs, output, blackout_output=None, *, pos=None, fmt: int = BH_OUT_RGBA32F, ss: int = 1,
                    stream=None, schedule: int = 0, dbg_n_rk=None, dbg_fate=None, width: int | None = None,
                    height: int | None = None) -> None:
        """bh_render_rays: render() -- with ss = k > 1, render(ss=k) -- with the ray of every pixel taken from the
        ray map `dirs`, a contiguous float32 device tensor (ss*height, ss*width, 3) of directions (any length: the
        kernel normalises them; raymap.* builds some), all from the one origin `pos` (default: the scene camera's
        position).  Any projection is a map.  Exact math, whatever the scene's math mode."""
        k = _ss_arg(ss)
        d = self._desc(output, blackout_output, fmt, dbg_n_rk, dbg_fate, BH_MATH_EXACT, BH_LAYOUT_ROWMAJOR, 0, 1,
                       width, height, schedule, None)
        _check_dirs(dirs, d.height * k, d.width * k, "render_rays")
        p = _pos_arg(self.camera_uniform.pos if pos is None else pos, "render_rays")
        check(self.lib.bh_render_rays(self._ctx, p, C.byref(self.uniforms.to_c()), C.byref(d), _ptr(dirs), k,
                                      _stream_handle(stream)), "bh_render_rays")

    def render_frames_rays(self, dirs, outputs, blackout_outputs=None, *, poses, origins=None,
                           fmt: int = BH_OUT_RGBA32F, ss: int = 1, stream=None, schedule: int = 0, dbg_n_rk=None,
                           dbg_fate=None, width: int | None = None, height: int | None = None) -> None:
        """bh_render_frames_rays: render_frames over one ray map in CAMERA space -- frame i is render_rays of the map
        turned by poses[i] (raymap.pose / raymap.pose_of; include/bh_render.h, bh_ray_pose) from its position, into
        outputs[i] / blackout_outputs[i].  `dirs` as render_rays takes it, shared by every frame; up to
        BH_MAX_FRAMES frames; dbg_n_rk / dbg_fate: per-frame lists (ss == 1).
        `origins` (an origin map: a tensor as `dirs`, of its shape, in camera space; raymap.thin_lens, ods,
        orthographic, stereo build pairs): bh_render_frames_rays_origins -- every ray starts at its pose's position
        plus its own turned origin."""
        what = "render_frames_rays"
        k = _ss_arg(ss)
        n = len(outputs)
        if origins is not None and poses is None:
            raise BhError(_abi.BH_ERR_INVALID_ARG, f"{what}: origins are in camera space and need a pose: give "
                                                   "poses=[raymap.pose(pos)] for the unit axes at pos")
        per = lambda v: v if v is not None else [None] * n  # noqa: E731
        bos, nrks, fates = per(blackout_outputs), per(dbg_n_rk), per(dbg_fate)
        if not (len(bos) == len(nrks) == len(fates) == n):
            raise BhError(_abi.BH_ERR_INVALID_ARG, f"{what}: per-frame lists must have one entry per frame")
        ps = _poses_arg(poses, n, what)
        descs = (_abi.bh_render_desc * n)(*[self._desc(outputs[i], bos[i], fmt, nrks[i], fates[i], BH_MATH_EXACT,
                                                       BH_LAYOUT_ROWMAJOR, 0, 1, width, height, schedule, None)
                                            for i in range(n)])
        _check_dirs(dirs, descs[0].height * k, descs[0].width * k, what)
        if origins is not None:
            _check_dirs(origins, descs[0].height * k, descs[0].width * k, what, "origins")
            check(self.lib.bh_render_frames_rays_origins(self._ctx, n, ps, C.byref(self.uniforms.to_c()), descs,
                                                         _ptr(dirs), _ptr(origins), k, _stream_handle(stream)),
                  "bh_render_frames_rays_origins")
            return
        check(self.lib.bh_render_frames_rays(self._ctx, n, ps, C.byref(self.uniforms.to_c()), descs, _ptr(dirs), k,
                                             _stream_handle(stream)), "bh_render_frames_rays")

    def render_shutter_rays(self, dirs, output, blackout_output=None, *, poses, fmt: int = BH_OUT_RGBA32F,
                            ss: int = 1, stream=None, schedule: int = 0, width: int | None = None,
                            height: int | None = None) -> None:
        """bh_render_frames_shutter_rays of one frame: render_shutter over the camera-space map `dirs`, the
        exposure's sub-frame cameras given as `poses` (n in {1, 2, 4, 8, 16})."""
        self.render_frames_shutter_rays(dirs, [output], None if blackout_output is None else [blackout_output],
                                        poses=[poses], fmt=fmt, ss=ss, stream=stream, schedule=schedule, width=width,
                                        height=height)

    def render_frames_shutter_rays(self, dirs, outputs, blackout_outputs=None, *, poses, fmt: int = BH_OUT_RGBA32F,
                                   ss: int = 1, stream=None, schedule: int = 0, width: int | None = None,
                                   height: int | None = None) -> None:
        """bh_render_frames_shutter_rays: several shutter frames over one camera-space map in one launch; `poses` is
        a list of n-lists, one per output frame, all of one length n, with len(outputs) * n at most BH_MAX_FRAMES."""
        what = "render_frames_shutter_rays"
        k = _ss_arg(ss)
        n = len(outputs)
        if n < 1 or len(poses) != n or not len(poses[0]) or any(len(g) != len(poses[0]) for g in poses):
            raise BhError(_abi.BH_ERR_INVALID_ARG, f"{what}: one list of n poses per output frame")
        n_sub = len(poses[0])
        bos = blackout_outputs if blackout_outputs is not None else [None] * n
        if len(bos) != n:
            raise BhError(_abi.BH_ERR_INVALID_ARG, f"{what}: per-frame lists must have one entry per frame")
        ps = _poses_arg([p for g in poses for p in g], n * n_sub, what)
        descs = (_abi.bh_render_desc * n)(*[self._desc(outputs[i], bos[i], fmt, None, None, BH_MATH_EXACT,
                                                       BH_LAYOUT_ROWMAJOR, 0, 1, width, height, schedule, None)
                                            for i in range(n)])
        _check_dirs(dirs, descs[0].height * k, descs[0].width * k, what)
        check(self.lib.bh_render_frames_shutter_rays(self._ctx, n, n_sub, ps, C.byref(self.uniforms.to_c()), descs,
                                                     _ptr(dirs), k, _stream_handle(stream)),
              "bh_render_frames_shutter_rays")

    def render_lens(self, lens, *, width: int | None = None, height: int | None = None, schedule: int = 0,
                    stream=None, dirs=None, pos=None, pose=None, origins=None, hits=None, arrivals=None) -> None:
        """bh_render_lens: march this scene's camera once into `lens`, a device buffer of height x width records
        (u, v) of 8 bytes (e.g. a float32 tensor (H, W, 2)) -- the view, without any sky.  Exact math, whatever
        the scene's math mode.  Shade it with shade(), as often and with as many skies as wanted.
        `dirs` (a ray map as render_rays takes it, (height, width, 3)): bh_render_lens_rays, the view of that map
        from `pos` (default: the scene camera's position); with `pose` (raymap.pose) instead of `pos`,
        bh_render_lens_rays_posed: the view of the camera-space map `dirs` turned by that pose; with `origins` (an
        origin map of `dirs`' shape) beside the pose, bh_render_lens_rays_origins.
        `hits` (a float32 device tensor (height, width, 3)): bh_render_lens_hits, or with `dirs` bh_render_lens_rays_posed_hits
        (`pose` defaults to the unit axes at the scene camera's position or at `pos`) -- the march also stores where
        each surface ray ended, for shade(hits=, disc=).  Not with `origins`.
        `arrivals` (beside `hits`, of its shape): bh_march_lens_arrivals or bh_march_lens_rays_posed_arrivals -- the
        march also stores the direction each surface ray ended with, for shade(arrivals=)."""
        d = _abi.bh_render_desc()
        d.width, d.height = width or self.width, height or self.height
        d.max_iters, d.scene_flags = self.max_iters, self.scene_flags
        d.math, d.layout, d.shard_count, d.schedule = BH_MATH_EXACT, BH_LAYOUT_ROWMAJOR, 1, schedule
        if lens is None:
            raise BhError(_abi.BH_ERR_INVALID_ARG, "render_lens: lens is required")
        _check_size(lens, d.width * d.height * 8, "lens", "render_lens")
        if arrivals is not None:
            if hits is None:
                raise BhError(_abi.BH_ERR_INVALID_ARG, "render_lens: an arrival map goes with a hit map (give hits)")
            _check_dirs(arrivals, d.height, d.width, "render_lens", "arrivals")
        arr = () if arrivals is None else (_ptr(arrivals),)
        if hits is not None:
            if origins is not None:
                raise BhError(_abi.BH_ERR_INVALID_ARG, "render_lens: a hit map is not built with an origin map")
            _check_dirs(hits, d.height, d.width, "render_lens", "hits")
            if dirs is None:
                if pos is not None or pose is not None:
                    raise BhError(_abi.BH_ERR_INVALID_ARG, "render_lens: pos and pose belong to a ray-map render (give dirs)")
                name = "bh_march_lens_arrivals" if arr else "bh_render_lens_hits"
                check(getattr(self.lib, name)(self._ctx, C.byref(self.camera_uniform.c), C.byref(self.uniforms.to_c()),
                                              C.byref(d), _ptr(lens), _ptr(hits), *arr, _stream_handle(stream)), name)
                return
            if pose is not None and pos is not None:
                raise BhError(_abi.BH_ERR_INVALID_ARG, "render_lens: give pos or pose, not both (a pose holds its position)")
            _check_dirs(dirs, d.height, d.width, "render_lens")
            if pose is None:  # a world-space map: the unit axes at the position
                from . import raymap
                pose = raymap.pose(self.camera_uniform.pos if pos is None else pos)
            ps = _poses_arg([pose], 1, "render_lens")
            name = "bh_march_lens_rays_posed_arrivals" if arr else "bh_render_lens_rays_posed_hits"
            check(getattr(self.lib, name)(self._ctx, ps, C.byref(self.uniforms.to_c()), C.byref(d), _ptr(dirs),
                                          _ptr(lens), _ptr(hits), *arr, _stream_handle(stream)), name)
            return
        if origins is not None and pose is None:
            raise BhError(_abi.BH_ERR_INVALID_ARG, "render_lens: origins are in camera space and need a pose: give "
                                                   "pose=raymap.pose(pos) for the unit axes at pos")
        if pose is not None:
            if pos is not None:
                raise BhError(_abi.BH_ERR_INVALID_ARG, "render_lens: give pos or pose, not both (a pose holds its position)")
            _check_dirs(dirs, d.height, d.width, "render_lens")
            ps = _poses_arg([pose], 1, "render_lens")
            if origins is not None:
                _check_dirs(origins, d.height, d.width, "render_lens", "origins")
                check(self.lib.bh_render_lens_rays_origins(self._ctx, ps, C.byref(self.uniforms.to_c()), C.byref(d),
                                                           _ptr(dirs), _ptr(origins), _ptr(lens),
                                                           _stream_handle(stream)), "bh_render_lens_rays_origins")
                return
            check(self.lib.bh_render_lens_rays_posed(self._ctx, ps, C.byref(self.uniforms.to_c()), C.byref(d),
                                                     _ptr(dirs), _ptr(lens), _stream_handle(stream)),
                  "bh_render_lens_rays_posed")
            return
        if dirs is not None:
            _check_dirs(dirs, d.height, d.width, "render_lens")
            p = _pos_arg(self.camera_uniform.pos if pos is None else pos, "render_lens")
            check(self.lib.bh_render_lens_rays(self._ctx, p, C.byref(self.uniforms.to_c()), C.byref(d), _ptr(dirs),
                                               _ptr(lens), _stream_handle(stream)), "bh_render_lens_rays")
            return
        if pos is not None:
            raise BhError(_abi.BH_ERR_INVALID_ARG, "render_lens: pos belongs to a ray-map render (give dirs)")
        check(self.lib.bh_render_lens(self._ctx, C.byref(self.camera_uniform.c), C.byref(self.uniforms.to_c()),
                                      C.byref(d), _ptr(lens), _stream_handle(stream)), "bh_render_lens")

    def shade(self, lens, output, blackout_output=None, *, fmt: int = BH_OUT_RGBA32F, sky: "Sky | None" = None,
              ss: int = 1, width: int | None = None, height: int | None = None, stream=None, mip: bool = False,
              hits=None, disc: "Disc | None" = None, spin: float = 0.0, gain: float = 1.0, rs: float | None = None,
              scene_flags: int | None = None, arrivals=None, beam: float = 1.0, sense: int = 1,
              distortion_power: float | None = None) -> None:
        """bh_shade_lens: `lens` (render_lens of ss*width x ss*height) and a sky -> the bytes render() -- with
        ss > 1, render(ss=ss) -- writes for that view with that sky.  `sky`: a Sky of this scene, or None for the
        scene's own.  Asynchronous on `stream`; allocates nothing (capturable from the first call).
        mip=True: bh_shade_lens_mip, the sky filtered through its mip chain, the level taken from the lens; `sky`
        must be a Sky(..., mips=True), ss 1, 2 or 4.
        hits= and disc= (render_lens(hits=) of the same lens and a Disc of this scene): bh_shade_lens_disc, the surface
        records that lie on the accretion disc coloured from the disc texture, turned by `spin` turns of its inner
        edge (Keplerian: slower further out) and scaled by `gain`; `rs` and `scene_flags` default to the scene's, which
        the lens was marched with.  Not with mip=True.
        arrivals= beside them (render_lens(hits=, arrivals=) of the same lens): bh_shade_lens_disc_beamed, each disc hit's
        colour scaled by g^4 -- g the Doppler and redshift factor of a Keplerian disc turning in `sense` (+1: the way
        a growing `spin` carries the texture), blended in by `beam` in 0 .. 1; `distortion_power` defaults to the
        scene's."""
        k = _ss_arg(ss)
        d = _abi.bh_shade_desc()
        d.width, d.height, d.ss, d.format = width or self.width, height or self.height, k, fmt
        if sky is not None and (sky.scene is not self or not sky.handle):
            raise BhError(_abi.BH_ERR_INVALID_ARG, "shade: sky must be an open Sky of this scene")
        _check_size(lens, d.width * d.height * k * k * 8, "lens", "shade")
        need = d.width * d.height * BYTES_PER_PIXEL.get(fmt, 0)
        _check_size(output, need, "output", "shade")
        _check_size(blackout_output, need, "blackout_output", "shade")
        d.lens, d.sky = _ptr(lens), None if sky is None else sky.handle
        d.out_col, d.out_blackout = _ptr(output), _ptr(blackout_output)
        if arrivals is not None and (hits is None or disc is None):
            raise BhError(_abi.BH_ERR_INVALID_ARG, "shade: a beamed disc shade takes hits=, disc= and arrivals= together")
        if hits is not None or disc is not None:
            if hits is None or disc is None or mip:
                raise BhError(_abi.BH_ERR_INVALID_ARG, "shade: a disc shade takes hits= and disc= together, without mip")
            if disc.scene is not self or not disc.handle:
                raise BhError(_abi.BH_ERR_INVALID_ARG, "shade: disc must be an open Disc of this scene")
            _check_dirs(hits, d.height * k, d.width * k, "shade", "hits")
            dd = _abi.bh_disc_desc()
            dd.hits, dd.disc = _ptr(hits), disc.handle
            dd.rs = self.uniforms.rs if rs is None else rs
            dd.scene_flags = self.scene_flags if scene_flags is None else scene_flags
            dd.spin, dd.gain = spin, gain
            if arrivals is not None:
                _check_dirs(arrivals, d.height * k, d.width * k, "shade", "arrivals")
                if sense not in (1, -1):
                    raise BhError(_abi.BH_ERR_INVALID_ARG, "shade: sense must be +1 or -1")
                bd = _abi.bh_beam_desc()
                bd.arrivals, bd.beam, bd.sense = _ptr(arrivals), beam, sense
                bd.distortion_power = self.uniforms.distortion_power if distortion_power is None else distortion_power
                check(self.lib.bh_shade_lens_disc_beamed(self._ctx, C.byref(d), C.byref(dd), C.byref(bd),
                                                         _stream_handle(stream)), "bh_shade_lens_disc_beamed")
                return
            check(self.lib.bh_shade_lens_disc(self._ctx, C.byref(d), C.byref(dd), _stream_handle(stream)),
                  "bh_shade_lens_disc")
            return
        name = "bh_shade_lens_mip" if mip else "bh_shade_lens"
        check(getattr(self.lib, name)(self._ctx, C.byref(d), _stream_handle(stream)), name)

    def set_clock_probe(self, acc, stride: int = 256) -> None:
        """bh_set_clock_probe: arm (acc = a zeroed device buffer of 128 u64) or disarm (acc = None) the
        shader-clock sampling of this scene's march launches; clock_mhz() reads the result."""
        if acc is not None:
            _check_size(acc, 128 * 8, "acc", "set_clock_probe")
        check(self.lib.bh_set_clock_probe(self._ctx, _ptr(acc), stride), "bh_set_clock_probe")
        # the armed ctx holds acc's raw pointer: keep the tensor alive until disarmed (or close), so the
        # caching allocator cannot hand its memory to another tensor while march launches add into it
        self._clock_acc = acc

    def graph_release(self) -> None:
        """bh_graph_release: unpin the order states and bloom scratch sets that stream captures marked
        (call it after destroying every graph captured from this scene)."""
        check(self.lib.bh_graph_release(self._ctx), "bh_graph_release")

    def bloom(self, col, blackout, out, *, levels: int = 3, schedule: int = 0, width: int | None = None,
              height: int | None = None, stream=None) -> None:
        """Bloom::render (src/bloom.rs:53-71): the Kawase bloom + remix chain over this scene's two
        BGRA8-sRGB targets (render with fmt=BH_OUT_BGRA8_SRGB) into `out` (the surface).  levels=3 is
        the reference's (src/state.rs:125)."""
        if col is None or blackout is None or out is None:
            raise BhError(_abi.BH_ERR_INVALID_ARG, "bloom: col, blackout and out are required")
        need = (width or self.width) * (height or self.height) * 4
        for t, name in ((col, "col"), (blackout, "blackout"), (out, "out")):
            _check_size(t, need, name, "bloom")
        check(self.lib.bh_bloom(self._ctx, _ptr(col), _ptr(blackout), width or self.width, height or self.height,
                                levels, schedule, _ptr(out), _stream_handle(stream)), "bh_bloom")


class Sky:
    """bh_sky (include/bh_render.h): a sky beside the scene's own, for Scene.shade(sky=...).  `array`: (h, w, 4)
    uint8 RGBA8 sRGB texels (synthetic_sky, load_sky).  It belongs to `scene`; Scene.close() closes it.
    mips=True: bh_sky_create_mips, the sky with its mip chain, for Scene.shade(mip=True)."""

    def __init__(self, scene: "Scene", array: np.ndarray, mips: bool = False) -> None:
        a = np.ascontiguousarray(array, dtype=np.uint8)
        if a.ndim != 3 or a.shape[2] != 4:
            raise ValueError("sky must be (H, W, 4) uint8 RGBA (Rgba8UnormSrgb texels)")
        self.scene, self.width, self.height = scene, a.shape[1], a.shape[0]
        h = C.c_void_p()
        name = "bh_sky_create_mips" if mips else "bh_sky_create"
        check(getattr(scene.lib, name)(scene._ctx, a.ctypes.data, a.shape[1], a.shape[0], C.byref(h)), name)
        self.handle = h.value
        scene._skies.append(self)

    @property
    def levels(self) -> int:
        """bh_sky_levels: the levels of the mip chain, level 0 included; 0 for a sky without one."""
        n = C.c_uint32()
        check(self.scene.lib.bh_sky_levels(self.handle, C.byref(n)), "bh_sky_levels")
        return n.value

    def level(self, l: int) -> np.ndarray:
        """bh_sky_read_level: level l >= 1 of the chain, copied from the device -> float16 (h_l, w_l, 4)."""
        w, h = C.c_uint32(), C.c_uint32()
        lv = _ss_arg(l)
        check(self.scene.lib.bh_sky_read_level(self.handle, lv, C.byref(w), C.byref(h), None), "bh_sky_read_level")
        out = np.empty((h.value, w.value, 4), np.float16)
        check(self.scene.lib.bh_sky_read_level(self.handle, lv, C.byref(w), C.byref(h), out.ctypes.data), "bh_sky_read_level")
        return out

    def close(self) -> None:
        """Free the device texels (after the shades that read them have completed).  A no-op when already
        closed, by hand or by Scene.close()."""
        if getattr(self, "handle", None):
            self.scene.lib.bh_sky_destroy(self.handle)
            self.handle = None
            if self in self.scene._skies:
                self.scene._skies.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Disc:
    """bh_disc (include/bh_render.h): a disc texture for Scene.shade(hits=, disc=).  `array`: (n_r, n_phi, 4) uint8
    RGBA8 sRGB texels (synthetic_disc, load_sky of an image): columns run around the disc, rows from its inner edge
    to its outer edge.  It belongs to `scene`; Scene.close() closes it."""

    def __init__(self, scene: "Scene", array: np.ndarray) -> None:
        a = np.ascontiguousarray(array, dtype=np.uint8)
        if a.ndim != 3 or a.shape[2] != 4:
            raise ValueError("disc must be (n_r, n_phi, 4) uint8 RGBA (Rgba8UnormSrgb texels)")
        self.scene, self.n_phi, self.n_r = scene, a.shape[1], a.shape[0]
        h = C.c_void_p()
        check(scene.lib.bh_disc_create(scene._ctx, a.ctypes.data, a.shape[1], a.shape[0], C.byref(h)), "bh_disc_create")
        self.handle = h.value
        scene._skies.append(self)  # closed with the scene, as its skies are

    def close(self) -> None:
        """Free the device texels (after the shades that read them have completed).  A no-op when already
        closed, by hand or by Scene.close()."""
        if getattr(self, "handle", None):
            self.scene.lib.bh_disc_destroy(self.handle)
            self.handle = None
            if self in self.scene._skies:
                self.scene._skies.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Presenter:
    """bh_presenter (include/bh_render.h): the frame the reference app presents per redraw -- State::render
    (src/state.rs:270-286): Scene::render into the two Bgra8UnormSrgb targets, then Bloom::render to the
    surface -- pipelined: a call's frames march while the previous call's are bloomed on a second stream, and
    (march_streams 2) while the previous call's march tail still runs on the other march stream.
    Every surface equals scene.render(..., fmt=BH_OUT_BGRA8_SRGB) + scene.bloom(...) bytes."""

    def __init__(self, scene: "Scene", width: int | None = None, height: int | None = None, *, levels: int = 3,
                 batch: int = 1, bloom_cus: int = 0, depth: int = 0, march_streams: int = 0,
                 max_iters: int | None = None, math: int | None = None) -> None:
        self.scene = scene
        self.width, self.height = width or scene.width, height or scene.height
        self.batch = batch
        d = _abi.bh_presenter_desc(self.width, self.height, max_iters or scene.max_iters, scene.scene_flags,
                                   scene.math if math is None else math, levels, batch, bloom_cus, depth, march_streams)
        h = C.c_void_p()
        check(scene.lib.bh_presenter_create(scene._ctx, C.byref(d), C.byref(h)), "bh_presenter_create")
        self.handle = h
        self._cams = (_abi.bh_camera_uniform * batch)()
        self._outs = (C.c_void_p * batch)()
        self._keep = None

    def present(self, surfaces, cameras=None, stream=None) -> None:
        """Frames cameras[i] (CameraUniform; default: the scene's camera) -> surfaces[i] (width x height BGRA8
        device images), len(surfaces) <= batch; asynchronous on `stream` (the stream then waits for them)."""
        n = len(surfaces)
        if not 1 <= n <= self.batch:
            raise BhError(_abi.BH_ERR_INVALID_ARG, f"present: 1..{self.batch} surfaces, got {n}")
        if cameras is None:
            cameras = [self.scene.camera_uniform] * n
        elif len(cameras) != n:
            raise BhError(_abi.BH_ERR_INVALID_ARG, "present: one camera per surface")
        for i, (c, t) in enumerate(zip(cameras, surfaces)):
            _check_size(t, self.width * self.height * 4, "surface", "present")
            self._cams[i] = c.c
            self._outs[i] = _ptr(t)
        self._keep = surfaces  # referenced until the next call (the stream orders their later users)
        check(self.scene.lib.bh_present_frames(self.handle, n, self._cams, C.byref(self.scene.uniforms.to_c()),
                                               self._outs, _stream_handle(stream)), "bh_present_frames")

    def close(self) -> None:
        if getattr(self, "handle", None):
            self.scene.lib.bh_presenter_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def clock_mhz(acc) -> dict:
    """The shader clock sampled by set_clock_probe: acc (128 u64 as an int64 array) -> per-XCD MHz and
    the clock over all sampled waves (100 MHz * shader ticks / reference ticks)."""
    a = np.asarray(acc, dtype=np.int64).view(np.uint64).reshape(8, 16)
    ticks, ref, waves = a[:, 0].astype(np.float64), a[:, 1].astype(np.float64), a[:, 2].astype(np.int64)
    per = [round(100.0 * t / r, 1) if r > 0 else None for t, r in zip(ticks, ref)]
    tot = float(ref.sum())
    return {"mhz": round(100.0 * float(ticks.sum()) / tot, 1) if tot > 0 else None,
            "per_xcd_mhz": per, "waves": int(waves.sum()),
            "wave_ms": round(tot / 1e5 / max(1, int(waves.sum())), 5)}


def _stream_handle(stream) -> int | None:
    if stream is None:
        try:
            import torch
            if torch.cuda.is_available():
                return torch.cuda.current_stream().cuda_stream
        except ImportError:
            pass
        return None
    if isinstance(stream, int):
        return stream
    return stream.cuda_stream


def _check_unpack(packed, outs, width, height, shard_count, shard_stride_tiles, packed_tile_bytes, out_bpp, what):
    # shard k's tiles start at k * shard_stride_tiles: the last shard's block ends the buffer's use
    last = shard_tile_count(width, height, shard_count - 1, shard_count) if shard_count >= 1 else 0
    _check_size(packed, ((shard_count - 1) * shard_stride_tiles + last) * packed_tile_bytes, "packed", what)
    for t, name in outs:
        _check_size(t, width * height * out_bpp, name, what)


def tiles_unpack(packed, out, width: int, height: int, shard_count: int, shard_stride_tiles: int,
                 bytes_per_pixel: int, stream=None) -> None:
    _check_unpack(packed, [(out, "out")], width, height, shard_count, shard_stride_tiles, 64 * bytes_per_pixel,
                  bytes_per_pixel, "tiles_unpack")
    check(load().bh_tiles_unpack(_ptr(packed), _ptr(out), width, height, shard_count, shard_stride_tiles,
                                 bytes_per_pixel, _stream_handle(stream)), "bh_tiles_unpack")


def tiles_unpack_rgb(packed, out, width: int, height: int, shard_count: int, shard_stride_tiles: int,
                     fmt: int, stream=None, rows_in_flight: int = 0) -> None:
    """bh_tiles_unpack_rgb(_rows): gathered BH_LAYOUT_TILES_RGB shards of format `fmt` -> row-major
    frame; rows_in_flight > 0 throttles it for overlap with a render (include/bh_render.h)."""
    bpp = _abi.BYTES_PER_PIXEL.get(fmt, 0)
    _check_unpack(packed, [(out, "out")], width, height, shard_count, shard_stride_tiles, 48 * bpp, bpp,
                  "tiles_unpack_rgb")
    if rows_in_flight:
        check(load().bh_tiles_unpack_rgb_rows(_ptr(packed), _ptr(out), width, height, shard_count,
                                              shard_stride_tiles, fmt, rows_in_flight, _stream_handle(stream)),
              "bh_tiles_unpack_rgb_rows")
    else:
        check(load().bh_tiles_unpack_rgb(_ptr(packed), _ptr(out), width, height, shard_count, shard_stride_tiles,
                                         fmt, _stream_handle(stream)), "bh_tiles_unpack_rgb")


def _rgbm_format(fmt: int):
    """(bytes per pixel of the unpacked targets, packed layout) of an RGBM unpack format (0 bytes if invalid)."""
    lay = BH_LAYOUT_TILES_RGBM14 if fmt & BH_UNPACK_RGBM14 else BH_LAYOUT_TILES_RGBM
    base = fmt & 0xFF
    ok = fmt & ~(0xFF | BH_UNPACK_RGBM14) == 0 and (lay == BH_LAYOUT_TILES_RGBM or base == BH_OUT_RGBA16F)
    return (_abi.BYTES_PER_PIXEL.get(base, 0) if ok else 0), lay


def tiles_unpack_rgbm(packed, out_col, out_blackout, width: int, height: int, shard_count: int,
                      shard_stride_tiles: int, fmt: int, stream=None, rows_in_flight: int = 0) -> None:
    """bh_tiles_unpack_rgbm: gathered BH_LAYOUT_TILES_RGBM shards -> both Scene::render targets, row-major
    (`out_blackout` None == Option::None).  fmt = BH_OUT_RGBA16F | BH_UNPACK_RGBM14: BH_LAYOUT_TILES_RGBM14
    shards."""
    bpp, lay = _rgbm_format(fmt)
    _check_unpack(packed, [(out_col, "out_col"), (out_blackout, "out_blackout")], width, height, shard_count,
                  shard_stride_tiles, tile_bytes(lay, fmt & 0xFF) if bpp else 0, bpp, "tiles_unpack_rgbm")
    check(load().bh_tiles_unpack_rgbm(_ptr(packed), _ptr(out_col), _ptr(out_blackout), width, height, shard_count,
                                      shard_stride_tiles, fmt, rows_in_flight, _stream_handle(stream)),
          "bh_tiles_unpack_rgbm")


class Partition:
    """bh_partition (include/bh_render.h): a weighted tile partition of a width x height frame over
    shard_count shards -- shard k owns weights[k] of every sum(weights) residues of (tx + 3*ty), each
    shard's packed order row-major over its tiles.  Pass it to Scene.render / render_frames
    (layout BH_LAYOUT_TILES*) and to tiles_unpack_rgbm."""

    def __init__(self, width: int, height: int, weights, device: int = 0) -> None:
        self.width, self.height = width, height
        self.weights = [int(w) for w in weights]
        self.shard_count = len(self.weights)
        w = (C.c_uint32 * self.shard_count)(*self.weights)
        h = C.c_void_p()
        check(load().bh_partition_create(width, height, self.shard_count, w, device, C.byref(h)), "bh_partition_create")
        self.handle = h.value
        self.counts = [self.tile_count(k) for k in range(self.shard_count)]

    def tile_count(self, shard_index: int) -> int:
        n = load().bh_partition_tile_count(self.handle, shard_index)
        if n < 0:
            raise BhError(int(n), "bh_partition_tile_count")
        return int(n)

    def close(self) -> None:
        if getattr(self, "handle", None):
            load().bh_partition_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def partition_map(width: int, height: int, weights):
    """bh_partition_map (host only): (owner, index) per tile t = ty * tiles_x + tx, as numpy arrays."""
    tiles = ((width + 7) // 8) * ((height + 7) // 8)
    owner = np.zeros(tiles, np.uint32)
    index = np.zeros(tiles, np.uint32)
    w = (C.c_uint32 * len(weights))(*[int(x) for x in weights])
    check(load().bh_partition_map(width, height, len(weights), w, owner.ctypes.data, index.ctypes.data),
          "bh_partition_map")
    return owner, index


def tiles_unpack_rgbm_partition(packed, out_col, out_blackout, partition: "Partition", shard_stride_tiles: int,
                                fmt: int, stream=None, rows_in_flight: int = 0) -> None:
    """bh_tiles_unpack_rgbm_partition: gathered BH_LAYOUT_TILES_RGBM shards of `partition` -> both targets
    (fmt with BH_UNPACK_RGBM14: BH_LAYOUT_TILES_RGBM14 shards)."""
    bpp, lay = _rgbm_format(fmt)
    S = partition.shard_count
    _check_size(packed, ((S - 1) * shard_stride_tiles + partition.counts[-1]) * (tile_bytes(lay, fmt & 0xFF)
                                                                                if bpp else 0), "packed",
                "tiles_unpack_rgbm_partition")
    for t, name in ((out_col, "out_col"), (out_blackout, "out_blackout")):
        _check_size(t, partition.width * partition.height * bpp, name, "tiles_unpack_rgbm_partition")
    check(load().bh_tiles_unpack_rgbm_partition(_ptr(packed), _ptr(out_col), _ptr(out_blackout), partition.handle,
                                                shard_stride_tiles, fmt, rows_in_flight, _stream_handle(stream)),
          "bh_tiles_unpack_rgbm_partition")


__all__ = ["Camera", "Sky", "lens_shade_host", "sky_mips_host", "ss_resolve_host", "refine_mask_host", "refine_cover_host", "Partition", "Presenter", "partition_map", "tiles_unpack_rgbm_partition", "CameraController", "CameraUniform", "Uniforms", "Scene", "synthetic_sky", "shard_tile_count", "tiles_unpack",
           "tiles_unpack_rgb", "tiles_unpack_rgbm", "tile_bytes", "BH_LAYOUT_TILES_RGBM", "BH_LAYOUT_TILES_RGBM14",
           "BH_UNPACK_RGBM14",
           "srgb_encode_table", "load_sky", "bloom_plan_failures", "BH_OUT_BGRA8_SRGB",
           "BhError", "MAX_ITERATIONS", "BH_OUT_RGBA32F", "BH_OUT_RGBA16F", "BH_MATH_EXACT", "BH_MATH_FAST",
           "BH_LAYOUT_ROWMAJOR", "BH_LAYOUT_TILES", "BH_LAYOUT_TILES_RGB", "BH_SCENE_DEFAULT", "BYTES_PER_PIXEL"]
