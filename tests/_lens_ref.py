"""Reference of the lens maps (bh_render_lens / bh_shade_lens) for tests/test_lens_host.py and
tests/test_gpu_lens.py.  Never the GPU's own output:

  records   the CPU oracle's trace_ray over oracle_np.pixel_dirs, ray by ray: the fate, and for a sky ray the
            fp32 formulas of include/bh_render.h on the ray's final direction (np.arctan2 in float64, rounded
            to fp32);
  frames    oracle.render_rows with the sky in question (and tests/_ss_ref.py's resolve_np for ss > 1);
  shade_np  a numpy restatement of "shading a record" over oracle_np._sample and _pow15, for hand-made records.

Every array is computed once per process and shared read-only."""
import functools

import numpy as np

import black_hole_ray_marching_amd as bh
import oracle
from oracle import oracle_np
from tests._cases import camera_uniform
from tests._ss_ref import CAP, DEFAULT, FLAGS, resolve_np, scenario_uniforms, sky_ss  # noqa: F401  (shared with the tests)

f32 = np.float32
CAMS = ["D", "E", "F2", "H"]       # E: all four fates at both sizes; F2, H: the camera at or inside the unit sphere
SIZES = [(13, 7), (40, 24)]        # partial tiles on both axes; whole and partial tiles
SKIES = ["ctx", "96x40", "1x1"]    # the context's own, a sky of another size, and one texel (every clamp)


@functools.lru_cache(maxsize=None)
def sky(name: str) -> np.ndarray:
    s = {"ctx": sky_ss, "96x40": lambda: bh.synthetic_sky(96, 40, seed=7),
         "1x1": lambda: bh.synthetic_sky(1, 1, seed=3)}[name]()
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def records(cam: str, W: int, H: int, k: int = 1, scenario=DEFAULT):
    """(records (kH, kW, 2) fp32, fate (kH, kW) uint8) of the virtual frame kW x kH with the camera uniform of
    W x H: what bh_render_lens must write."""
    cu, U = camera_uniform(cam, W, H), bytes(scenario_uniforms(scenario).to_c())
    raw = np.frombuffer(cu.to_bytes(), f32)
    pos, tri = raw[0:3], raw[16:28].reshape(3, 4)[:, :3]
    dirs = oracle_np.pixel_dirs(tri, k * W, k * H)
    rec = np.zeros((k * H * k * W, 2), f32)
    fate = np.zeros(k * H * k * W, np.uint8)
    for i, rd0 in enumerate(dirs):
        _, _, f, _, rd = oracle.trace_ray(pos, rd0, U, sky_ss(), scenario[0], scenario[1])
        fate[i] = f
        if f == bh.BH_FATE_BLACKOUT:
            rec[i] = (bh.BH_LENS_BLACKOUT, 0.0)
        elif f == bh.BH_FATE_SURFACE:
            rec[i] = (bh.BH_LENS_SURFACE, 0.0)
        else:
            rd = rd.astype(f32)
            ln = np.sqrt((rd[0] * rd[0] + rd[1] * rd[1]) + rd[2] * rd[2])
            n = rd / ln
            az = f32(np.arctan2(np.float64(n[2]), np.float64(n[0])))
            rec[i] = ((az + oracle_np.ONE_PI) / oracle_np.TWO_PI, f32(1) - (n[1] + f32(1)) * f32(0.5))
    assert rec.dtype == f32
    rec, fate = rec.reshape(k * H, k * W, 2), fate.reshape(k * H, k * W)
    rec.setflags(write=False)
    fate.setflags(write=False)
    return rec, fate


@functools.lru_cache(maxsize=None)
def frame(cam: str, W: int, H: int, sky_name: str, k: int = 1, scenario=DEFAULT):
    """(col, blackout_col) fp32 (H, W, 4) of the view through `sky_name`: the oracle's frame, for k > 1 the
    normative resolve of the oracle's virtual frame."""
    cu, U = camera_uniform(cam, W, H), scenario_uniforms(scenario)
    col, bo, _, _ = oracle.render_rows(cu.to_bytes(), bytes(U.to_c()), sky(sky_name), k * W, k * H, scenario[0], scenario[1])
    assert not np.isnan(col).any() and not np.isnan(bo).any(), "the oracle frame holds a NaN"
    if k > 1:
        col, bo = resolve_np(col, k), resolve_np(bo, k)
    col.setflags(write=False)
    bo.setflags(write=False)
    return col, bo


def shade_np(rec: np.ndarray, sky_arr: np.ndarray):
    """(col, blackout_col) fp32 (..., 4) of records (..., 2): include/bh_render.h's "shading a record" over
    the numpy oracle's sampler."""
    u, v = rec[..., 0].astype(f32), rec[..., 1].astype(f32)
    r, g, b = oracle_np._sample(np.asarray(sky_arr), oracle_np.srgb_lut(), u, v)
    g, b = oracle_np._pow15(g), oracle_np._pow15(b)
    col = np.stack([r, g, b], -1).astype(f32)
    col[u == f32(bh.BH_LENS_BLACKOUT)] = 0.0
    col[u == f32(bh.BH_LENS_SURFACE)] = 1.0
    keep = ~(((col[..., 0] * col[..., 0] + col[..., 1] * col[..., 1]) + col[..., 2] * col[..., 2]) < f32(1))
    one = np.ones(col.shape[:-1] + (1,), f32)
    bo = np.where(keep[..., None], col, f32(0))
    return np.concatenate([col, one], -1), np.concatenate([bo, one], -1)
