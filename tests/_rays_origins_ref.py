"""Reference of the origin-map renders (bh_render_frames_rays_origins, bh_render_lens_rays_origins) for
tests/test_rays_origins_host.py and tests/test_gpu_rays_origins.py.  Never the GPU's own output: for a camera-space
direction map, an origin map and a pose, ray by ray,

  the origin   the formula of include/bh_render.h ("Origin maps") restated in numpy fp32, every intermediate an
               np.float32 array and one rounding per operation, in the stated association:
               w[c] = (ox r[c] + oy u[c]) + oz f[c],  ro0[c] = pos[c] + w[c];
  the vector   tests/_rays_pose_ref.apply_np of the direction map, normalised as tests/_rays_ref.normalise does;
  the rest     the CPU oracle's trace_ray(ro0, rd0) -- which derives h2 and the photon-sphere centre from ro0 itself --
               then fs_main's blackout rule and the lens formula, as tests/_rays_ref.trace has them for one position;
  ss > 1       tests/_ss_ref.resolve_np over the per-ray colours of the virtual frame's maps.

Poses, maps and origin sets are named, so every trace is computed once per process and shared read-only."""
import functools

import numpy as np

import black_hole_ray_marching_amd as bh
import oracle
from oracle import oracle_np
from tests import _rays_pose_ref as pref
from tests import _rays_ref as ref
from tests._rays_ref import DEFAULT, canonical_nan  # noqa: F401  (shared with the tests)
from tests._ss_ref import resolve_np, scenario_uniforms, sky_ss

f32 = np.float32
ALL_FATES = pref.ALL_FATES
SEED = 0            # the scatter's: default_rng(SEED)
SCATTER = 0.06      # its half-width
R2_OUT = f32(1.01)  # march_slot's camera-outside threshold on |ro0|^2

# the unit axes at position H beside tests/_rays_pose_ref's named poses: the hand row's radii are exact under it
EXTRA = {"axesH": ("H", np.eye(3, dtype=f32))}
NAMED_POSES = ("axesD", "axesH", "rotH", "shearF2", "mirrorD")  # unit axes (twice), rotated, sheared and scaled, mirrored


def rows(name: str) -> np.ndarray:
    """(4, 3) fp32: pos, r, u, f of a pose of this file or of tests/_rays_pose_ref."""
    if name in EXTRA:
        p, b = EXTRA[name]
        return np.concatenate([ref.position(p)[None, :], b]).astype(f32)
    return pref.rows(name)


def sequence(n: int) -> tuple:
    """n distinct pose names: the unit axes at D and at H lead, then tests/_rays_pose_ref's sequence (positions D, H
    and F2 in turn) without its own unit axes."""
    return (("axesD", "axesH") + pref.sequence(n, 1))[:n]


def ro0_np(p: np.ndarray, o: np.ndarray) -> np.ndarray:
    """The origin formula in numpy fp32: pos[c] + ((ox * r[c] + oy * u[c]) + oz * f[c]), each operation rounded once."""
    p, o = np.asarray(p, f32), np.asarray(o, f32)
    pos, r, u, f = p[0], p[1], p[2], p[3]
    ox, oy, oz = o[..., 0], o[..., 1], o[..., 2]
    out = np.empty(o.shape, f32)
    with np.errstate(all="ignore"):
        for c in range(3):
            a = ox * r[c]
            b = oy * u[c]
            ab = a + b
            cc = oz * f[c]
            w = ab + cc
            out[..., c] = pos[c] + w
            assert a.dtype == b.dtype == ab.dtype == cc.dtype == w.dtype == f32
    return out


def r2_np(ro0: np.ndarray) -> np.ndarray:
    """|ro0|^2 as the kernels' dot forms it: (x x + y y) + z z in fp32."""
    with np.errstate(all="ignore"):
        x, y, z = ro0[..., 0], ro0[..., 1], ro0[..., 2]
        out = (x * x + y * y) + z * z
    assert out.dtype == f32
    return out


# ---- the origin sets (camera space) ---------------------------------------------------------------------------------
def _radius_above(r2: float) -> np.float32:
    """The smallest fp32 r >= sqrt(r2) whose fp32 square exceeds fp32(r2) -- or equals it, when r2 is 1."""
    r = f32(np.sqrt(np.float64(f32(r2))))
    if r2 == 1.0:
        return f32(1.0)
    while not f32(r * r) > f32(r2):
        r = np.nextafter(r, f32(np.inf))
    return r


def hand_origins() -> np.ndarray:
    """The hand-made origins of a set's row 0, (13, 3) fp32.  With D and H the positions of tests/_rays_ref:
      0      -D: ro0 = 0 exactly under the unit axes at D (a NaN photon-sphere centre, h2 = 0);
      1..4   (0, 0, -r) - H for r^2 = 1.0 (exactly), 1.005, the first fp32 square above fp32(1.01), 1.02: under the
             unit axes at H both the difference and the sum back are exact, so |ro0|^2 is r * r as fp32 forms it;
      5      -H + 1e-30 (0.3, -0.5, 0): ro0 = (3e-31, -5e-31, 0) there -- dot(ro0, ro0) underflows (normalize_x's
             IEEE fallback);
      6      1e30 (-0.6, 0.2, 0.7): it overflows;
      7      -H + (0.6, 1e-41, -0.8): a subnormal component at radius 1;
      8      1e-30 (0.3, -0.5, 0.8): lost beside every component of a position that is not 0;
      9..12  inside the unit sphere from H, far above the disc, the zero origin, the far side of the hole."""
    D, H = ref.position("D").astype(np.float64), ref.position("H").astype(np.float64)
    o = [-D]
    for r2 in (1.0, 1.005, 1.01, 1.02):
        o.append(np.array((0.0, 0.0, -np.float64(_radius_above(r2)))) - H)
    o += [-H + 1e-30 * np.array((0.3, -0.5, 0.0)), 1e30 * np.array((-0.6, 0.2, 0.7)),
          -H + np.array((0.6, ref.SUBNORMAL, -0.8)), 1e-30 * np.array((0.3, -0.5, 0.8)),
          -H + np.array((0.5, 0.0, 0.0)), np.array((0.0, 3.0, 0.0)), np.zeros(3), -2.0 * H]
    out = np.asarray(o, np.float64).astype(f32)
    assert out.shape == (13, 3) and np.isfinite(out).all()
    return out


NONFINITE = {(1, 2): (np.nan, 0.0, 0.0), (3, 6): (np.inf, 0.0, 0.0), (6, 1): (0.0, -np.inf, np.inf), (7, 7): (1e30, 0.0, 0.0)}


@functools.lru_cache(maxsize=None)
def origins(kind: str, W: int, H: int) -> np.ndarray:
    """(H, W, 3) fp32 by name: "zero" (all +0), "scatter" (0.06 uniform(-1, 1) of default_rng(SEED)), "hand" (the
    scatter with row 0 the hand-made origins, repeated along the row), "nonfinite" (8 x 8: the scatter with four
    origins replaced, NONFINITE: (y, x) -> origin)."""
    if kind == "zero":
        o = np.zeros((H, W, 3), f32)
    else:
        o = (SCATTER * np.random.default_rng(SEED).uniform(-1.0, 1.0, (H, W, 3))).astype(f32)
        if kind == "hand":
            h = hand_origins()
            for x in range(W):
                o[0, x] = h[x % len(h)]
        elif kind == "nonfinite":
            assert (W, H) == (8, 8)
            for (y, x), v in NONFINITE.items():
                o[y, x] = v
        else:
            assert kind == "scatter", kind
    o.setflags(write=False)
    return o


# ---- the trace --------------------------------------------------------------------------------------------------------
def trace(m: np.ndarray, ro0: np.ndarray, scenario=DEFAULT):
    """tests/_rays_ref.trace with an origin per ray: (col, blackout_col (H, W, 4), records (H, W, 2), fate (H, W) uint8,
    n_rk (H, W) uint16) of the world-space map m from the world-space origins ro0."""
    H, W = m.shape[:2]
    assert ro0.shape == m.shape and ro0.dtype == f32
    U = bytes(scenario_uniforms(scenario).to_c())
    dirs = ref.normalise(m).reshape(-1, 3)
    pos = np.ascontiguousarray(ro0, f32).reshape(-1, 3)
    col = np.ones((H * W, 4), f32)
    rec = np.zeros((H * W, 2), f32)
    fate = np.zeros(H * W, np.uint8)
    n_rk = np.zeros(H * W, np.uint16)
    for i, rd0 in enumerate(dirs):
        rgb, n, f, _, rd = oracle.trace_ray(pos[i], rd0, U, sky_ss(), scenario[0], scenario[1])
        col[i, :3], fate[i], n_rk[i] = rgb, f, n
        if f == bh.BH_FATE_BLACKOUT:
            rec[i] = (bh.BH_LENS_BLACKOUT, 0.0)
        elif f == bh.BH_FATE_SURFACE:
            rec[i] = (bh.BH_LENS_SURFACE, 0.0)
        else:
            with np.errstate(all="ignore"):
                rd = rd.astype(f32)
                ln = np.sqrt((rd[0] * rd[0] + rd[1] * rd[1]) + rd[2] * rd[2])
                n3 = rd / ln
                az = f32(np.arctan2(np.float64(n3[2]), np.float64(n3[0])))
                rec[i] = ((az + oracle_np.ONE_PI) / oracle_np.TWO_PI, f32(1) - (n3[1] + f32(1)) * f32(0.5))
    with np.errstate(all="ignore"):
        r, g, b = col[:, 0], col[:, 1], col[:, 2]
        keep = ~(((r * r + g * g) + b * b) < f32(1))
    bo = np.where(keep[:, None], col, np.array([0, 0, 0, 1], f32)).astype(f32)
    out = (col.reshape(H, W, 4), bo.reshape(H, W, 4), rec.reshape(H, W, 2), fate.reshape(H, W), n_rk.reshape(H, W))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def world(name: str, okind: str, W: int, H: int) -> np.ndarray:
    """The world-space origins of a pose over an origin set."""
    out = ro0_np(rows(name), origins(okind, W, H))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def traced(name: str, mkind: str, okind: str, W: int, H: int, scenario=DEFAULT):
    """trace of tests/_rays_pose_ref's camera map `mkind` turned by the pose, from the pose's origins over the origin
    set `okind`: (col, blackout_col, records, fate, n_rk)."""
    p = rows(name)
    return trace(pref.apply_np(p, pref.camera_map(mkind, W, H)), world(name, okind, W, H), scenario)


def frames(names, mkind: str, okind: str, W: int, H: int, k: int = 1):
    """[(col, blackout_col)] fp32 (H, W, 4), one per pose: the maps of the virtual frame kW x kH, resolved."""
    out = []
    for n in names:
        col, bo = traced(n, mkind, okind, k * W, k * H)[:2]
        out.append((col, bo) if k == 1 else (resolve_np(col, k), resolve_np(bo, k)))
    return out


def fates(names, mkind: str, okind: str, W: int, H: int) -> set:
    seen = set()
    for n in names:
        seen |= set(np.unique(traced(n, mkind, okind, W, H)[3]).tolist())
    return seen


def r2_classes(name: str, okind: str, W: int, H: int):
    """Counts of the pose's origins with |ro0|^2 <= 1, in (1, 1.01] and above 1.01 (NaN: none of them)."""
    q = r2_np(world(name, okind, W, H))
    with np.errstate(invalid="ignore"):
        return int((q <= f32(1)).sum()), int(((q > f32(1)) & (q <= R2_OUT)).sum()), int((q > R2_OUT).sum())


def straddling_tiles(name: str, okind: str, W: int, H: int) -> int:
    """8 x 8 tiles that hold origins on both sides of the camera-outside threshold: the waves that must not take the
    camera-outside step."""
    q = r2_np(world(name, okind, W, H))
    n = 0
    for ty in range(0, H, 8):
        for tx in range(0, W, 8):
            with np.errstate(invalid="ignore"):
                out = q[ty:ty + 8, tx:tx + 8] > R2_OUT
            n += bool(out.any() and not out.all())
    return n
