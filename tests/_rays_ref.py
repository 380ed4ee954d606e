"""Reference of the ray-map renders (bh_render_rays / bh_render_lens_rays) for tests/test_rays_host.py and
tests/test_gpu_rays.py.  Never the GPU's own output: for a map and a position, ray by ray,

  the direction   the map's vector normalised in numpy fp32 as oracle_np.pixel_dirs normalises:
                  d / sqrt((x*x + y*y) + z*z)  (a zero, infinite or NaN vector gives what IEEE gives);
  the colour      the CPU oracle's trace_ray of that direction from the position (cap and flags of tests/_ss_ref.py);
  blackout_col    fs_main's rule on it, dot(col, col) < 1 ? 0 : col (tests/_lens_ref.shade_np's);
  the lens record tests/_lens_ref.records' formula on trace_ray's final direction;
  ss > 1          tests/_ss_ref.resolve_np over the per-ray colours.

The maps the tests render are built here too, by name, so every reference is computed once per process and shared
read-only."""
import functools

import numpy as np

import black_hole_ray_marching_amd as bh
import oracle
from black_hole_ray_marching_amd import raymap
from oracle import oracle_np
from tests._cases import CAMERAS, camera_uniform
from tests._ss_ref import CAP, DEFAULT, FLAGS, resolve_np, scenario_uniforms, sky_ss  # noqa: F401  (shared with the tests)

f32 = np.float32
POSITIONS = ["D", "H", "F2"]       # outside and far; just outside the unit sphere (camera-outside step); inside it
SIZES = [(40, 24), (13, 7)]
E_AIM = (2.6, 0.0, 20.0)           # camera E's aim from its position: the shadow's edge, the photon sphere grazed
SUBNORMAL = float(np.float32(1e-41))


def position(name: str) -> np.ndarray:
    return np.asarray(CAMERAS[name][0], f32)


def hand_rays(name: str) -> np.ndarray:
    """The hand-made rays of a general map's row 0, (16, 3) fp32: the rays no pinhole frame holds, and one (the last)
    that gives the position inside the unit sphere its surface hit."""
    p = position(name).astype(np.float64)
    a = np.cross(p, (0.0, 1.0, 0.0))
    b = np.cross(p, a)
    rays = [-p, p,                                          # exactly radial, inward and outward: ro0 x rd = 0
            a, b, a * 0.25 - b * 3.0,                       # perpendicular to pos
            (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1),
            np.array((0.3, -0.5, 0.8)) * 1e-30,             # normalize_x's IEEE fallback: dot(d, d) underflows
            np.array((-0.6, 0.2, 0.7)) * 1e30,              # ... and overflows
            (0.6, SUBNORMAL, -0.8),                         # ... and one subnormal component
            E_AIM,
            (4.0, -0.08, -4.0)]                             # outward from inside the unit sphere (F2), onto the disc
    out = np.asarray(rays, np.float64).astype(f32)
    assert out.shape == (16, 3) and np.isfinite(out).all()
    return out


@functools.lru_cache(maxsize=None)
def general_map(name: str, W: int, H: int) -> np.ndarray:
    """(H, W, 3) fp32: row 0 the hand-made rays -- all 16, repeated, where the row holds them (W = 40); at W = 13 the
    13 that start at ray 5 * (index of the position), so the three positions cover all 16 -- the other rows
    raymap.equirect: the full sphere around the position, partial tiles on both axes."""
    m = raymap.equirect(W, H).copy()
    h = hand_rays(name)
    first = 0 if W >= len(h) else 5 * POSITIONS.index(name)
    for x in range(W):
        m[0, x] = h[(first + x) % len(h)]
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def equirect_map(W: int, H: int) -> np.ndarray:
    m = raymap.equirect(W, H)
    m.setflags(write=False)
    return m


NONFINITE = {(1, 2): (0.0, 0.0, 0.0), (3, 6): (np.inf, 0.0, 0.0), (6, 1): (np.nan, 1.0, 0.0), (7, 7): (0.0, -np.inf, np.inf)}


@functools.lru_cache(maxsize=None)
def nonfinite_map() -> np.ndarray:
    """8 x 8: the equirect map with four rays replaced (NONFINITE: (y, x) -> vector)."""
    m = raymap.equirect(8, 8).copy()
    for (y, x), v in NONFINITE.items():
        m[y, x] = v
    m.setflags(write=False)
    return m


def normalise(m: np.ndarray) -> np.ndarray:
    d = np.asarray(m, f32)
    with np.errstate(all="ignore"):
        x, y, z = d[..., 0], d[..., 1], d[..., 2]
        ln = np.sqrt((x * x + y * y) + z * z)
        out = d / ln[..., None]
    assert out.dtype == f32
    return out


def trace(m: np.ndarray, pos: np.ndarray, scenario=DEFAULT):
    """(col, blackout_col (H, W, 4), records (H, W, 2), fate (H, W) uint8, n_rk (H, W) uint16) of the map from pos."""
    H, W = m.shape[:2]
    U = bytes(scenario_uniforms(scenario).to_c())
    dirs = normalise(m).reshape(-1, 3)
    col = np.ones((H * W, 4), f32)
    rec = np.zeros((H * W, 2), f32)
    fate = np.zeros(H * W, np.uint8)
    n_rk = np.zeros(H * W, np.uint16)
    for i, rd0 in enumerate(dirs):
        rgb, n, f, _, rd = oracle.trace_ray(pos, rd0, U, sky_ss(), scenario[0], scenario[1])
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
def general(name: str, W: int, H: int, scenario=DEFAULT):
    """trace() of general_map(name, W, H) from the position; in the default scenario the map reaches all four fates
    (asserted here; the fates of the others: tests/test_scenarios_host.py)."""
    out = trace(general_map(name, W, H), position(name), scenario)
    seen = set(np.unique(out[3]).tolist())
    want = {bh.BH_FATE_CAP, bh.BH_FATE_ESCAPE, bh.BH_FATE_SURFACE, bh.BH_FATE_BLACKOUT}
    assert scenario != DEFAULT or seen == want, f"general map {name} {W}x{H}: fates {sorted(seen)}"
    return out


@functools.lru_cache(maxsize=None)
def nonfinite(name: str):
    return trace(nonfinite_map(), position(name))


@functools.lru_cache(maxsize=None)
def equirect_ss(name: str, W: int, H: int, k: int, scenario=DEFAULT):
    """(col, blackout_col) (H, W, 4): ss = k over the virtual frame's equirect map, resolved by the normative tree."""
    col, bo, _, _, _ = trace(equirect_map(k * W, k * H), position(name), scenario)
    assert not np.isnan(col).any() and not np.isnan(bo).any()
    rc, rb = resolve_np(col, k), resolve_np(bo, k)
    rc.setflags(write=False)
    rb.setflags(write=False)
    return rc, rb


@functools.lru_cache(maxsize=None)
def pinhole_map(cam: str, W: int, H: int, k: int = 1) -> np.ndarray:
    """raymap.pinhole of the virtual frame kW x kH with the camera uniform of W x H."""
    m = raymap.pinhole(camera_uniform(cam, W, H), k * W, k * H)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def oracle_dbg(cam: str, W: int, H: int, scenario=DEFAULT):
    """(n_rk (H, W) uint16, fate (H, W) uint8) of the oracle's frame (render_rows)."""
    cu, U = camera_uniform(cam, W, H), scenario_uniforms(scenario)
    _, _, n_rk, fate = oracle.render_rows(cu.to_bytes(), bytes(U.to_c()), sky_ss(), W, H, scenario[0], scenario[1])
    return n_rk.astype(np.uint16), fate.astype(np.uint8)


def canonical_nan(a: np.ndarray) -> np.ndarray:
    """fp32 values as uint32 with every NaN's payload and sign replaced by one pattern."""
    a = np.ascontiguousarray(a, f32)
    u = a.view(np.uint32).copy()
    u[np.isnan(a)] = 0x7FC00000
    return u
