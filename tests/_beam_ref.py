"""Reference of the arrival maps and the beamed disc shade (bh_march_lens_arrivals, bh_march_lens_rays_posed_arrivals,
bh_shade_lens_disc_beamed) for tests/test_beam_host.py and tests/test_gpu_beam.py.  Never the GPU's own output, and not
csrc/bh_lens.hpp either:

  views       tests/_disc_ref.py's (records, fate, hits) and the arrival: the CPU oracle's trace_ray once more for the
              rays whose fate is SURFACE, its final rd (the direction of the state whose ro is the hit), +0 elsewhere;
  factor_np   a numpy restatement of steps 6 to 8 of "Beamed disc shades" as include/bh_render.h words them;
  shade_np    that factor over tests/_disc_ref.shade_np's colours, the blackout test on the product;
  shade_ss    tests/_ss_ref.resolve_np over the per-record colours.

Every view is traced once per process and shared read-only."""
import functools

import numpy as np

import black_hole_ray_marching_amd as bh
import oracle
from oracle import oracle_np
from tests import _disc_ref as dref
from tests._cases import uniforms
from tests._rays_pose_ref import apply_np
from tests._rays_ref import normalise
from tests._ss_ref import resolve_np, sky_ss

f32 = np.float32
RS = dref.RS
DP = f32(bh.Uniforms.default().distortion_power)
FRAMES, FLAG_SETS = dref.FRAMES, dref.FLAG_SETS


def _arrivals(pos, dirs, cap, flags, fate):
    """(N, 3): trace_ray's final rd of the rays (pos, dirs[i]) whose fate is SURFACE, +0 for the others"""
    U = bytes(uniforms().to_c())
    arr = np.zeros((len(dirs), 3), f32)
    for i in np.flatnonzero(fate.reshape(-1) == bh.BH_FATE_SURFACE):
        _, _, f, _, rd = oracle.trace_ray(pos, dirs[i], U, sky_ss(), cap, flags)
        assert f == bh.BH_FATE_SURFACE
        arr[i] = rd
    return arr


def _pinhole_rays(cam, W, H, k):
    raw = np.frombuffer(dref.view_uniform(cam, W, H).to_bytes(), f32)
    return raw[0:3], oracle_np.pixel_dirs(raw[16:28].reshape(3, 4)[:, :3], k * W, k * H)


def _frozen(rec, fate, hits, arr):
    arr = arr.reshape(hits.shape)
    arr.setflags(write=False)
    return rec, fate, hits, arr


@functools.lru_cache(maxsize=None)
def pinhole_view(cam: str, W: int, H: int, cap: int, flags: int = 3, k: int = 1):
    """(records, fate, hits, arrivals) of the virtual frame kW x kH: what bh_march_lens_arrivals must write."""
    rec, fate, hits = dref.pinhole_view(cam, W, H, cap, flags, k)
    pos, dirs = _pinhole_rays(cam, W, H, k)
    return _frozen(rec, fate, hits, _arrivals(pos, dirs, cap, flags, fate))


@functools.lru_cache(maxsize=None)
def posed_view(cam: str, kind: str, W: int, H: int, cap: int, flags: int = 3):
    """(records, fate, hits, arrivals) of the posed ray map: what bh_march_lens_rays_posed_arrivals must write."""
    rec, fate, hits = dref.posed_view(cam, kind, W, H, cap, flags)
    p = dref.pose_rows(cam, kind)
    dirs = normalise(apply_np(p, dref.ray_map(cam, kind, W, H))).reshape(-1, 3)
    return _frozen(rec, fate, hits, _arrivals(p[0], dirs, cap, flags, fate))


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def factor_np(hits, arr, *, rs=RS, dp=DP, beam=1.0, sense=1, parts=False):
    """(f, g) fp32 per record, as if each were a disc hit: steps 6 to 8 of the rule up to the factor; parts: and
    (E2, q, den)."""
    hits, arr = np.asarray(hits, f32), np.asarray(arr, f32)
    rs, dp, beam, sense = f32(rs), f32(dp), f32(beam), f32(sense)
    one, inf = f32(1), f32(np.inf)
    with np.errstate(all="ignore"):
        p = [hits[..., c] for c in range(3)]
        d = [arr[..., c] for c in range(3)]
        x, y, z = p
        r2 = dot(p, p)                                                      # 6.
        r = np.sqrt(r2)
        L = [y * d[2] - z * d[1], z * d[0] - x * d[2], x * d[1] - y * d[0]]
        h2 = dot(L, L)
        E2 = dot(d, d) - ((dp * rs) * h2) / (r2 * r)
        E = np.sqrt(E2)
        rho = np.sqrt(x * x + z * z)                                        # 7.
        om = np.sqrt((f32(0.5) * rs) / ((rho * rho) * rho))
        q = one - (f32(1.5) * rs) / rho
        den = one - (sense * om) * (L[1] / E)
        g = np.sqrt(q) / den
        g = np.where((E2 > 0) & (q > 0) & (den > 0) & (g < inf), g, one)
        ge = one + beam * (g - one)                                         # 8.
        f = (ge * ge) * (ge * ge)
    assert f.dtype == f32 and g.dtype == f32
    return (f, g, E2, q, den) if parts else (f, g)


def disc_mask(rec, hits, *, rs=RS, flags=3):
    """the records that reach step 5: surface records of a scene with the disc whose hit has sd < 0.001"""
    surf = np.asarray(rec, f32)[..., 0] == f32(bh.BH_LENS_SURFACE)
    return surf & bool(flags & bh.BH_SCENE_DISC) & dref.on_disc(hits, rs)


def shade_np(rec, hits, arr, sky_arr, disc_arr, *, rs=RS, flags=3, spin=0.0, gain=1.0, dp=DP, beam=1.0, sense=1):
    """(col, blackout_col) fp32 (..., 4) per record: include/bh_render.h's rule."""
    col = dref.shade_np(rec, hits, sky_arr, disc_arr, rs=rs, flags=flags, spin=spin, gain=gain)[0][..., :3].copy()
    f = factor_np(hits, arr, rs=rs, dp=dp, beam=beam, sense=sense)[0]
    on = disc_mask(rec, hits, rs=rs, flags=flags)
    with np.errstate(all="ignore"):
        for ch in range(3):
            col[..., ch] = np.where(on, col[..., ch] * f, col[..., ch])
        keep = ~(((col[..., 0] * col[..., 0] + col[..., 1] * col[..., 1]) + col[..., 2] * col[..., 2]) < f32(1))
    one = np.ones(col.shape[:-1] + (1,), f32)
    bo = np.where(keep[..., None], col, f32(0))
    return np.concatenate([col, one], -1), np.concatenate([bo, one], -1)


def shade_ss(rec, hits, arr, sky_arr, disc_arr, k: int, **kw):
    col, bo = shade_np(rec, hits, arr, sky_arr, disc_arr, **kw)
    return (col, bo) if k == 1 else (resolve_np(col, k), resolve_np(bo, k))


def assert_both_sides(view, what: str = "") -> None:
    """From the oracle alone: the frame holds a disc hit with g > 1 (the approaching side) and one with g < 1."""
    rec, _, hits, arr = view
    _, g = factor_np(hits, arr)
    on = disc_mask(rec, hits)
    got = dict(brighter=int((on & (g > 1)).sum()), dimmer=int((on & (g < 1)).sum()))
    assert all(got.values()), f"{what}: the frame lacks a side of the disc: {got}"


def energy_drift(cam: str, W: int, H: int, cap: int) -> float:
    """max |E_hit / E_camera - 1| over the frame's disc hits, in f64: E^2 = |rd|^2 - dp rs |ro x rd|^2 / |ro|^3 of
    the ray as it leaves the camera and of the oracle's final state."""
    rec, _, hits, arr = pinhole_view(cam, W, H, cap)
    pos, dirs = _pinhole_rays(cam, W, H, 1)
    on = disc_mask(rec, hits).reshape(-1)

    def energy(ro, rd):
        ro, rd = np.asarray(ro, np.float64), np.asarray(rd, np.float64)
        L = np.cross(ro, rd)
        return np.sqrt((rd * rd).sum(-1) - float(DP) * float(RS) * (L * L).sum(-1) / np.linalg.norm(ro, axis=-1) ** 3)

    e0 = energy(np.broadcast_to(pos, dirs.shape)[on], dirs[on])
    e1 = energy(hits.reshape(-1, 3)[on], arr.reshape(-1, 3)[on])
    return float(np.abs(e1 / e0 - 1.0).max())
