"""Reference of the filtered lens shade (bh_sky_create_mips / bh_shade_lens_mip) for tests/test_lens_mip_host.py
and tests/test_gpu_lens_mip.py: a numpy restatement of "Filtered lens shades" in include/bh_render.h, written from
that text.  Never the GPU's output, and never the library's host mirror:

  mips_np        the chain of a sky, level by level (numpy's float32 -> float16 cast rounds to nearest even);
  level_np       valid, q, L, f and what the census counts, for every record of a lens grid;
  shade_mip_np   (col, blackout_col) of a lens grid: oracle_np._sample / _pow15 for level 0 and the plain path
                 (tests/_lens_ref.shade_np), the same bilinear arithmetic on the float levels above, and
                 tests/_ss_ref.resolve_np for ss > 1;
  hand_grid      the hand-made records: what the oracle's views do not reach.

Every array is computed once per process and shared read-only."""
import functools

import numpy as np

import black_hole_ray_marching_amd as bh
from oracle import oracle_np
from tests._lens_ref import shade_np
from tests._ss_ref import resolve_np

f32 = np.float32
SKIES = ["1x1", "7x5", "96x40", "512x256"]
KS = [1, 2, 4]


@functools.lru_cache(maxsize=None)
def sky(name: str) -> np.ndarray:
    w, h = (int(v) for v in name.split("x"))
    s = bh.synthetic_sky(w, h, seed=7 if name == "96x40" else 3 if name == "1x1" else 11)
    s.setflags(write=False)
    return s


def n_levels_of(w0: int, h0: int) -> int:
    return 1 + int(np.floor(np.log2(max(w0, h0))))


@functools.lru_cache(maxsize=None)
def mips_np(name: str):
    """[None, level 1, level 2, ...]: float16 (h_l, w_l, 4) each"""
    s = sky(name)
    prev = oracle_np.srgb_lut()[s[..., :3]].astype(f32)  # level 0 as fp32 linear values
    out = [None]
    for _ in range(1, n_levels_of(s.shape[1], s.shape[0])):
        hp, wp = prev.shape[:2]
        w, h = max(1, wp >> 1), max(1, hp >> 1)
        i, j = np.arange(w), np.arange(h)
        x0, x1 = np.minimum(2 * i, wp - 1), np.minimum(2 * i + 1, wp - 1)
        y0, y1 = np.minimum(2 * j, hp - 1), np.minimum(2 * j + 1, hp - 1)
        a, b = prev[y0][:, x0], prev[y0][:, x1]
        c, d = prev[y1][:, x0], prev[y1][:, x1]
        val = ((a + b) + (c + d)) * f32(0.25)
        assert val.dtype == f32
        lev = np.concatenate([val.astype(np.float16), np.ones((h, w, 1), np.float16)], -1)
        lev.setflags(write=False)
        out.append(lev)
        prev = lev[..., :3].astype(f32)
    return out


def level_np(rec: np.ndarray, w0: int, h0: int) -> dict:
    """Per record of the grid rec (Hv, Wv, 2): valid, rho2, q, L, f, filtered (valid, q > 0 and a chain of more than
    one level), and for the census seam (a valid pair whose du wrapped) and lone (a valid centre with an existing
    invalid neighbour)."""
    rec = np.asarray(rec, f32)
    u, v = rec[..., 0], rec[..., 1]
    with np.errstate(invalid="ignore"):
        valid = (u >= f32(0)) & (v == v)
    seam = np.zeros(valid.shape, bool)
    lone = np.zeros(valid.shape, bool)

    def axis_f(ax):
        n = rec.shape[ax]
        if n == 1:
            return np.zeros(valid.shape, f32)
        idx = np.arange(n) + 1
        idx[-1] = n - 2
        un, vn, nvalid = np.take(u, idx, ax), np.take(v, idx, ax), np.take(valid, idx, ax)
        with np.errstate(invalid="ignore", over="ignore"):
            du = np.abs(un - u)
            wrap = du > f32(0.5)
            du = np.where(wrap, f32(1) - du, du)
            dv = np.abs(vn - v)
            su, sv = du * f32(w0), dv * f32(h0)
            F = su * su + sv * sv
        seam[...] |= valid & nvalid & wrap
        lone[...] |= valid & ~nvalid
        return np.where(nvalid, F, f32(0)).astype(f32)

    rho2 = np.fmax(axis_f(1), axis_f(0))
    q = np.ascontiguousarray(rho2).view(np.int32) - np.int32(0x3F800000)
    filtered = valid & (q > 0) & (n_levels_of(w0, h0) > 1)
    L = q >> 24
    f = (q & 0xFFFFFF).astype(f32) * f32(2.0 ** -24)
    return dict(valid=valid, rho2=rho2, q=q, L=L, f=f, filtered=filtered, seam=seam, lone=lone)


def _sample_level(lev: np.ndarray, u, v):
    """the bilinear sample of bh_shade_lens on a float level (h, w, 3): its sides, no table"""
    h, w = lev.shape[:2]
    tx = u * f32(w) - f32(0.5)
    ty = v * f32(h) - f32(0.5)
    tx = np.fmin(np.fmax(tx, f32(-1)), f32(w))
    ty = np.fmin(np.fmax(ty, f32(-1)), f32(h))
    fx, fy = np.floor(tx), np.floor(ty)
    a, b = (tx - fx)[..., None], (ty - fy)[..., None]
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    x1, y1 = np.clip(x0 + 1, 0, w - 1), np.clip(y0 + 1, 0, h - 1)
    x0, y0 = np.clip(x0, 0, w - 1), np.clip(y0, 0, h - 1)
    ia, ib = f32(1) - a, f32(1) - b
    top = lev[y0, x0] * ia + lev[y0, x1] * a
    bot = lev[y1, x0] * ia + lev[y1, x1] * a
    out = top * ib + bot * b
    assert out.dtype == f32
    return out


def shade_mip_np(rec: np.ndarray, sky_name: str, k: int = 1):
    """(col, blackout_col) fp32 (H, W, 4) of the lens grid rec (kH, kW, 2) with the sky `sky_name`."""
    rec = np.asarray(rec, f32)
    s = sky(sky_name)
    h0, w0 = s.shape[:2]
    n = n_levels_of(w0, h0)
    col = shade_np(rec, s)[0][..., :3].copy()  # the plain path, every record
    lv = level_np(rec, w0, h0)
    m = lv["filtered"]
    if m.any():
        u, v, L, f = rec[..., 0][m], rec[..., 1][m], lv["L"][m], lv["f"][m][:, None]
        chain = mips_np(sky_name)
        r0, g0, b0 = oracle_np._sample(s, oracle_np.srgb_lut(), u, v)
        S = [np.stack([r0, g0, b0], -1).astype(f32)] + [_sample_level(chain[l][..., :3].astype(f32), u, v) for l in range(1, n)]
        S = np.stack(S)  # (n, records, 3)
        last = L >= n - 1
        lo_i, hi_i = np.minimum(L, n - 1), np.minimum(L + 1, n - 1)
        at = np.arange(len(u))
        c = np.where(last[:, None], S[n - 1], S[lo_i, at] * (f32(1) - f) + S[hi_i, at] * f).astype(f32)
        c[:, 1], c[:, 2] = oracle_np._pow15(c[:, 1]), oracle_np._pow15(c[:, 2])
        col[m] = c
    assert col.dtype == f32
    keep = ~(((col[..., 0] * col[..., 0] + col[..., 1] * col[..., 1]) + col[..., 2] * col[..., 2]) < f32(1))
    one = np.ones(col.shape[:-1] + (1,), f32)
    bo = np.concatenate([np.where(keep[..., None], col, f32(0)), one], -1)
    col = np.concatenate([col, one], -1)
    if k > 1:
        col, bo = resolve_np(col, k), resolve_np(bo, k)
    return col, bo


@functools.lru_cache(maxsize=None)
def shade_mip_ref(cam: str, W: int, H: int, sky_name: str, k: int = 1):
    """shade_mip_np of the oracle's records of a view, shared by the tests that need it"""
    from tests._lens_ref import records
    col, bo = shade_mip_np(records(cam, W, H, k)[0], sky_name, k)
    col.setflags(write=False)
    bo.setflags(write=False)
    return col, bo


@functools.lru_cache(maxsize=None)
def hand_grid(W: int = 70, H: int = 9) -> np.ndarray:
    """Hand-made records (H, W, 2), nine kinds of row repeating down the grid.  70 x 9 is wider than a wave and taller
    than a workgroup's 4 rows.  Row kinds (r % 9), x the column:
      0, 1  equal rows, u = 0.25 + n(x) / 512 with steps n(x+1) - n(x) cycling 0, 1, 2, v = 0.5: with the 512x256 sky
            rho2 is exactly 0 (equal neighbours), 1 (plain) and 4 (L = 1, f = 0);
      2     the seam: u alternating 0.999 and 0.001;
      3     v stepping by 1.0 along x (the last level of the 7x5 sky);
      4     v stepping by 2.0 along x (the last level of every sky here);
      5     NaN u, NaN v, both sentinels and NaN pairs between valid records: each as centre and as neighbour;
      6     valid, smooth -- above a row of invalid records;
      7     invalid records only: sentinels and NaNs;
      8     valid, coarse steps -- when last, its y neighbour is the row above."""
    nan = f32(np.nan)
    x = np.arange(W)
    g = np.zeros((H, W, 2), f32)
    steps = np.cumsum(np.concatenate([[0], (x[:-1] % 3)]))
    kinds = [f32(0.3), nan, f32(0.31), f32(0.32), f32(0.33), f32(bh.BH_LENS_BLACKOUT), f32(0.35), f32(bh.BH_LENS_SURFACE), nan, f32(0.36)]
    vkind = [f32(0.6), f32(0.5), f32(0.61), nan, f32(0.62), f32(0), f32(0.63), f32(0), nan, f32(0.64)]
    for r in range(H):
        t = r % 9
        if t in (0, 1):
            g[r, :, 0], g[r, :, 1] = f32(0.25) + steps.astype(f32) / f32(512), 0.5
        elif t == 2:
            g[r, :, 0], g[r, :, 1] = np.where(x % 2 == 0, f32(0.999), f32(0.001)), 0.4
        elif t == 3:
            g[r, :, 0], g[r, :, 1] = 0.5, (x % 5).astype(f32) - f32(2)
        elif t == 4:
            g[r, :, 0], g[r, :, 1] = 0.37, f32(2) * (x % 3).astype(f32) - f32(1)
        elif t == 5:
            g[r, :, 0], g[r, :, 1] = np.array(kinds, f32)[x % 10], np.array(vkind, f32)[x % 10]
        elif t == 6:
            g[r, :, 0], g[r, :, 1] = f32(0.2) + f32(0.01) * x.astype(f32), 0.7
        elif t == 7:
            g[r, :, 0] = np.array([bh.BH_LENS_BLACKOUT, bh.BH_LENS_SURFACE, np.nan], f32)[x % 3]
            g[r, :, 1] = np.where(x % 3 == 2, nan, f32(0))
        else:
            g[r, :, 0], g[r, :, 1] = f32(0.05) + f32(0.013) * x.astype(f32), f32(0.2) + f32(0.002) * x.astype(f32)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def hand_grids() -> dict:
    """name -> (records, k): the 70 x 9 grid, a 1-wide grid (column 1 of a 70-row grid: every row kind, a NaN and a
    sentinel among them), two 1-high grids (the mixed row and the seam row) and a single record at ss 1; grids of
    140 x 18 and 280 x 36 records for 70 x 9 pixels at ss 2 and 4"""
    out = {"70x9": (hand_grid(), 1), "1x70": (hand_grid(9, 70)[:, 1:2], 1), "70x1": (hand_grid()[5:6], 1),
           "70x1 seam": (hand_grid()[2:3], 1), "1x1": (hand_grid()[:1, :1], 1),
           "70x9 ss2": (hand_grid(140, 18), 2), "70x9 ss4": (hand_grid(280, 36), 4)}
    return {n: (np.ascontiguousarray(g), k) for n, (g, k) in out.items()}
