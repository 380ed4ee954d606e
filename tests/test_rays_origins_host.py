"""Origin maps, host side (no GPU): bh_ray_origins_apply_host against the numpy restatement of the origin formula
(tests/_rays_origins_ref.ro0_np), bit for bit, over the tests' origin sets under each named pose; the header's identity
and -0 statements; in-place use; the error returns and NULL checks of the three new symbols with bh_last_error's
prefix; the symbols at ABI version 8; the builders raymap.thin_lens, ods, orthographic and stereo; the Python-side
refusals; and, from the reference alone, the fates and radius classes the GPU tests' sets reach."""
import ctypes as C

import numpy as np
import pytest

import black_hole_ray_marching_amd as bh
from black_hole_ray_marching_amd import _abi, raymap, scene as scene_mod
from tests import _rays_origins_ref as oref
from tests import _rays_pose_ref as pref
from tests import _rays_ref as ref

f32 = np.float32
SYMBOLS = ["bh_render_frames_rays_origins", "bh_render_lens_rays_origins", "bh_ray_origins_apply_host"]
BAD = _abi.BH_ERR_INVALID_ARG


def test_abi_has_the_origin_symbols():
    lib = bh.load()
    assert lib.bh_abi_version() == 8 == _abi.ABI_VERSION
    for name in SYMBOLS:
        assert name in _abi.SIGNATURES and hasattr(lib, name), name
    assert len(_abi.SIGNATURES["bh_render_frames_rays_origins"][1]) == len(_abi.SIGNATURES["bh_render_frames_rays"][1]) + 1
    assert len(_abi.SIGNATURES["bh_render_lens_rays_origins"][1]) == len(_abi.SIGNATURES["bh_render_lens_rays_posed"][1]) + 1
    for name in ("apply_origins", "thin_lens", "ods", "orthographic", "stereo"):
        assert name in raymap.__all__ and callable(getattr(raymap, name)), name


# ---- the host helper ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("okind,W,H", [("scatter", 40, 24), ("scatter", 13, 7), ("hand", 40, 24), ("hand", 13, 7),
                                       ("nonfinite", 8, 8), ("scatter", 1, 1)])
@pytest.mark.parametrize("name", oref.NAMED_POSES)
def test_apply_host_is_the_numpy_formula(name, okind, W, H):
    o = oref.origins(okind, W, H)
    p = oref.rows(name)
    got, want = raymap.apply_origins(p, o), oref.ro0_np(p, o)
    assert got.shape == (H, W, 3) and got.dtype == f32 and got.flags.c_contiguous
    assert np.array_equal(ref.canonical_nan(got), ref.canonical_nan(want))
    if okind == "nonfinite":
        for (y, x), v in oref.NONFINITE.items():
            assert np.isfinite(want[y, x]).all() == np.isfinite(np.asarray(v)).all(), (y, x)
        assert np.isfinite(want[0, 0]).all()
    else:
        assert np.isfinite(want).all()


def test_hand_row_radii_under_the_unit_axes():
    """What the hand row is for: ro0 = 0 exactly under the unit axes at D; under the unit axes at H |ro0|^2 exactly 1,
    then in (1, 1.01], then the first fp32 value above fp32(1.01), then above it; magnitudes of 1e-30 and 1e30 and a
    subnormal component -- where normalize_x leaves its cores -- among the origins the kernels normalise."""
    d = oref.world("axesD", "hand", 13, 7)[0]
    assert np.array_equal(d[0].view(np.uint32), np.zeros(3, np.uint32)), "ro0 = +0 exactly"
    h = oref.world("axesH", "hand", 13, 7)[0]
    q = oref.r2_np(h)
    assert q[1] == f32(1.0) and f32(1.0) < q[2] <= oref.R2_OUT
    assert q[3] > oref.R2_OUT and q[3] == np.nextafter(oref.R2_OUT, f32(2)) and q[4] > q[3]
    assert 0 < np.abs(h[5][:2]).max() < 1e-30 and h[5][2] == 0 and q[5] == 0, "dot(ro0, ro0) underflows"
    assert np.isinf(q[6]) and np.isfinite(h[6]).all(), "and overflows"
    assert 0 < abs(h[7][1]) < np.finfo(f32).tiny, "a subnormal component"
    assert h[8][2] == ref.position("H")[2] and 0 < np.abs(h[8][:2]).min(), "1e-30 is lost beside a non-zero component"
    assert np.array_equal(oref.world("axesH", "hand", 13, 7)[0, 11], ref.position("H")), "the zero origin"


@pytest.mark.parametrize("name", oref.NAMED_POSES)
def test_zero_origins_are_the_position(name):
    """The header's identity: an all +0 origin map gives ro0 = pos bit for bit for a finite basis and a position
    without a -0."""
    p = oref.rows(name)
    assert np.isfinite(p).all() and not (np.signbit(p[0]) & (p[0] == 0)).any()
    got = raymap.apply_origins(p, oref.origins("zero", 13, 7))
    assert np.array_equal(got.view(np.uint32), np.broadcast_to(p[0], (7, 13, 3)).view(np.uint32))


def test_negative_zero_position_and_non_finite_basis():
    """... and what it does not promise: a -0 component of pos becomes +0, and 0 * inf makes every origin NaN."""
    z = np.zeros((2, 2, 3), f32)
    p = oref.rows("axesD").copy()
    p[0] = (-0.0, 1.0, -2.0)
    got = raymap.apply_origins(p, z)
    assert (got[..., 0] == 0).all() and not np.signbit(got[..., 0]).any()
    assert np.array_equal(got[..., 1:], np.broadcast_to(p[0, 1:], (2, 2, 2)))
    p = oref.rows("axesD").copy()
    p[1, 0] = np.inf
    got = raymap.apply_origins(p, z)
    assert np.isnan(got[..., 0]).all() and np.array_equal(got[..., 1:], np.broadcast_to(p[0, 1:], (2, 2, 2)))
    assert np.array_equal(ref.canonical_nan(got), ref.canonical_nan(oref.ro0_np(p, z)))


def test_apply_host_error_returns_and_in_place():
    lib = bh.load()
    call = lib.bh_ray_origins_apply_host
    rows = oref.rows("rotH")
    p = _abi.bh_ray_pose.from_buffer_copy(rows.tobytes())
    o = np.array(oref.origins("hand", 13, 7))
    out = np.full((7, 13, 3), 7.0, f32)
    assert call(None, o.ctypes.data, 13, 7, out.ctypes.data) == BAD
    assert lib.bh_last_error().decode().startswith("bh_ray_origins_apply_host")
    assert call(C.byref(p), None, 13, 7, out.ctypes.data) == BAD
    assert call(C.byref(p), o.ctypes.data, 13, 7, None) == BAD
    for W, H in ((0, 7), (13, 0), (65537, 1), (1, 65537)):
        assert call(C.byref(p), o.ctypes.data, W, H, out.ctypes.data) == BAD, (W, H)
    assert (out == 7.0).all(), "a refused call wrote"
    assert call(C.byref(p), o.ctypes.data, 13, 7, out.ctypes.data) == _abi.BH_OK
    want = oref.ro0_np(rows, oref.origins("hand", 13, 7))
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    assert call(C.byref(p), o.ctypes.data, 13, 7, o.ctypes.data) == _abi.BH_OK  # in place
    assert np.array_equal(o.view(np.uint32), want.view(np.uint32))
    for bad_o in (np.ones((8, 8, 4), f32), np.ones((8, 8), f32), np.ones(3, f32)):
        with pytest.raises(bh.BhError) as e:
            raymap.apply_origins(p, bad_o)
        assert e.value.status == BAD
    with pytest.raises(bh.BhError) as e:
        raymap.apply_origins(np.ones((3, 3), f32), np.ones((8, 8, 3), f32))
    assert e.value.status == BAD


def test_library_refusals_that_need_no_device():
    """The NULL and alignment checks come before any device work, and name the function."""
    lib = bh.load()
    p = _abi.bh_ray_pose()
    U, d = _abi.bh_uniforms(), _abi.bh_render_desc()
    frames, lens = lib.bh_render_frames_rays_origins, lib.bh_render_lens_rays_origins
    ctx = 0x1000  # never dereferenced: each call below fails a pointer check first
    for args in ((None, 1, C.byref(p), C.byref(U), C.byref(d), 0x1000, 0x2000, 1, None),
                 (ctx, 1, None, C.byref(U), C.byref(d), 0x1000, 0x2000, 1, None),
                 (ctx, 1, C.byref(p), None, C.byref(d), 0x1000, 0x2000, 1, None),
                 (ctx, 1, C.byref(p), C.byref(U), None, 0x1000, 0x2000, 1, None),
                 (ctx, 1, C.byref(p), C.byref(U), C.byref(d), None, 0x2000, 1, None),
                 (ctx, 1, C.byref(p), C.byref(U), C.byref(d), 0x1002, 0x2000, 1, None),
                 (ctx, 1, C.byref(p), C.byref(U), C.byref(d), 0x1000, None, 1, None),
                 (ctx, 1, C.byref(p), C.byref(U), C.byref(d), 0x1000, 0x2001, 1, None),
                 (ctx, 1, C.byref(p), C.byref(U), C.byref(d), 0x1000, 0x2002, 1, None),
                 (ctx, 1, C.byref(p), C.byref(U), C.byref(d), 0x1000, 0x2003, 1, None)):
        assert frames(*args) == BAD, args
        assert lib.bh_last_error().decode().startswith("bh_render_frames_rays_origins")
    for args in ((None, C.byref(p), C.byref(U), C.byref(d), 0x1000, 0x2000, 0x3000, None),
                 (ctx, None, C.byref(U), C.byref(d), 0x1000, 0x2000, 0x3000, None),
                 (ctx, C.byref(p), C.byref(U), C.byref(d), None, 0x2000, 0x3000, None),
                 (ctx, C.byref(p), C.byref(U), C.byref(d), 0x1000, None, 0x3000, None),
                 (ctx, C.byref(p), C.byref(U), C.byref(d), 0x1000, 0x2002, 0x3000, None),
                 (ctx, C.byref(p), C.byref(U), C.byref(d), 0x1000, 0x2000, None, None),
                 (ctx, C.byref(p), C.byref(U), C.byref(d), 0x1000, 0x2000, 0x3004, None)):
        assert lens(*args) == BAD, args
        assert lib.bh_last_error().decode().startswith("bh_render_lens_rays_origins")


class _Tensor:
    """What scene._check_dirs looks at, without a device."""

    def __init__(self, shape, size=4, floating=True, contiguous=True, cuda=True):
        self.shape, self._size, self._c, self.is_cuda = shape, size, contiguous, cuda
        self.dtype = type("dtype", (), {"is_floating_point": floating, "__repr__": lambda s: "dtype"})()

    def data_ptr(self):
        return 0x1000

    def element_size(self):
        return self._size

    def is_contiguous(self):
        return self._c


def test_python_side_refusals():
    """The checks an origin map gets are the ones `dirs` gets, under its own name; origins without a pose name
    raymap.pose(pos)."""
    chk = scene_mod._check_dirs
    chk(_Tensor((7, 13, 3)), 7, 13, "render_frames_rays", "origins")
    cases = {"None": None, "numpy": np.zeros((7, 13, 3), f32), "shape": _Tensor((7, 13, 4)), "size": _Tensor((14, 26, 3)),
             "half": _Tensor((7, 13, 3), size=2), "int": _Tensor((7, 13, 3), floating=False),
             "strided": _Tensor((7, 13, 3), contiguous=False), "host": _Tensor((7, 13, 3), cuda=False)}
    for what, t in cases.items():
        with pytest.raises(bh.BhError) as e:
            chk(t, 7, 13, "render_frames_rays", "origins")
        assert e.value.status == BAD and str(e.value).startswith("render_frames_rays: origins "), what
        with pytest.raises(bh.BhError) as e:
            chk(t, 7, 13, "render_frames_rays")
        assert e.value.status == BAD and str(e.value).startswith("render_frames_rays: dirs "), what
    s = bh.Scene.__new__(bh.Scene)  # no context: the refusal comes before anything reads one
    t = _Tensor((7, 13, 3))
    with pytest.raises(bh.BhError) as e:
        bh.Scene.render_frames_rays(s, t, [t], poses=None, origins=t, width=13, height=7)
    assert e.value.status == BAD and "raymap.pose(pos)" in str(e.value)


# ---- builders ----------------------------------------------------------------------------------------------------------
def test_thin_lens():
    W, H, k, fovy, A, D = 13, 7, 4, 0.9, 0.05, 12.5
    dirs, org = raymap.thin_lens(W, H, fovy, A, D, k=k, seed=3)
    for a in (dirs, org):
        assert a.shape == (k * H, k * W, 3) and a.dtype == f32 and a.flags.c_contiguous and np.isfinite(a).all()
    d, o = dirs.astype(np.float64), org.astype(np.float64)
    assert (o[..., 2] == 0).all() and (np.hypot(o[..., 0], o[..., 1]) <= A * (1 + 1e-7)).all(), "lens points within the aperture"
    assert np.hypot(o[..., 0], o[..., 1]).max() > 0.8 * A and len(np.unique(org.reshape(-1, 3), axis=0)) == k * k * W * H
    # every sample of a pixel meets the pixel centre's perspective ray on the plane z = focus
    hit = o + d * ((D - o[..., 2]) / d[..., 2])[..., None]
    centre = np.repeat(np.repeat(raymap.perspective(W, H, fovy).astype(np.float64) * D, k, 0), k, 1)
    assert np.abs(hit - centre).max() <= 1e-5 * D
    # the strata: sample (i, j) of a pixel lies in cell (i, j) of the square the concentric map takes to the disc
    lx, ly = o[..., 0] / A, o[..., 1] / A
    rad = np.hypot(lx, ly)
    assert rad.reshape(H, k, W, k).max(axis=(1, 3)).min() > 0.5, "every pixel's samples spread over its lens"
    # aperture 0: perspective, each pixel k x k times, and zero origins
    d0, o0 = raymap.thin_lens(W, H, fovy, 0.0, D, k=k)
    assert np.array_equal(d0.view(np.uint32), np.repeat(np.repeat(raymap.perspective(W, H, fovy), k, 0), k, 1).view(np.uint32))
    assert np.array_equal(o0.view(np.uint32), np.zeros((k * H, k * W, 3), np.uint32))
    d1, o1 = raymap.thin_lens(W, H, fovy, A, D)  # k = 1: one jittered sample per pixel
    assert d1.shape == (H, W, 3) and o1.shape == (H, W, 3)
    again = raymap.thin_lens(W, H, fovy, A, D, k=k, seed=3)
    assert np.array_equal(again[1], org) and not np.array_equal(raymap.thin_lens(W, H, fovy, A, D, k=k, seed=4)[1], org)
    for kw in (dict(k=3), dict(k=0), dict(aperture=-1.0), dict(aperture=np.nan), dict(focus=0.0), dict(focus=np.inf),
               dict(fovy=0.0), dict(fovy=4.0), dict(seed=-1), dict(seed=0.5), dict(W=0), dict(W=20000, k=8)):
        with pytest.raises(bh.BhError) as e:
            raymap.thin_lens(**{**dict(W=W, H=H, fovy=fovy, aperture=A, focus=D), **kw})
        assert e.value.status == BAD, kw


def test_ods():
    W, H, ipd = 40, 24, 0.065
    dl, ol = raymap.ods(W, H, ipd, "left")
    dr, orr = raymap.ods(W, H, ipd, "right")
    eq = raymap.equirect(W, H)
    assert np.array_equal(dl, eq) and np.array_equal(dr, eq)
    for o in (ol, orr):
        assert o.shape == (H, W, 3) and o.dtype == f32 and o.flags.c_contiguous
        assert np.abs(np.linalg.norm(o.astype(np.float64), axis=-1) - ipd / 2).max() <= 1e-7 * ipd
        assert (o[..., 1] == 0).all()
    assert np.array_equal(ol, -orr), "left = -right"
    horiz = eq.astype(np.float64) * (1.0, 0.0, 1.0)
    assert np.abs((horiz * orr).sum(-1)).max() <= 1e-8, "perpendicular to the column's horizontal direction"
    lon = (2.0 * (np.arange(W) + 0.5) / W - 1.0) * np.pi
    want = np.stack([np.cos(lon), np.zeros(W), -np.sin(lon)], -1) * (ipd / 2)
    assert np.array_equal(orr, np.broadcast_to(want.astype(f32), (H, W, 3)))
    assert (raymap.ods(W, H, 0.0, "left")[1] == 0).all()
    for kw in (dict(eye="both"), dict(ipd=-1.0), dict(ipd=np.inf), dict(W=0)):
        with pytest.raises(bh.BhError) as e:
            raymap.ods(**{**dict(W=W, H=H, ipd=ipd, eye="left"), **kw})
        assert e.value.status == BAD, kw


def test_orthographic_and_stereo():
    W, H, hh = 13, 7, 2.5
    d, o = raymap.orthographic(W, H, hh)
    assert d.shape == o.shape == (H, W, 3) and d.dtype == o.dtype == f32
    assert np.array_equal(d, np.broadcast_to(np.array((0, 0, 1), f32), (H, W, 3)))
    sx, sy = (np.arange(W) + 0.5) / W, (np.arange(H) + 0.5) / H
    want = np.stack(np.broadcast_arrays(((2 * sx - 1) * (hh * W / H))[None, :], ((1 - 2 * sy) * hh)[:, None], 0.0), -1)
    assert np.array_equal(o, want.astype(f32))
    for bad in (0.0, -1.0, np.nan, "x"):
        with pytest.raises(bh.BhError) as e:
            raymap.orthographic(W, H, bad)
        assert e.value.status == BAD
    W, ipd, fovy = 26, 0.065, 0.9
    d, o = raymap.stereo(W, H, fovy, ipd)
    assert d.shape == o.shape == (H, W, 3) and d.dtype == o.dtype == f32 and d.flags.c_contiguous
    half = raymap.perspective(W // 2, H, fovy)
    assert np.array_equal(d[:, :W // 2], half) and np.array_equal(d[:, W // 2:], half)
    assert np.array_equal(o[:, :W // 2], np.broadcast_to(np.array((-ipd / 2, 0, 0), f32), (H, W // 2, 3)))
    assert np.array_equal(o[:, W // 2:], np.broadcast_to(np.array((ipd / 2, 0, 0), f32), (H, W // 2, 3)))
    for kw in (dict(W=13), dict(ipd=-0.1), dict(fovy=0.0)):
        with pytest.raises(bh.BhError) as e:
            raymap.stereo(**{**dict(W=W, H=H, fovy=fovy, ipd=ipd), **kw})
        assert e.value.status == BAD, kw


# ---- what the GPU tests' sets hold, from the reference alone --------------------------------------------------------
@pytest.mark.parametrize("W,H", [(13, 7), (40, 24)])
def test_scatter_from_H_reaches_every_fate_and_straddles_the_threshold(W, H):
    """From position H (0, 0, -1.02) the scatter's origins lie inside the unit sphere, between it and |ro0|^2 = 1.01, and
    beyond; some 8 x 8 tile holds origins on both sides of 1.01 -- the wave that must take the general step; and the
    rays reach all four fates."""
    for okind in ("scatter", "hand"):
        assert oref.fates(["axesH"], "general", okind, W, H) == oref.ALL_FATES, okind
        inside, between, outside = oref.r2_classes("axesH", okind, W, H)
        assert inside > 0 and between > 0 and outside > 0, (inside, between, outside)
        assert oref.straddling_tiles("axesH", okind, W, H) >= 1
    assert oref.straddling_tiles("rotH", "scatter", W, H) >= 1


def test_origin_sets_of_the_gpu_tests():
    assert len({tuple(oref.rows(n).ravel().tolist()) for n in oref.sequence(33)}) == 33, "every pose differs"
    for n in (1, 3, 33):
        assert oref.fates(oref.sequence(n), "general", "hand", 13, 7) == oref.ALL_FATES, n
    assert oref.fates(oref.sequence(3), "general", "hand", 40, 24) == oref.ALL_FATES
    # D: every origin outside (the camera-outside step); F2: every origin inside the unit sphere
    assert oref.r2_classes("rotD", "scatter", 40, 24)[:2] == (0, 0)
    assert oref.r2_classes("rotF2", "scatter", 40, 24)[1:] == (0, 0)
    o = oref.origins("scatter", 40, 24)
    assert o.dtype == f32 and np.abs(o).max() <= 0.06 and np.abs(o).max() > 0.059
    want = (0.06 * np.random.default_rng(0).uniform(-1, 1, (24, 40, 3))).astype(f32)
    assert np.array_equal(o, want)
    nf = oref.origins("nonfinite", 8, 8)
    assert np.isnan(nf[1, 2, 0]) and np.isinf(nf[3, 6, 0]) and np.isinf(nf[6, 1, 1:]).all() and nf[7, 7, 0] == f32(1e30)
    assert np.isfinite(nf).sum() == nf.size - 4
