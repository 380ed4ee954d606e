"""Posed ray maps, host side (no GPU): bh_ray_pose_apply_host against the numpy restatement of the pose formula
(tests/_rays_pose_ref.apply_np), bit for bit; its error returns; raymap.pose / pose_of / apply_pose; the Python-side
refusals of Scene.render_frames_rays, render_(frames_)shutter_rays and render_lens(pose=...) that need no device; the
library's NULL checks; the four new symbols at ABI version 8; and the fates the GPU tests' sets reach."""
import ctypes as C

import numpy as np
import pytest

import black_hole_ray_marching_amd as bh
from black_hole_ray_marching_amd import _abi, raymap, scene as scene_mod
from tests import _rays_pose_ref as pref
from tests import _rays_ref as ref

f32 = np.float32
SYMBOLS = ["bh_render_frames_rays", "bh_render_frames_shutter_rays", "bh_render_lens_rays_posed", "bh_ray_pose_apply_host"]


def test_abi_has_the_posed_symbols():
    lib = bh.load()
    assert lib.bh_abi_version() == 8 == _abi.ABI_VERSION
    for name in SYMBOLS:
        assert name in _abi.SIGNATURES and hasattr(lib, name), name
    assert C.sizeof(_abi.bh_ray_pose) == 48
    assert [(_abi.bh_ray_pose.pos.offset, _abi.bh_ray_pose.r.offset, _abi.bh_ray_pose.u.offset, _abi.bh_ray_pose.f.offset)] == [(0, 12, 24, 36)]
    for m in ("render_frames_rays", "render_shutter_rays", "render_frames_shutter_rays"):
        assert callable(getattr(bh.Scene, m)), m


def apply_host(rows, m):
    return raymap.apply_pose(rows, m)


@pytest.mark.parametrize("W,H", [(40, 24), (13, 7)])
@pytest.mark.parametrize("name", pref.POSES + ["turn0", "turn7"])
def test_apply_host_is_the_numpy_formula(name, W, H):
    m = pref.camera_map("general", W, H)
    p = pref.rows(name)
    got, want = apply_host(p, m), pref.apply_np(p, m)
    assert got.shape == (H, W, 3) and got.dtype == f32 and got.flags.c_contiguous
    assert np.array_equal(ref.canonical_nan(got), ref.canonical_nan(want))
    assert np.isfinite(want).all(), "a general map under a named pose stays finite"


def test_apply_host_non_finite_and_one_pixel():
    p = pref.rows("rotH")
    m = ref.nonfinite_map()
    got, want = apply_host(p, m), pref.apply_np(p, m)
    assert np.array_equal(ref.canonical_nan(got), ref.canonical_nan(want))
    for (y, x), v in ref.NONFINITE.items():  # inf * 0 and nan spread as IEEE spreads them; the zero vector stays zero
        assert np.isfinite(want[y, x]).all() == np.isfinite(np.asarray(v)).all(), (y, x)
    assert np.isnan(want).any() and np.isfinite(want[0, 0]).all()
    one = np.array([[[0.25, -3.0, 1.5]]], f32)
    for name in pref.POSES:
        q = pref.rows(name)
        assert np.array_equal(apply_host(q, one).view(np.uint32), pref.apply_np(q, one).view(np.uint32)), name


def test_unit_axes_keep_finite_vectors_and_lose_a_negative_zero():
    """What the header says of a pose of unit axes: every finite vector without a -0 comes back bit for bit; a -0
    component may come back +0 ((+0) + (-0) = +0), and an infinite one makes the other components NaN (inf * 0)."""
    p = pref.rows("axesD")
    m = pref.camera_map("general", 40, 24)
    got = apply_host(p, m)
    plain = ~(np.signbit(m) & (m == 0)).any(-1)  # the vectors without a -0 (the hand-made rays hold some)
    assert plain.sum() > 900 and not plain.all()
    assert np.array_equal(got[plain].view(np.uint32), m[plain].view(np.uint32))
    assert np.array_equal(got, m), "and the others differ in a zero's sign at the most"
    z = apply_host(p, np.array([[[-0.0, 1.0, 2.0]]], f32))
    assert z[0, 0, 0] == 0.0 and not np.signbit(z[0, 0, 0])
    i = apply_host(p, np.array([[[np.inf, 1.0, 2.0]]], f32))
    assert np.isinf(i[0, 0, 0]) and np.isnan(i[0, 0, 1]) and np.isnan(i[0, 0, 2])


def test_apply_host_error_returns():
    lib = bh.load()
    call = lib.bh_ray_pose_apply_host
    p = _abi.bh_ray_pose.from_buffer_copy(pref.rows("rotH").tobytes())
    m = np.ones((8, 8, 3), f32)
    out = np.full((8, 8, 3), 7.0, f32)
    bad = _abi.BH_ERR_INVALID_ARG
    assert call(None, m.ctypes.data, 8, 8, out.ctypes.data) == bad
    assert lib.bh_last_error().decode().startswith("bh_ray_pose_apply_host")
    assert call(C.byref(p), None, 8, 8, out.ctypes.data) == bad
    assert call(C.byref(p), m.ctypes.data, 8, 8, None) == bad
    for W, H in ((0, 8), (8, 0), (65537, 1), (1, 65537)):
        assert call(C.byref(p), m.ctypes.data, W, H, out.ctypes.data) == bad, (W, H)
    assert (out == 7.0).all(), "a refused call wrote"
    assert call(C.byref(p), m.ctypes.data, 8, 8, out.ctypes.data) == _abi.BH_OK and not (out == 7.0).any()
    assert call(C.byref(p), m.ctypes.data, 8, 8, m.ctypes.data) == _abi.BH_OK  # in place
    assert np.array_equal(m, out)
    for dirs in (np.ones((8, 8, 4), f32), np.ones((8, 8), f32), np.ones(3, f32)):
        with pytest.raises(bh.BhError) as e:
            raymap.apply_pose(p, dirs)
        assert e.value.status == bad
    with pytest.raises(bh.BhError) as e:
        raymap.apply_pose(np.ones((3, 3), f32), np.ones((8, 8, 3), f32))
    assert e.value.status == bad


def test_pose_builders():
    p = raymap.pose((7.0, 1.5, -9.0), (0.3, -0.2, 0.9), (0.1, 1.0, 0.0))
    assert isinstance(p, _abi.bh_ray_pose)
    rows = raymap.pose_rows(p)
    assert rows.shape == (4, 3) and rows.dtype == f32
    r, u, f = raymap.basis((0.3, -0.2, 0.9), (0.1, 1.0, 0.0))
    want = np.stack([np.asarray((7.0, 1.5, -9.0)), r, u, f]).astype(f32)
    assert np.array_equal(rows.view(np.uint32), want.view(np.uint32)), "the float64 basis rounded once to fp32"
    d = raymap.pose_rows(raymap.pose((0.0, 0.0, -20.0)))  # the default frame is the unit axes
    assert np.array_equal(d[1:], np.eye(3, dtype=f32))
    # a camera-space map turned by pose(forward, up) is the builder's map of that forward and up
    W, H = 13, 7
    for build in (raymap.equirect, lambda w, h, *a: raymap.perspective(w, h, 0.9, *a)):
        turned = raymap.apply_pose(p, build(W, H)).astype(np.float64)
        direct = build(W, H, (0.3, -0.2, 0.9), (0.1, 1.0, 0.0)).astype(np.float64)
        assert np.abs(turned - direct).max() <= 1e-6
    cam = bh.Camera.look_at((7.0, 1.5, -9.0), (0.0, 0.0, 0.0), 40, 24)
    c = raymap.pose_rows(raymap.pose_of(cam))
    assert np.array_equal(c, raymap.pose_rows(raymap.pose(cam.pos, cam.dir, cam.up)))
    assert np.array_equal(c[0], np.asarray(cam.pos, f32))
    for call in (lambda: raymap.pose((1.0, 2.0)), lambda: raymap.pose("abc"), lambda: raymap.pose((0, 0, 0), (0, 0, 0)),
                 lambda: raymap.pose((0, 0, 0), (0, 1, 0), (0, 2, 0)), lambda: raymap.pose_of(object())):
        with pytest.raises(bh.BhError) as e:
            call()
        assert e.value.status == _abi.BH_ERR_INVALID_ARG


def test_python_side_refusals_of_poses():
    """scene._poses_arg, which the posed methods run before the library is called."""
    arg = scene_mod._poses_arg
    good = pref.rows("rotH")
    ps = arg([good, raymap.pose((0.0, 0.0, -20.0))], 2, "render_frames_rays")
    assert len(ps) == 2 and np.array_equal(raymap.pose_rows(ps[0]), good)
    assert np.array_equal(raymap.pose_rows(ps[1])[1:], np.eye(3, dtype=f32))
    cases = {"None": (None, 1), "count": ([good], 2), "empty": ([], 0), "too many": ([good] * 257, 257),
             "shape": ([np.zeros((3, 3), f32)], 1), "flat": ([np.zeros(12, f32)], 1), "text": (["abc"], 1),
             "ragged": ([[(1, 2, 3), (1, 2), (1, 2, 3), (1, 2, 3)]], 1), "number": (5.0, 1)}
    for name, (poses, n) in cases.items():
        with pytest.raises(bh.BhError) as e:
            arg(poses, n, "render_frames_rays")
        assert e.value.status == _abi.BH_ERR_INVALID_ARG and str(e.value).startswith("render_frames_rays"), name


def test_library_refusals_that_need_no_device():
    """The NULL checks come before any device work: a NULL context is refused, with the function's name."""
    lib = bh.load()
    p = _abi.bh_ray_pose()
    U, d = _abi.bh_uniforms(), _abi.bh_render_desc()
    bad = _abi.BH_ERR_INVALID_ARG
    assert lib.bh_render_frames_rays(None, 1, C.byref(p), C.byref(U), C.byref(d), 0x1000, 1, None) == bad
    assert lib.bh_last_error().decode().startswith("bh_render_frames_rays")
    assert lib.bh_render_frames_shutter_rays(None, 1, 2, C.byref(p), C.byref(U), C.byref(d), 0x1000, 1, None) == bad
    assert lib.bh_last_error().decode().startswith("bh_render_frames_shutter_rays")
    assert lib.bh_render_lens_rays_posed(None, C.byref(p), C.byref(U), C.byref(d), 0x1000, 0x1000, None) == bad
    assert lib.bh_last_error().decode().startswith("bh_render_lens_rays_posed")


def test_pose_sets_reach_every_fate():
    """The sets tests/test_gpu_rays_pose.py renders: distinct poses, and all four fates in each (default scenario)."""
    assert len(set(pref.sequence(33))) == 33
    seen = {tuple(pref.rows(n).ravel().tolist()) for n in pref.sequence(33)}
    assert len(seen) == 33, "every pose of the longest set differs"
    for n in (1, 2, 3, 33):
        pref.assert_all_fates(pref.sequence(n), "general", 13, 7, f"frames n = {n} 13x7")
    pref.assert_all_fates(pref.sequence(3), "general", 40, 24, "frames n = 3 40x24")
    lens = {np.round(np.linalg.norm(pref.rows("shearF2")[i]), 6) for i in (1, 2)}
    assert min(lens) < 2e-3 and max(lens) > 5e2, "the sheared pose's rows: about 1e-3 and 1e3 long"
    assert np.linalg.det(pref.rows("mirrorD")[1:].astype(np.float64)) < -0.99
    assert np.linalg.det(pref.rows("rotH")[1:].astype(np.float64)) > 0.99
