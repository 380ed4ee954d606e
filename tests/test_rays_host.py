"""Ray maps, host side (no GPU): bh_ray_map_pinhole_host against the numpy oracle's pixel directions, bit for bit
after the oracle's normalisation; its error returns; the raymap builders' shapes, dtype, unit length and stated
formulas; the Python-side refusals of Scene.render_rays / render_lens(dirs=...) that need no device; and the presence
of the three ray-map symbols at ABI version 8."""
import ctypes as C

import numpy as np
import pytest

import black_hole_ray_marching_amd as bh
from black_hole_ray_marching_amd import _abi, raymap, scene as scene_mod
from oracle import oracle_np
from tests import _rays_ref
from tests._cases import camera_uniform

f32 = np.float32
SYMBOLS = ["bh_render_rays", "bh_render_lens_rays", "bh_ray_map_pinhole_host"]


def test_abi_has_the_ray_map_symbols():
    lib = bh.load()
    assert lib.bh_abi_version() == 8 == _abi.ABI_VERSION
    for name in SYMBOLS:
        assert name in _abi.SIGNATURES and hasattr(lib, name), name
    assert bh.raymap is raymap and callable(bh.Scene.render_rays)


@pytest.mark.parametrize("W,H", [(13, 7), (40, 24), (1, 1)])
@pytest.mark.parametrize("cam", ["A", "D", "E", "F2", "H"])
def test_pinhole_map_is_the_oracle_direction(cam, W, H):
    cu = camera_uniform(cam, W, H)
    m = raymap.pinhole(cu, W, H)
    assert m.shape == (H, W, 3) and m.dtype == f32 and m.flags.c_contiguous
    want = oracle_np.pixel_dirs(cu.world_tri, W, H).reshape(H, W, 3)
    got = _rays_ref.normalise(m)
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want, f32).view(np.uint32))
    if W > 1:  # (the one pixel of 1 x 1 is the centre ray, already of length 1)
        assert not np.array_equal(m, got), "the map holds the unnormalised vector"


def test_pinhole_map_error_returns():
    lib = bh.load()
    cu = camera_uniform("A", 8, 8)
    out = np.full((8, 8, 3), 7.0, f32)
    call = lib.bh_ray_map_pinhole_host
    assert call(None, 8, 8, out.ctypes.data) == _abi.BH_ERR_INVALID_ARG
    assert lib.bh_last_error().decode().startswith("bh_ray_map_pinhole_host")
    assert call(C.byref(cu.c), 8, 8, None) == _abi.BH_ERR_INVALID_ARG
    for W, H in ((0, 8), (8, 0), (65537, 1), (1, 65537)):
        assert call(C.byref(cu.c), W, H, out.ctypes.data) == _abi.BH_ERR_INVALID_ARG, (W, H)
    other = camera_uniform("A", 8, 8)
    other.c.screen_tri[0][0] = 2.0
    assert call(C.byref(other.c), 8, 8, out.ctypes.data) == _abi.BH_ERR_UNSUPPORTED
    assert lib.bh_last_error().decode().startswith("bh_ray_map_pinhole_host")
    assert (out == 7.0).all(), "a refused call wrote"
    assert call(C.byref(cu.c), 8, 8, out.ctypes.data) == _abi.BH_OK and not (out == 7.0).any()
    for bad in (0, -1, 65537, 2.5, True):
        with pytest.raises(bh.BhError) as e:
            raymap.pinhole(cu, bad, 8)
        assert e.value.status == _abi.BH_ERR_INVALID_ARG


FWD, UP = (0.3, -0.2, 0.9), (0.1, 1.0, 0.0)
BUILDERS = {
    "perspective": lambda W, H: raymap.perspective(W, H, 1.0, FWD, UP),
    "equirect": lambda W, H: raymap.equirect(W, H, FWD, UP),
    "fisheye": lambda W, H: raymap.fisheye(W, H, np.pi, FWD, UP),
    "fisheye360": lambda W, H: raymap.fisheye(W, H, 2 * np.pi, FWD, UP),
}


def unit(m):
    d = m.astype(np.float64)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


@pytest.mark.parametrize("W,H", [(13, 7), (40, 24), (1, 1), (7, 13)])
@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_builders_shape_dtype_and_length(name, W, H):
    m = BUILDERS[name](W, H)
    assert m.shape == (H, W, 3) and m.dtype == f32 and m.flags.c_contiguous and np.isfinite(m).all()
    ln = np.linalg.norm(m.astype(np.float64), axis=-1)
    if name == "perspective":  # f + offsets in the image plane: the component along f is 1
        r, u, f = raymap.basis(FWD, UP)
        assert np.allclose(m.astype(np.float64) @ f, 1.0, atol=1e-6) and (ln >= 1.0 - 1e-6).all()
    else:
        assert np.abs(ln - 1.0).max() <= 1e-6


def test_equirect_formula():
    W, H = 41, 21  # odd: a centre column and a centre row of pixels
    r, u, f = raymap.basis(FWD, UP)
    m = raymap.equirect(W, H, FWD, UP).astype(np.float64)
    assert np.abs(m[H // 2, W // 2] - f).max() <= 1e-6, "the centre looks along forward"
    assert np.abs(m[:, W // 2] @ r).max() <= 1e-6, "the centre column lies in the (forward, up) plane"
    lat = (0.5 - (np.arange(H) + 0.5) / H) * np.pi
    assert np.abs(m[:, W // 2] @ u - np.sin(lat)).max() <= 1e-6 and np.abs(m[:, W // 2] @ f - np.cos(lat)).max() <= 1e-6
    lon = (2 * (np.arange(W) + 0.5) / W - 1) * np.pi
    assert np.abs(m[H // 2] @ r - np.sin(lon)).max() <= 1e-6 and np.abs(m[H // 2] @ f - np.cos(lon)).max() <= 1e-6
    assert (m[0] @ u > 0.98).all() and (m[-1] @ u < -0.98).all(), "the top row looks up"
    d = raymap.equirect(40, 24)  # the default frame: forward +z, up +y, right = cross(f, up)
    assert d.shape == (24, 40, 3) and d[12, 20, 2] > 0.98 and d[0, 0, 1] > 0.98


def test_perspective_formula():
    W, H, fovy = 40, 24, 0.9
    r, u, f = raymap.basis(FWD, UP)
    m = raymap.perspective(W, H, fovy, FWD, UP).astype(np.float64)
    t = np.tan(fovy / 2)
    sx, sy = (np.arange(W) + 0.5) / W, (np.arange(H) + 0.5) / H
    assert np.abs(m @ r - ((2 * sx - 1) * t * W / H)[None, :]).max() <= 1e-6
    assert np.abs(m @ u - ((1 - 2 * sy) * t)[:, None]).max() <= 1e-6
    # the scene camera's own projection, up to the normalisation: fovy, dir and up of the default camera
    for cam in (bh.Camera.default(W, H), bh.Camera.look_at((7.0, 1.5, -9.0), (0.0, 0.0, 0.0), W, H)):
        cu = bh.CameraUniform()
        cu.update(cam)
        same = unit(raymap.perspective(W, H, cam.fovy, cam.dir, cam.up)) - unit(raymap.pinhole(cu, W, H))
        assert np.abs(same).max() <= 1e-5


def test_fisheye_formula():
    W, H, fov = 41, 21, np.pi
    r, u, f = raymap.basis(FWD, UP)
    m = raymap.fisheye(W, H, fov, FWD, UP).astype(np.float64)
    assert np.abs(m[H // 2, W // 2] - f).max() <= 1e-6
    X = (2 * (np.arange(W) + 0.5) / W - 1) * W / H
    theta = np.minimum(np.abs(X), 1.0) * fov / 2  # along the centre row: equidistant in the angle from forward
    row = m[H // 2]
    along = row @ f
    across = np.linalg.norm(row - along[:, None] * f, axis=-1)
    assert np.abs(np.arctan2(across, along) - theta).max() <= 1e-6  # (arccos of fp32 values near 1 resolves 3e-4)
    outside = np.abs(X) > 1.0
    assert outside.any() and np.abs(m[H // 2][outside] @ f).max() <= 1e-6, "beyond the circle: the rim's direction"
    off = np.arange(W) != W // 2
    assert np.array_equal(np.sign(row @ r)[off], np.sign(X)[off]), "image right is +r"


def test_cube_faces():
    N = 9
    r, u, f = raymap.basis(FWD, UP)
    axes = {"+x": r, "-x": -r, "+y": u, "-y": -u, "+z": f, "-z": -f}
    seen = []
    for face in raymap.FACES:
        m = raymap.cube_face(N, face, FWD, UP)
        assert m.shape == (N, N, 3) and m.dtype == f32
        d = m.astype(np.float64)
        assert np.abs(d[N // 2, N // 2] - axes[face]).max() <= 1e-6, face
        assert np.abs(d @ axes[face] - 1.0).max() <= 1e-6, face  # on the cube's face
        for other, a in axes.items():
            if other[1] != face[1]:
                assert np.abs(d @ a).max() <= 1.0 - 1.0 / N + 1e-6
        seen.append(unit(m).reshape(-1, 3))
    # the six faces tile the sphere: every axis direction and every octant's diagonal is near some pixel
    allv = np.concatenate(seen)
    for probe in [(1, 1, 1), (-1, 1, -1), (1, -1, -1), (-1, -1, 1), (1, 0, 0), (0, -1, 0)]:
        p = np.asarray(probe, np.float64)
        assert (allv @ (p / np.linalg.norm(p))).max() > 0.97
    with pytest.raises(bh.BhError):
        raymap.cube_face(N, "front")


def test_builders_refuse_bad_arguments():
    for call in (lambda: raymap.equirect(0, 8), lambda: raymap.equirect(8, 65537), lambda: raymap.equirect(8.0, 8),
                 lambda: raymap.perspective(8, 8, 0.0), lambda: raymap.perspective(8, 8, np.pi),
                 lambda: raymap.perspective(8, 8, float("nan")), lambda: raymap.fisheye(8, 8, 7.0),
                 lambda: raymap.fisheye(8, 8, -1.0), lambda: raymap.equirect(8, 8, (0, 0, 0)),
                 lambda: raymap.equirect(8, 8, (0, 1, 0), (0, 2, 0)), lambda: raymap.equirect(8, 8, (0, 1), (0, 1, 0)),
                 lambda: raymap.cube_face(0, "+x")):
        with pytest.raises(bh.BhError) as e:
            call()
        assert e.value.status == _abi.BH_ERR_INVALID_ARG


def test_python_side_refusals_of_a_ray_map():
    """scene._check_dirs and _pos_arg, which Scene.render_rays and render_lens(dirs=...) run before the library is
    called: host tensors stand in for device ones up to the last check, which refuses them for being on the host."""
    torch = pytest.importorskip("torch")
    check = scene_mod._check_dirs
    good = torch.zeros((7, 13, 3), dtype=torch.float32)
    cases = {"None": None, "numpy": np.zeros((7, 13, 3), f32), "shape": torch.zeros((7, 13, 4)),
             "transposed": torch.zeros((13, 7, 3)), "flat": torch.zeros(7 * 13 * 3),
             "float64": torch.zeros((7, 13, 3), dtype=torch.float64), "int32": torch.zeros((7, 13, 3), dtype=torch.int32),
             "float16": torch.zeros((7, 13, 3), dtype=torch.float16),
             "strided": torch.zeros((7, 13, 6), dtype=torch.float32)[:, :, ::2], "host": good}
    for name, t in cases.items():
        with pytest.raises(bh.BhError) as e:
            check(t, 7, 13, "render_rays")
        assert e.value.status == _abi.BH_ERR_INVALID_ARG and str(e.value).startswith("render_rays"), name
    assert "device" in str(e.value)
    check(0x1000, 7, 13, "render_rays")  # a raw pointer is trusted
    for pos in ((1.0, 2.0), (1.0, 2.0, 3.0, 4.0), "abc", None, 5.0, ("a", "b", "c")):
        with pytest.raises(bh.BhError) as e:
            scene_mod._pos_arg(pos, "render_rays")
        assert e.value.status == _abi.BH_ERR_INVALID_ARG, pos
    p = scene_mod._pos_arg(np.asarray((1.5, -2.0, 0.25), f32), "render_rays")
    assert list(p) == [1.5, -2.0, 0.25]


def test_library_refusals_that_need_no_device():
    """The NULL checks come before any device work: a NULL context is refused, with the function's name."""
    lib = bh.load()
    pos = (C.c_float * 3)(0.0, 0.0, -20.0)
    U, d = _abi.bh_uniforms(), _abi.bh_render_desc()
    assert lib.bh_render_rays(None, pos, C.byref(U), C.byref(d), 0x1000, 1, None) == _abi.BH_ERR_INVALID_ARG
    assert lib.bh_last_error().decode().startswith("bh_render_rays")
    assert lib.bh_render_lens_rays(None, pos, C.byref(U), C.byref(d), 0x1000, 0x1000, None) == _abi.BH_ERR_INVALID_ARG
    assert lib.bh_last_error().decode().startswith("bh_render_lens_rays")


def test_general_maps_reach_every_fate():
    """tests/_rays_ref.general asserts the four fates per position and size; the hand-made rays are all in use."""
    used = set()
    for name in _rays_ref.POSITIONS:
        for W, H in _rays_ref.SIZES:
            _rays_ref.general(name, W, H)
        h = _rays_ref.hand_rays(name)
        row = _rays_ref.general_map(name, 13, 7)[0]
        used |= {i for i in range(len(h)) if (row == h[i]).all(-1).any()}
        assert (_rays_ref.general_map(name, 40, 24)[0, :16] == h).all()
    assert used == set(range(16))
