"""Adaptive supersampling, host side (no GPU): bh_refine_mask_host -- the detect kernel's own lane code
(csrc/bh_refine.hpp) run tile by tile on the host -- against the numpy restatement of the normative rule
(tests/_adaptive_ref.py), and bh_refine_cover_host -- the work-list march's item -> tile -> pixel mapping --
against "every pixel of a refined tile exactly once, every other pixel never"."""
import ctypes as C

import numpy as np
import pytest

import black_hole_ray_marching_amd as bh
from black_hole_ray_marching_amd import _abi
from tests._adaptive_ref import CAMS, DT, KS, SIZES, T, pixel_mask, plain, tile_mask

FMTS = [bh.BH_OUT_RGBA32F, bh.BH_OUT_RGBA16F, bh.BH_OUT_BGRA8_SRGB]


def test_entry_points_exported_and_prototyped():
    lib = bh.load()
    for name in ("bh_render_adaptive", "bh_render_frames_adaptive", "bh_refine_mask_host", "bh_refine_cover_host"):
        assert name in _abi.SIGNATURES, name
        fn = getattr(lib, name)  # AttributeError: not exported
        res, args = _abi.SIGNATURES[name]
        assert fn.restype is res and list(fn.argtypes) == list(args)
    assert _abi.SIGNATURES["bh_render_adaptive"][1][-2:] == [C.POINTER(_abi.bh_adaptive_desc), C.c_void_p]
    assert C.sizeof(_abi.bh_adaptive_desc) == 24 and _abi.bh_adaptive_desc.tile_mask.offset == 8
    assert lib.bh_abi_version() == 8  # additive: callers probe for the symbols


@pytest.mark.parametrize("t", [T, 0.0])
@pytest.mark.parametrize("blackout", [True, False])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("W,H", SIZES)
def test_mask_host_equals_numpy_rule_on_oracle_frames(W, H, fmt, blackout, t):
    seen = set()
    for cam in CAMS:
        pc, pb = plain(cam, W, H, fmt)
        want = tile_mask(fmt, pc, pb if blackout else None, t)
        got = bh.refine_mask_host(pc, pb if blackout else None, fmt, t)
        assert got.dtype == np.uint8 and got.shape == want.shape
        assert np.array_equal(got, want), f"camera {cam}: got\n{got}\nwant\n{want}"
        seen |= set(np.unique(want).tolist())
    if (W, H) != (13, 7) and t == T:
        assert seen == {0, 1}, "the oracle frames show refined and unrefined tiles"


def _frame(fmt, W, H, value=0.25):
    """a flat frame: every colour channel `value` (a byte 64 in BGRA8), alpha 1"""
    a = np.empty((H, W, 4), DT[fmt])
    if fmt == bh.BH_OUT_BGRA8_SRGB:
        a[..., :3], a[..., 3] = 64, 255
    else:
        a[..., :3], a[..., 3] = value, 1.0
    return a


def _bump(fmt, a, x, y, ch=1, by=0.5):
    """raise one channel of pixel (x, y) by `by` (by * 255 bytes in BGRA8): exact in every format"""
    a[y, x, ch] += DT[fmt](round(by * 255)) if fmt == bh.BH_OUT_BGRA8_SRGB else DT[fmt](by)


def _both(fmt, col, bo, t):
    """the host function's mask, checked against the numpy rule"""
    got = bh.refine_mask_host(col, bo, fmt, t)
    assert np.array_equal(got, tile_mask(fmt, col, bo, t))
    return got


@pytest.mark.parametrize("fmt", FMTS)
class TestSynthetic:
    W, H = 24, 16  # 3 x 2 tiles

    def test_one_odd_pixel_at_7_7_refines_the_four_tiles_around_the_corner_it_touches(self, fmt):
        a = _frame(fmt, self.W, self.H)
        _bump(fmt, a, 7, 7)
        # (7, 7) is tile (0, 0)'s last pixel: its neighbours (8, 7) and (7, 8) lie in tiles (1, 0) and (0, 1)
        assert _both(fmt, a, None, T).tolist() == [[1, 1, 0], [1, 0, 0]]

    def test_one_odd_pixel_at_8_8(self, fmt):
        a = _frame(fmt, self.W, self.H)
        _bump(fmt, a, 8, 8)
        # tile (1, 1)'s first pixel: neighbours (7, 8) in tile (0, 1) and (8, 7) in tile (1, 0)
        assert _both(fmt, a, None, T).tolist() == [[0, 1, 0], [1, 1, 0]]

    def test_an_edge_on_a_tile_boundary_refines_both_tiles(self, fmt):
        a = _frame(fmt, self.W, self.H)
        for y in range(self.H):
            for x in range(8, self.W):
                _bump(fmt, a, x, y)  # columns 0..7 against 8..23: the step lies between tiles 0 and 1
        assert _both(fmt, a, None, T).tolist() == [[1, 1, 0], [1, 1, 0]]

    def test_a_difference_only_in_the_blackout_target(self, fmt):
        a, b = _frame(fmt, self.W, self.H), _frame(fmt, self.W, self.H)
        _bump(fmt, b, 20, 3)
        assert _both(fmt, a, b, T).tolist() == [[0, 0, 1], [0, 0, 0]]
        assert not _both(fmt, a, None, T).any()  # without the second target only col counts

    def test_a_difference_only_in_alpha_refines_nothing(self, fmt):
        a = _frame(fmt, self.W, self.H)
        a[5, 5, 3] = 0
        assert not _both(fmt, a, a.copy(), 0.0).any()

    def test_d_equal_to_T_refines_nothing(self, fmt):
        a = _frame(fmt, self.W, self.H)
        _bump(fmt, a, 12, 4, by=0.2)  # 0.45 - 0.25 in fp32 / fp16, 51 bytes
        v = a[4, 12, 1]
        d = float(np.float32(v) - np.float32(a[4, 11, 1]))
        t = d / 255.0 if fmt == bh.BH_OUT_BGRA8_SRGB else d
        if fmt == bh.BH_OUT_BGRA8_SRGB:
            assert np.float32(t) * np.float32(255.0) == np.float32(d), "T * 255 is exactly d in fp32"
        assert np.float32(t) == t or fmt == bh.BH_OUT_BGRA8_SRGB
        assert not _both(fmt, a, None, t).any()  # strict >
        below = float(np.nextafter(np.float32(t), np.float32(0)))
        assert _both(fmt, a, None, below).tolist() == [[0, 1, 0], [0, 0, 0]]

    def test_a_1x1_frame_refines_nothing(self, fmt):
        a = _frame(fmt, 1, 1)
        got = _both(fmt, a, a.copy(), 0.0)
        assert got.shape == (1, 1) and not got.any()

    def test_a_row_end_is_no_neighbour_of_the_next_row_start(self, fmt):
        """Every row is the same ramp in x whose steps stay below T while its ends are far apart: the
        right-hand column differs from the next row's left-hand column and from no true neighbour.  Nothing
        is refined; a row-major wrap would refine tile columns 0 and 2."""
        a = _frame(fmt, self.W, self.H)
        for x in range(self.W):
            a[:, x, :3] = 5 + 10 * x if fmt == bh.BH_OUT_BGRA8_SRGB else DT[fmt](0.25 + 0.05 * x)
        v = a[0, :, 0].astype(np.float64)
        scale = 255.0 if fmt == bh.BH_OUT_BGRA8_SRGB else 1.0
        assert np.abs(np.diff(v)).max() < T * scale < abs(v[-1] - v[0])
        assert not _both(fmt, a, a.copy(), T).any()
        # frames one pixel wide or high: every pixel is a row's start and end at once
        col = _frame(fmt, 1, 16)
        _bump(fmt, col, 0, 9)
        assert _both(fmt, col, None, T).tolist() == [[0], [1]]
        row = _frame(fmt, 16, 1)
        _bump(fmt, row, 9, 0)
        assert _both(fmt, row, None, T).tolist() == [[0, 1]]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("W,H", SIZES)
def test_cover_host(W, H, k):
    ty, tx = (H + 7) // 8, (W + 7) // 8
    masks = {f"oracle {cam}": tile_mask(bh.BH_OUT_RGBA32F, *plain(cam, W, H), T) for cam in CAMS}
    masks["all ones"] = np.ones((ty, tx), np.uint8)
    masks["checkerboard"] = (np.add.outer(np.arange(ty), np.arange(tx)) & 1).astype(np.uint8)
    masks["none"] = np.zeros((ty, tx), np.uint8)
    for name, m in masks.items():
        writes = bh.refine_cover_host(W, H, k, m)  # raises BH_ERR_INTERNAL on an index outside W * H
        assert writes.shape == (H, W)
        want = pixel_mask(m, W, H).astype(np.uint8)  # exactly once inside refined tiles, never elsewhere
        assert np.array_equal(writes, want), f"{name}: {np.argwhere(writes != want)[:4].tolist()}"


def test_cover_host_leaves_no_byte_past_the_frame():
    W, H, k = 13, 7, 4
    buf = np.full(W * H + 64, 0xA5, np.uint8)
    m = np.ones((1, 2), np.uint8)
    assert bh.load().bh_refine_cover_host(W, H, k, m.ctypes.data, buf.ctypes.data) == _abi.BH_OK
    assert (buf[:W * H] == 1).all() and (buf[W * H:] == 0xA5).all()


@pytest.mark.parametrize("t", [float("nan"), -1.0, float("inf"), -0.0 - 1e-30])
def test_mask_host_refuses_bad_thresholds(t):
    a = np.zeros((8, 8, 4), np.float32)
    m = np.full((1, 1), 7, np.uint8)
    lib = bh.load()
    assert lib.bh_refine_mask_host(a.ctypes.data, None, 8, 8, bh.BH_OUT_RGBA32F, t, m.ctypes.data) == _abi.BH_ERR_INVALID_ARG
    assert m[0, 0] == 7


def test_host_functions_refuse_bad_arguments():
    lib = bh.load()
    a = np.zeros((8, 8, 4), np.float32)
    m = np.full((1, 1), 7, np.uint8)
    w = np.full((8, 8), 7, np.uint8)
    bad = _abi.BH_ERR_INVALID_ARG
    assert lib.bh_refine_mask_host(None, None, 8, 8, 0, 0.1, m.ctypes.data) == bad
    assert lib.bh_refine_mask_host(a.ctypes.data, None, 8, 8, 0, 0.1, None) == bad
    assert lib.bh_refine_mask_host(a.ctypes.data, None, 0, 8, 0, 0.1, m.ctypes.data) == bad
    assert lib.bh_refine_mask_host(a.ctypes.data, None, 8, 0, 0, 0.1, m.ctypes.data) == bad
    assert lib.bh_refine_mask_host(a.ctypes.data, None, 8, 8, 3, 0.1, m.ctypes.data) == bad
    assert lib.bh_refine_mask_host(a.ctypes.data, None, 32769, 1, 0, 0.1, m.ctypes.data) == bad
    assert m[0, 0] == 7
    assert lib.bh_refine_mask_host(a.ctypes.data, None, 8, 8, 0, 0.0, m.ctypes.data) == _abi.BH_OK and m[0, 0] == 0
    for ss in (0, 1, 3, 16):
        assert lib.bh_refine_cover_host(8, 8, ss, m.ctypes.data, w.ctypes.data) == bad
    assert lib.bh_refine_cover_host(8, 8, 2, None, w.ctypes.data) == bad
    assert lib.bh_refine_cover_host(8, 8, 2, m.ctypes.data, None) == bad
    assert lib.bh_refine_cover_host(0, 8, 2, m.ctypes.data, w.ctypes.data) == bad
    assert lib.bh_refine_cover_host(32769, 1, 2, m.ctypes.data, w.ctypes.data) == bad
    assert (w == 7).all()
