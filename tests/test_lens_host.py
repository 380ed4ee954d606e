"""Lens maps on the CPU: bh_lens_shade_host -- the shade kernel's own per-pixel code (csrc/bh_lens.hpp) -- over
the reference records of tests/_lens_ref.py equals the CPU oracle's frames with each sky, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import black_hole_ray_marching_amd as bh
from black_hole_ray_marching_amd import _abi
from tests._lens_ref import CAMS, SIZES, SKIES, frame, records, shade_np, sky

f32 = np.float32


def assert_bits(got, want, what):
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    assert got.shape == want.shape, what
    bad = (got.view(np.uint32) != want.view(np.uint32)).any(-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ, first at {np.argwhere(bad)[:4].tolist()}"


def test_reference_records_are_sane():
    """What the issue states about the reference records, asserted so that a degenerate case cannot hide a
    failure: no NaN, every sky ray's u in [6.9e-5, 1), camera E with all four fates at both sizes."""
    for W, H in SIZES:
        for cam in CAMS:
            rec, fate = records(cam, W, H)
            assert not np.isnan(rec).any()
            sky_ray = fate <= bh.BH_FATE_ESCAPE
            u = rec[..., 0][sky_ray]
            assert (u >= f32(6.9e-5)).all() and (u < 1).all()
            assert (rec[..., 0][fate == bh.BH_FATE_BLACKOUT] == bh.BH_LENS_BLACKOUT).all()
            assert (rec[..., 0][fate == bh.BH_FATE_SURFACE] == bh.BH_LENS_SURFACE).all()
        assert set(np.unique(records("E", W, H)[1]).tolist()) == {0, 1, 2, 3}


@pytest.mark.parametrize("sky_name", SKIES)
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("cam", CAMS)
def test_shade_host_equals_the_oracle(cam, W, H, sky_name):
    col, bo = bh.lens_shade_host(records(cam, W, H)[0], sky(sky_name))
    wc, wb = frame(cam, W, H, sky_name)
    assert_bits(col, wc, "col")
    assert_bits(bo, wb, "blackout_col")


@pytest.mark.parametrize("W,H,k", [(13, 7, 2), (13, 7, 4), (13, 7, 8), (40, 24, 2)])
@pytest.mark.parametrize("cam", ["E", "H"])
def test_shade_host_ss_equals_the_resolved_oracle(cam, W, H, k):
    col, bo = bh.lens_shade_host(records(cam, W, H, k)[0], sky("96x40"), ss=k)
    wc, wb = frame(cam, W, H, "96x40", k)
    assert_bits(col, wc, f"ss={k} col")
    assert_bits(bo, wb, f"ss={k} blackout_col")


@pytest.mark.parametrize("sky_name", SKIES)
def test_hand_made_records(sky_name):
    """NaN coordinates take texel (0, 0); the corners clamp; the sentinels are 0 and 1 whatever the sky."""
    nan = float("nan")
    rec = np.array([[[nan, 0.5], [0.5, nan], [0.0, 0.0], [1.0, 1.0], [bh.BH_LENS_BLACKOUT, 0.0],
                     [bh.BH_LENS_SURFACE, 0.0], [0.25, 0.75], [nan, nan]]], f32)
    s = sky(sky_name)
    col, bo = bh.lens_shade_host(rec, s)
    wc, wb = shade_np(rec, s)
    assert_bits(col, wc, "col")
    assert_bits(bo, wb, "blackout_col")
    t00, _ = shade_np(np.array([[[0.0, 0.0]]], f32), np.ascontiguousarray(s[:1, :1]))
    for i in (0, 1, 7):
        assert_bits(col[0, i], t00[0, 0], "a NaN record shades as texel (0, 0)")
    assert (col[0, 4] == (0, 0, 0, 1)).all() and (bo[0, 4] == (0, 0, 0, 1)).all()
    assert (col[0, 5] == (1, 1, 1, 1)).all() and (bo[0, 5] == (1, 1, 1, 1)).all()


def test_error_returns():
    lib = bh.load()
    rec = np.zeros((4, 4, 2), f32)
    s = sky("1x1")
    out = np.full((4, 4, 4), 7.0, f32)

    def call(lens=rec.ctypes.data, w=4, h=4, ss=1, sk=s.ctypes.data, sw=1, sh=1, col=out.ctypes.data, bo=None):
        return lib.bh_lens_shade_host(lens, w, h, ss, sk, sw, sh, col, bo)

    assert call() == _abi.BH_OK and (out[..., 3] == 1).all()
    out[:] = 7.0
    for kw in (dict(lens=None), dict(sk=None), dict(col=None), dict(w=0), dict(h=0), dict(ss=0), dict(ss=3),
               dict(ss=16), dict(sw=0), dict(sh=0), dict(sw=32769), dict(w=32769, ss=2), dict(h=65537)):
        assert call(**kw) == _abi.BH_ERR_INVALID_ARG, kw
    assert (out == 7.0).all()
    for bad in (np.zeros((4, 4, 3), f32), np.zeros((5, 4, 2), f32)):
        with pytest.raises(bh.BhError) as e:
            bh.lens_shade_host(bad, s, ss=1 if bad.shape[2] == 3 else 2)
        assert e.value.status == _abi.BH_ERR_INVALID_ARG
    assert bh.BH_LENS_BLACKOUT == -1.0 and bh.BH_LENS_SURFACE == -2.0 and C.sizeof(_abi.bh_shade_desc) == 48
