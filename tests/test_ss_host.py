"""Supersampled render, host side (no GPU): the C ABI's new entry points and bh_ss_resolve_host -- the march
kernel's own lane code (csrc/bh_ss.hpp: butterfly levels, writer lanes, output index) run wave by wave on
the host -- against the numpy restatement of the normative resolve tree (tests/_ss_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import black_hole_ray_marching_amd as bh
from black_hole_ray_marching_amd import _abi
from tests._ss_ref import KS, SIZES, oracle_virtual, resolve_np


def test_entry_points_exported_and_prototyped():
    lib = bh.load()
    for name in ("bh_render_ss", "bh_render_frames_ss", "bh_ss_resolve_host"):
        assert name in _abi.SIGNATURES, name
        fn = getattr(lib, name)  # AttributeError: not exported
        res, args = _abi.SIGNATURES[name]
        assert fn.restype is res and list(fn.argtypes) == list(args)
    # ss is the argument before the stream; the resolve takes (samples, width, height, ss, out)
    assert _abi.SIGNATURES["bh_render_ss"][1][-2:] == [C.c_uint32, C.c_void_p]
    assert _abi.SIGNATURES["bh_render_frames_ss"][1][-2:] == [C.c_uint32, C.c_void_p]
    assert len(_abi.SIGNATURES["bh_ss_resolve_host"][1]) == 5
    assert lib.bh_abi_version() == 8  # additive: callers probe for the symbols


def assert_same_bits(got, want):
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), f"{int(bad.any(-1).sum())} pixels differ, first at {np.argwhere(bad)[:4].tolist()}"


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("W,H", SIZES)
def test_resolve_host_equals_numpy_tree_on_oracle_frames(W, H, k):
    col, bo, fate = oracle_virtual("E", W, H, k)
    assert not np.isnan(col).any() and not np.isnan(bo).any(), "the oracle frame holds a NaN"
    assert set(np.unique(fate)) == {0, 1, 2, 3}, "camera E shows all four fates at every size and k"
    for samples in (col, bo):
        got = bh.ss_resolve_host(samples, k)
        assert got.shape == (H, W, 4)
        assert_same_bits(got, resolve_np(samples, k))
    # pixels whose samples are all equal resolve to exactly that value
    s = col.reshape(H, k, W, k, 4)
    same = (s == s[:, :1, :, :1]).all(axis=(1, 3, 4))
    assert same.any()
    assert_same_bits(bh.ss_resolve_host(col, k)[same][:, :3], s[:, 0, :, 0][same][:, :3])


@pytest.mark.parametrize("k", KS)
def test_resolve_host_equals_numpy_tree_on_random_values(k):
    W, H = 9, 5
    rng = np.random.default_rng(0x55AA + k)
    # magnitudes spread over many binades: the add order shows in the low bits
    a = (rng.standard_normal((k * H, k * W, 4)) * np.exp2(rng.integers(-12, 12, (k * H, k * W, 4)))).astype(np.float32)
    want = resolve_np(a, k)
    assert_same_bits(bh.ss_resolve_host(a, k), want)
    # the check has teeth: a row-major running sum of the same samples differs in bits somewhere
    run = np.zeros((H, W, 3), np.float32)
    for j in range(k):
        for i in range(k):
            run = run + a[j::k, i::k, :3]
    run = run * np.float32(1.0 / (k * k))
    assert (run.view(np.uint32) != want[..., :3].view(np.uint32)).any()


@pytest.mark.parametrize("ss", [0, 3, 16])
def test_resolve_host_refuses_bad_ss(ss):
    a = np.zeros((8, 8, 4), np.float32)
    out = np.full((8, 8, 4), 7.0, np.float32)
    st = bh.load().bh_ss_resolve_host(a.ctypes.data, 1, 1, ss, out.ctypes.data)
    assert st == _abi.BH_ERR_INVALID_ARG
    assert (out == 7.0).all()


def test_resolve_host_ss1_is_a_copy_with_alpha_one():
    rng = np.random.default_rng(3)
    a = rng.standard_normal((5, 9, 4)).astype(np.float32)
    got = bh.ss_resolve_host(a, 1)
    assert_same_bits(got[..., :3], a[..., :3])
    assert (got[..., 3] == 1.0).all()


def _shape_cases():
    """(width, height, ss) just outside the frames the kernels index: a side 0, or ss * side one past 65536"""
    for ss in (2, 4, 8):
        yield 65536 // ss + 1, 1, ss
        yield 1, 65536 // ss + 1, ss
        yield 0, 1, ss
        yield 1, 0, ss


def test_host_mirrors_refuse_a_bad_frame_shape_before_reading():
    """bh_ss_resolve_host, bh_lens_shade_host and bh_refine_cover_host share one shape check (frame_shape_ok,
    csrc/bh_host.hpp), made before anything is read: the buffers here hold one element each."""
    lib = bh.load()
    one = np.zeros(4, np.float32)   # one sample, one lens record and more, one pixel
    byte = np.zeros(1, np.uint8)
    sky = np.zeros(4, np.uint8)
    for W, H, ss in _shape_cases():
        case = (W, H, ss)
        assert lib.bh_ss_resolve_host(one.ctypes.data, W, H, ss, one.ctypes.data) == _abi.BH_ERR_INVALID_ARG, case
        assert lib.bh_lens_shade_host(one.ctypes.data, W, H, ss, sky.ctypes.data, 1, 1, one.ctypes.data,
                                      None) == _abi.BH_ERR_INVALID_ARG, case
        assert lib.bh_refine_cover_host(W, H, ss, byte.ctypes.data, byte.ctypes.data) == _abi.BH_ERR_INVALID_ARG, case
    assert not one.any() and not byte.any()
