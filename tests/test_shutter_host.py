"""Shutter render, host side (no GPU): the C ABI's new entry points and bh_shutter_resolve_host -- the shutter
kernel's own mapping and time tree (csrc/bh_shutter.hpp) run workgroup by workgroup on the host -- against the
numpy restatement of the normative tree over the CPU oracle's frames (tests/_shutter_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import black_hole_ray_marching_amd as bh
from black_hole_ray_marching_amd import _abi
from tests._shutter_ref import (NS, SIZES, mixed, oracle_virtual, reference, running_sum_np, samples, sweep,
                                time_tree_np)


def test_entry_points_exported_and_prototyped():
    lib = bh.load()
    for name in ("bh_render_shutter", "bh_render_frames_shutter", "bh_shutter_resolve_host"):
        assert name in _abi.SIGNATURES, name
        fn = getattr(lib, name)  # AttributeError: not exported
        res, args = _abi.SIGNATURES[name]
        assert fn.restype is res and list(fn.argtypes) == list(args)
    assert _abi.SIGNATURES["bh_render_shutter"][1][-2:] == [C.c_uint32, C.c_void_p]
    assert _abi.SIGNATURES["bh_render_frames_shutter"][1][1:3] == [C.c_uint32, C.c_uint32]
    assert len(_abi.SIGNATURES["bh_shutter_resolve_host"][1]) == 7
    assert lib.bh_abi_version() == 8  # additive: callers probe for the symbols


def assert_same_bits(got, want, what=""):
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.any(-1).sum())} pixels differ, first at {np.argwhere(bad)[:4].tolist()}"


def virtual_samples(cams, W, H, k, target):
    """(n, kH, kW, 4): the oracle's virtual frames of `cams`, target 0 (col) or 1 (blackout_col)"""
    return np.stack([oracle_virtual(c, W, H, k)[target] for c in cams])


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("n", NS)
def test_resolve_host_equals_the_reference(n, W, H, k):
    """One output frame, both targets: the mirror over the oracle's virtual frames is the reference bit for bit;
    and (from the oracle alone) the tree is not a running sum, so the order is what is tested."""
    cams = mixed(n, W, H)
    fates = np.concatenate([oracle_virtual(c, W, H, k)[2].ravel() for c in cams])
    if n >= 8:
        assert set(np.unique(fates)) == {0, 1, 2, 3}, "the mixed cameras show all four fates"
    want = reference(cams, W, H, k)
    for target in (0, 1):
        got = bh.shutter_resolve_host(virtual_samples(cams, W, H, k, target), n, k)
        assert got.shape == (1, H, W, 4)
        assert_same_bits(got[0], want[target], f"target {target}")
        assert (got[..., 3] == 1.0).all()
    if n >= 4:
        # per case, on the col target (the blackout target of a small frame is mostly exact zeros and ones, whose
        # sums round nowhere: its count is printed, not asserted)
        count = []
        for target in (0, 1):
            s = samples(cams, W, H, k)[target]
            differ = (running_sum_np(s).view(np.uint32) != time_tree_np(s).view(np.uint32)).any(-1)
            count.append(int(differ.sum()))
        print(f"n={n} {W}x{H} ss={k}: tree != running sum on {count[0]} (col) and {count[1]} (blackout_col) pixels")
        assert count[0] > 0, "the tree and a running sum agree everywhere: the case cannot tell them apart"


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("n", [2, 8])
def test_resolve_host_three_frames(n, W, H, k):
    """Three output frames with different camera sets in one call: each equals its own reference."""
    sets = [mixed(n, W, H, first=0), sweep(n, W, H), mixed(n, W, H, first=3)]
    for target in (0, 1):
        s = np.concatenate([virtual_samples(cams, W, H, k, target) for cams in sets])
        got = bh.shutter_resolve_host(s, n, k)
        assert got.shape == (3, H, W, 4)
        for f, cams in enumerate(sets):
            assert_same_bits(got[f], reference(cams, W, H, k)[target], f"frame {f} target {target}")


@pytest.mark.parametrize("n", NS)
def test_resolve_host_equals_numpy_tree_on_random_values(n):
    W, H = 9, 5
    rng = np.random.default_rng(0x5A77 + n)
    # magnitudes spread over many binades: the add order shows in the low bits
    a = (rng.standard_normal((2 * n, H, W, 4)) * np.exp2(rng.integers(-12, 12, (2 * n, H, W, 4)))).astype(np.float32)
    got = bh.shutter_resolve_host(a, n)
    for f in range(2):
        assert_same_bits(got[f], time_tree_np(a[f * n:(f + 1) * n]), f"frame {f}")
    if n >= 4:
        assert (running_sum_np(a[:n]).view(np.uint32) != got[0].view(np.uint32)).any()


def test_resolve_host_n1_is_the_ss_resolve():
    rng = np.random.default_rng(5)
    a = rng.standard_normal((3, 10, 18, 4)).astype(np.float32)
    got = bh.shutter_resolve_host(a, 1, 2)
    for f in range(3):
        assert_same_bits(got[f], bh.ss_resolve_host(a[f], 2), f"frame {f}")


@pytest.mark.parametrize("n_frames,n_sub,W,H,ss", [
    (1, 0, 8, 8, 1), (1, 3, 8, 8, 1), (1, 32, 8, 8, 1),      # n_sub outside {1, 2, 4, 8, 16}
    (17, 16, 8, 8, 1), (129, 2, 8, 8, 1), (0, 2, 8, 8, 1),   # n_frames * n_sub above BH_MAX_FRAMES, no frame
    (1, 2, 8, 8, 0), (1, 2, 8, 8, 3), (1, 2, 8, 8, 16),      # ss outside {1, 2, 4, 8}
    (1, 2, 0, 8, 1), (1, 2, 8, 0, 1), (1, 2, 32769, 1, 2), (1, 2, 1, 8193, 8)])  # the size limits of bh_render_ss
def test_resolve_host_error_returns(n_frames, n_sub, W, H, ss):
    """Refused before anything is read or written: the buffers hold one pixel each."""
    one = np.zeros(4, np.float32)
    out = np.full(4, 7.0, np.float32)
    st = bh.load().bh_shutter_resolve_host(one.ctypes.data, n_frames, n_sub, W, H, ss, out.ctypes.data)
    assert st == _abi.BH_ERR_INVALID_ARG
    assert (out == 7.0).all()


def test_resolve_host_null_pointers():
    one = np.zeros(8, np.float32)
    lib = bh.load()
    assert lib.bh_shutter_resolve_host(None, 1, 2, 1, 1, 1, one.ctypes.data) == _abi.BH_ERR_INVALID_ARG
    assert lib.bh_shutter_resolve_host(one.ctypes.data, 1, 2, 1, 1, 1, None) == _abi.BH_ERR_INVALID_ARG


def test_render_entry_points_refuse_bad_arguments_without_a_device():
    """Argument checks that need no context: a null context or a bad n_sub is a status, not a crash."""
    lib = bh.load()
    cam, U, d = _abi.bh_camera_uniform(), _abi.bh_uniforms(), _abi.bh_render_desc()
    assert lib.bh_render_shutter(None, 2, C.byref(cam), C.byref(U), C.byref(d), 1, None) == _abi.BH_ERR_INVALID_ARG
    for n_sub in (0, 3, 5, 32):
        assert lib.bh_render_frames_shutter(None, 1, n_sub, C.byref(cam), C.byref(U), C.byref(d), 1, None) == _abi.BH_ERR_INVALID_ARG
    assert lib.bh_render_frames_shutter(None, 1, 2, C.byref(cam), C.byref(U), C.byref(d), 3, None) == _abi.BH_ERR_INVALID_ARG
