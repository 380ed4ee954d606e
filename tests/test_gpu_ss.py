"""Supersampled render on the GPU (bh_render_ss / Scene.render(ss=k)): k x k rays per pixel resolved in the
march wave, against the CPU oracle's fp32 render of the virtual frame kW x kH resolved by the numpy tree of
tests/_ss_ref.py and encoded as the format stores it -- bit for bit.  The reference is never the GPU's own
output, except in the fast-math test, which says why."""
import ctypes as C
import functools

import numpy as np
import pytest

import black_hole_ray_marching_amd as bh
from black_hole_ray_marching_amd import _abi
from tests._cases import camera_uniform, uniforms
from tests._gpu_common import FAST_TOL
from tests._ss_ref import CAP, FLAGS, KS, SIZES, expected_bytes, reference, resolve_np, sky_ss

pytestmark = pytest.mark.gpu

DT = {bh.BH_OUT_RGBA32F: "float32", bh.BH_OUT_RGBA16F: "float16", bh.BH_OUT_BGRA8_SRGB: "uint8"}
SENTINEL = 0xA5  # every byte of a buffer before a render (an fp32 / fp16 of all-0xA5 bytes is no value a frame holds)


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def new_scene(math=bh.BH_MATH_EXACT):
    return bh.Scene(16, 16, sky=sky_ss(), max_iters=CAP, scene_flags=FLAGS, math=math)


@pytest.fixture(scope="module")
def scene(torch_cuda):
    s = new_scene()
    yield s
    s.close()


def target(torch, W, H, fmt):
    t = torch.full((H, W, 4 * _abi.BYTES_PER_PIXEL[fmt] // 4), SENTINEL, dtype=torch.uint8, device="cuda")
    return t.view(getattr(torch, DT[fmt]))


def as_bytes(t):
    return t.cpu().numpy().view(np.uint8)


def render_ss(torch, scene, cam, W, H, k, fmt=bh.BH_OUT_RGBA32F, blackout=True, schedule=0, math=None):
    """(col bytes, blackout bytes or None) of Scene.render(ss=k) into sentinel-filled targets"""
    scene.camera_uniform, scene.uniforms = camera_uniform(cam, W, H), uniforms()
    col = target(torch, W, H, fmt)
    bo = target(torch, W, H, fmt) if blackout else None
    scene.render(col, bo, fmt=fmt, width=W, height=H, schedule=schedule, ss=k, math=math)
    torch.cuda.synchronize()
    return as_bytes(col), None if bo is None else as_bytes(bo)


def assert_frame(got, want_bytes, what):
    want = want_bytes.reshape(got.shape)
    bad = (got != want).any(-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ, first at {np.argwhere(bad)[:4].tolist()}"


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("cam", ["D", "E", "H"])
def test_oracle_parity(torch_cuda, cam, W, H, k):
    """Both targets bit-equal to the reference; a fresh scene, so the first render runs in the centre-out order
    and the second in the order learned from the first's tile costs.  Camera E also on each build of the exact
    kernels."""
    rc, rb = reference(cam, W, H, k)
    sc = new_scene()
    try:
        for order in ("centre-out", "learned"):
            gc, gb = render_ss(torch_cuda, sc, cam, W, H, k)
            assert_frame(gc, expected_bytes(bh.BH_OUT_RGBA32F, rc), f"col, {order} order")
            assert_frame(gb, expected_bytes(bh.BH_OUT_RGBA32F, rb), f"blackout_col, {order} order")
        if cam == "E":
            for flag in (bh.BH_SCHED_FLAG_ISSUE_ORDER, bh.BH_SCHED_FLAG_LATENCY):
                gc, gb = render_ss(torch_cuda, sc, cam, W, H, k, schedule=bh.BH_SCHED_TILE | flag)
                assert_frame(gc, expected_bytes(bh.BH_OUT_RGBA32F, rc), f"col, schedule flag {flag:#x}")
                assert_frame(gb, expected_bytes(bh.BH_OUT_RGBA32F, rb), f"blackout_col, schedule flag {flag:#x}")
    finally:
        sc.close()


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("fmt", [bh.BH_OUT_RGBA16F, bh.BH_OUT_BGRA8_SRGB])
def test_formats_encode_the_resolved_value(torch_cuda, scene, fmt, k):
    W, H = 40, 24
    rc, rb = reference("E", W, H, k)
    gc, gb = render_ss(torch_cuda, scene, "E", W, H, k, fmt=fmt)
    assert_frame(gc, expected_bytes(fmt, rc), "col")
    assert_frame(gb, expected_bytes(fmt, rb), "blackout_col")


@pytest.mark.parametrize("k", KS)
def test_one_target(torch_cuda, scene, k):
    """blackout_output=None: col is unchanged, and a separately allocated buffer keeps its sentinel."""
    W, H = 40, 24
    rc, _ = reference("E", W, H, k)
    other = target(torch_cuda, W, H, bh.BH_OUT_RGBA32F)
    gc, gb = render_ss(torch_cuda, scene, "E", W, H, k, blackout=False)
    assert gb is None
    assert_frame(gc, expected_bytes(bh.BH_OUT_RGBA32F, rc), "col")
    assert (as_bytes(other) == SENTINEL).all()


@pytest.mark.parametrize("fmt", [bh.BH_OUT_RGBA32F, bh.BH_OUT_BGRA8_SRGB])
def test_ss1_is_the_plain_render(torch_cuda, scene, fmt):
    """ss = 1 through the new entry points is byte-equal to Scene.render on the same frame."""
    torch = torch_cuda
    W, H = 40, 24
    scene.camera_uniform, scene.uniforms = camera_uniform("E", W, H), uniforms()
    pc, pb = target(torch, W, H, fmt), target(torch, W, H, fmt)
    scene.render(pc, pb, fmt=fmt, width=W, height=H)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    for frames in (False, True):
        c, b = target(torch, W, H, fmt), target(torch, W, H, fmt)
        d = scene._desc(c, b, fmt, None, None, None, bh.BH_LAYOUT_ROWMAJOR, 0, 1, W, H, 0, None)
        cu, U = scene.camera_uniform.c, scene.uniforms.to_c()
        if frames:
            st = scene.lib.bh_render_frames_ss(scene._ctx, 1, C.byref(cu), C.byref(U), C.byref(d), 1, stream)
        else:
            st = scene.lib.bh_render_ss(scene._ctx, C.byref(cu), C.byref(U), C.byref(d), 1, stream)
        assert st == _abi.BH_OK
        torch.cuda.synchronize()
        assert np.array_equal(as_bytes(c), as_bytes(pc)) and np.array_equal(as_bytes(b), as_bytes(pb))


def test_multi_frame(torch_cuda, scene):
    """render_frames with three different cameras in one launch: each frame equals its single-frame reference."""
    torch = torch_cuda
    W, H, k = 40, 24, 2
    cams = ["D", "E", "H"]
    scene.uniforms = uniforms()
    cols = [target(torch, W, H, bh.BH_OUT_RGBA32F) for _ in cams]
    bos = [target(torch, W, H, bh.BH_OUT_RGBA32F) for _ in cams]
    scene.render_frames(cols, bos, cameras=[camera_uniform(c, W, H) for c in cams], width=W, height=H, ss=k)
    torch.cuda.synchronize()
    for cam, c, b in zip(cams, cols, bos):
        rc, rb = reference(cam, W, H, k)
        assert_frame(as_bytes(c), expected_bytes(bh.BH_OUT_RGBA32F, rc), f"frame {cam} col")
        assert_frame(as_bytes(b), expected_bytes(bh.BH_OUT_RGBA32F, rb), f"frame {cam} blackout_col")


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("W,H", SIZES)
def test_fast_math_by_composition(torch_cuda, W, H, k):
    """BH_MATH_FAST has no bit-exact oracle, so it is checked by composition: ss = k in fast math must be
    bit-equal to the numpy tree over the GPU's OWN fast-math plain render of the virtual frame kW x kH.  This
    checks the new resolve (and that it takes each sample exactly as the plain kernel stores it) against the
    existing fast march, which the parity tests hold to its tolerance."""
    (gc, gb), (wc, wb) = _fast_pair(torch_cuda, W, H, k)
    for name, g, w in (("col", gc, wc), ("blackout_col", gb, wb)):
        d = np.abs(g.view(np.float32) - w)
        print(f"fast ss={k} {W}x{H} {name}: {int((g.view(np.uint32) != w.view(np.uint32)).any(-1).sum())} of {W * H} "
              f"pixels differ in bits, max |delta| {float(d.max()):.3e}")
    assert_frame(gc.view(np.uint8), expected_bytes(bh.BH_OUT_RGBA32F, wc), "col")
    assert_frame(gb.view(np.uint8), expected_bytes(bh.BH_OUT_RGBA32F, wb), "blackout_col")


@functools.lru_cache(maxsize=None)
def _fast_pair(torch, W, H, k):
    """((col, blackout_col) of ss = k in fast math, the numpy tree over the GPU's fast-math plain render of
    kW x kH), as fp32 (H, W, 4) arrays"""
    sc = new_scene(math=bh.BH_MATH_FAST)
    try:
        sc.camera_uniform, sc.uniforms = camera_uniform("E", W, H), uniforms()
        vc, vb = target(torch, k * W, k * H, bh.BH_OUT_RGBA32F), target(torch, k * W, k * H, bh.BH_OUT_RGBA32F)
        sc.render(vc, vb, width=k * W, height=k * H)
        torch.cuda.synchronize()
        vc, vb = vc.cpu().numpy(), vb.cpu().numpy()
        assert not np.isnan(vc).any() and not np.isnan(vb).any()
        gc, gb = render_ss(torch, sc, "E", W, H, k)
        return (gc.view(np.float32), gb.view(np.float32)), (resolve_np(vc, k), resolve_np(vb, k))
    finally:
        sc.close()




@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("W,H", SIZES)
def test_fast_math_within_the_fast_tolerance(torch_cuda, W, H, k):
    """The same composition held to the fast mode's own bar: every sample of the two fast kernels is within
    FAST_TOL, so every average of k^2 of them is.  (Catches a resolve over the wrong lanes or with the wrong
    scale in the fast build; the add order is checked bit for bit in exact math.)"""
    (gc, _), (wc, _) = _fast_pair(torch_cuda, W, H, k)
    assert float(np.abs(gc - wc).max()) < FAST_TOL
    assert (gc[..., 3] == 1.0).all()


def _refused(torch, scene, status, W=40, H=24, ss=2, sentence=False, **kw):
    """The render raises `status` and launches nothing: the output keeps its sentinel."""
    scene.camera_uniform, scene.uniforms = camera_uniform("E", 40, 24), uniforms()
    col = target(torch, W, H, bh.BH_OUT_RGBA32F)
    with pytest.raises(bh.BhError) as e:
        scene.render(col, None, width=W, height=H, ss=ss, **kw)
    assert e.value.status == status
    if sentence:
        text = scene.lib.bh_last_error().decode()
        assert text.startswith("bh_render_ss") and text.endswith(".") and " " in text
    torch.cuda.synchronize()
    assert (as_bytes(col) == SENTINEL).all()


@pytest.mark.parametrize("ss", [0, 3, 16])
def test_refuses_bad_ss(torch_cuda, scene, ss):
    _refused(torch_cuda, scene, _abi.BH_ERR_INVALID_ARG, ss=ss)


@pytest.mark.parametrize("W,H", [(32769, 1), (1, 32769)])
def test_refuses_a_virtual_frame_above_65536(torch_cuda, scene, W, H):
    _refused(torch_cuda, scene, _abi.BH_ERR_INVALID_ARG, W=W, H=H, ss=2)


@pytest.mark.parametrize("what", ["layout", "shard_count", "pair", "persistent", "dbg_n_rk", "dbg_fate", "dbg_steps"])
def test_refuses_what_the_resolve_does_not_cover(torch_cuda, scene, what):
    torch = torch_cuda
    W, H = 40, 24
    kw = {"layout": dict(layout=bh.BH_LAYOUT_TILES),
          "shard_count": dict(shard_count=2, shard_index=1),
          "pair": dict(schedule=bh.BH_SCHED_PAIR),
          "persistent": dict(schedule=bh.BH_SCHED_PERSISTENT),
          "dbg_n_rk": dict(dbg_n_rk=torch.zeros((H, W), dtype=torch.int16, device="cuda")),
          "dbg_fate": dict(dbg_fate=torch.zeros((H, W), dtype=torch.uint8, device="cuda")),
          "dbg_steps": dict(dbg_steps=torch.zeros((H, W), dtype=torch.int16, device="cuda"))}[what]
    _refused(torch, scene, _abi.BH_ERR_UNSUPPORTED, sentence=True, **kw)
    for t in kw.values():
        if hasattr(t, "cpu"):
            assert not t.cpu().numpy().any()


def test_refuses_a_partition(torch_cuda, scene):
    torch = torch_cuda
    W, H = 40, 24
    part = bh.Partition(W, H, [1])
    try:
        scene.camera_uniform, scene.uniforms = camera_uniform("E", W, H), uniforms()
        col = target(torch, W, H, bh.BH_OUT_RGBA32F)
        d = scene._desc(col, None, bh.BH_OUT_RGBA32F, None, None, None, bh.BH_LAYOUT_ROWMAJOR, 0, 1, W, H, 0, None)
        d.partition = part.handle
        st = scene.lib.bh_render_ss(scene._ctx, C.byref(scene.camera_uniform.c), C.byref(scene.uniforms.to_c()),
                                    C.byref(d), 2, torch.cuda.current_stream().cuda_stream)
        assert st == _abi.BH_ERR_UNSUPPORTED
        assert scene.lib.bh_last_error().decode().startswith("bh_render_ss")
        torch.cuda.synchronize()
        assert (as_bytes(col) == SENTINEL).all()
    finally:
        part.close()


def test_static_order_flag_is_allowed(torch_cuda, scene):
    W, H, k = 13, 7, 4
    rc, rb = reference("E", W, H, k)
    gc, gb = render_ss(torch_cuda, scene, "E", W, H, k, schedule=bh.BH_SCHED_TILE | bh.BH_SCHED_FLAG_STATIC_ORDER)
    assert_frame(gc, expected_bytes(bh.BH_OUT_RGBA32F, rc), "col")
    assert_frame(gb, expected_bytes(bh.BH_OUT_RGBA32F, rb), "blackout_col")
