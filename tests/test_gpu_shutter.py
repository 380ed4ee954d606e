"""Shutter render on the GPU (bh_render_shutter / Scene.render_shutter): n cameras per output frame, marched by
the n waves of one workgroup and resolved there, against the CPU oracle's fp32 frame of every camera averaged by
the numpy time tree of tests/_shutter_ref.py and encoded as the format stores it -- bit for bit.  The reference
is never the GPU's own output, except where a test says why."""
import ctypes as C
import functools
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import black_hole_ray_marching_amd as bh
from black_hole_ray_marching_amd import _abi
from tests._cases import camera_uniform, uniforms
from tests._shutter_ref import (CAMERA_SETS, CAP, FLAGS, NS, SIZES, expected_bytes, mixed, reference, samples, sky_ss,
                                sweep, time_tree_np)

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
F32, F16, BGRA8 = bh.BH_OUT_RGBA32F, bh.BH_OUT_RGBA16F, bh.BH_OUT_BGRA8_SRGB
SENTINEL = 0xA5  # every byte of a buffer before a render (an fp32 / fp16 of all-0xA5 bytes is no value a frame holds)
GUARD = 4096     # bytes on either side of a target that no render may touch


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def new_scene(math=bh.BH_MATH_EXACT):
    sc = bh.Scene(16, 16, sky=sky_ss(), max_iters=CAP, scene_flags=FLAGS, math=math)
    sc.uniforms = uniforms()
    return sc


@pytest.fixture(scope="module")
def scene(torch_cuda):
    s = new_scene()
    yield s
    s.close()


class Target:
    """A W x H target of `fmt` inside a sentinel-filled buffer with a guard region on either side; handed to
    the library as a raw device pointer."""

    def __init__(self, torch, W, H, fmt):
        self.shape = (H, W, _abi.BYTES_PER_PIXEL[fmt])
        self.n = W * H * _abi.BYTES_PER_PIXEL[fmt]
        self.buf = torch.full((2 * GUARD + self.n,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.ptr = self.buf.data_ptr() + GUARD

    def reset(self):
        self.buf.fill_(SENTINEL)

    def bytes(self):
        return self.buf[GUARD:GUARD + self.n].cpu().numpy().reshape(self.shape)

    def guards_intact(self):
        b = self.buf.cpu().numpy()
        return bool((b[:GUARD] == SENTINEL).all() and (b[GUARD + self.n:] == SENTINEL).all())

    def untouched(self):
        return bool((self.buf.cpu().numpy() == SENTINEL).all())


def render_shutter(torch, scene, cams, W, H, fmt=F32, blackout=True, **kw):
    """(col bytes, blackout bytes or None) of Scene.render_shutter into guarded, sentinel-filled targets"""
    col = Target(torch, W, H, fmt)
    bo = Target(torch, W, H, fmt) if blackout else None
    scene.render_shutter(col.ptr, None if bo is None else bo.ptr, cameras=list(cams), fmt=fmt, width=W, height=H, **kw)
    torch.cuda.synchronize()
    assert col.guards_intact() and (bo is None or bo.guards_intact()), "a store outside the target"
    return col.bytes(), None if bo is None else bo.bytes()


def assert_frame(got, want_bytes, what):
    want = want_bytes.reshape(got.shape)
    bad = (got != want).any(-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ, first at {np.argwhere(bad)[:4].tolist()}"


def assert_both(got, ref, fmt, what):
    assert_frame(got[0], expected_bytes(fmt, ref[0]), f"{what}: col")
    assert_frame(got[1], expected_bytes(fmt, ref[1]), f"{what}: blackout_col")


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("cams", ["mixed", "sweep"])
def test_oracle_parity(torch_cuda, cams, n, W, H):
    """Both targets bit-equal to the reference, by uint32 compare of RGBA32F: in the centre-out order
    (BH_SCHED_FLAG_STATIC_ORDER), in the order of a fresh state, in the order learned from that call's tile costs
    (a second call on the same stream), and on each build of the exact kernels."""
    cs = CAMERA_SETS[cams](n, W, H)
    ref = reference(cs, W, H)
    sc = new_scene()
    try:
        T = bh.BH_SCHED_TILE
        for what, schedule in (("static order", T | bh.BH_SCHED_FLAG_STATIC_ORDER), ("fresh state", T), ("learned order", T),
                               ("issue-order build", T | bh.BH_SCHED_FLAG_ISSUE_ORDER),
                               ("latency build", T | bh.BH_SCHED_FLAG_LATENCY)):
            got = render_shutter(torch_cuda, sc, cs, W, H, schedule=schedule)
            assert got[0].view(np.uint32).shape == (H, W, 4)
            assert_both(got, ref, F32, what)
    finally:
        sc.close()


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("n", [2, 8])
@pytest.mark.parametrize("k", [2, 4])
def test_composes_with_ss(torch_cuda, scene, k, n, W, H):
    cs = mixed(n, W, H)
    assert_both(render_shutter(torch_cuda, scene, cs, W, H, ss=k), reference(cs, W, H, k), F32, f"ss={k}")


def _encode_then_average(fmt, s):
    """The other order: every sample encoded as `fmt` stores it, the encoded values averaged and stored again."""
    if fmt == F16:
        dec = s.astype(np.float16).astype(np.float32)
        dec[..., 3] = 1.0
        return expected_bytes(fmt, time_tree_np(dec))
    enc = np.stack([expected_bytes(fmt, x) for x in s]).astype(np.float64)
    return np.rint(enc.mean(0)).astype(np.uint8)


@pytest.mark.parametrize("fmt", [F16, BGRA8])
@pytest.mark.parametrize("n", [4, 16])
def test_formats_encode_the_resolved_value(torch_cuda, scene, fmt, n):
    W, H = 40, 24
    cs = mixed(n, W, H)
    ref = reference(cs, W, H)
    # from the reference alone: "encode, then average" gives other bytes somewhere, so the order is what is tested
    other = _encode_then_average(fmt, samples(cs, W, H, 1)[0])
    assert (other.reshape(H, W, -1) != expected_bytes(fmt, ref[0]).reshape(H, W, -1)).any()
    assert_both(render_shutter(torch_cuda, scene, cs, W, H, fmt=fmt), ref, fmt, "resolve, then encode")


@pytest.mark.parametrize("n", NS)
def test_one_target(torch_cuda, scene, n):
    """out_blackout == NULL: col is unchanged, and a separately allocated buffer keeps its sentinel."""
    W, H = 40, 24
    cs = mixed(n, W, H)
    other = Target(torch_cuda, W, H, F32)
    gc, gb = render_shutter(torch_cuda, scene, cs, W, H, blackout=False)
    assert gb is None
    assert_frame(gc, expected_bytes(F32, reference(cs, W, H)[0]), "col")
    assert other.untouched()


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("fmt", [F32, BGRA8])
def test_n_sub_1_is_the_plain_render(torch_cuda, scene, fmt, k):
    """n_sub = 1 is passed on: byte-equal to Scene.render / Scene.render(ss=k) of the same camera."""
    torch = torch_cuda
    W, H = 40, 24
    cu = camera_uniform("E", W, H)
    scene.camera_uniform = cu
    pc, pb = Target(torch, W, H, fmt), Target(torch, W, H, fmt)
    scene.render(pc.ptr, pb.ptr, fmt=fmt, width=W, height=H, ss=k)
    torch.cuda.synchronize()
    gc, gb = render_shutter(torch, scene, [cu], W, H, fmt=fmt, ss=k)
    assert np.array_equal(gc, pc.bytes()) and np.array_equal(gb, pb.bytes())


def _frames_call(torch, scene, sets, W, H, **kw):
    cols = [Target(torch, W, H, F32) for _ in sets]
    bos = [Target(torch, W, H, F32) for _ in sets]
    scene.render_frames_shutter([t.ptr for t in cols], [t.ptr for t in bos], cameras=[list(s) for s in sets],
                                width=W, height=H, **kw)
    torch.cuda.synchronize()
    assert all(t.guards_intact() for t in cols + bos)
    return [(c.bytes(), b.bytes()) for c, b in zip(cols, bos)]


def test_multi_frame(torch_cuda, scene):
    """3 frames x n = 4 in one call, different camera sets per frame: each frame equals its own single-frame call
    (and the reference)."""
    W, H, n = 40, 24, 4
    sets = [mixed(n, W, H), sweep(n, W, H), mixed(n, W, H, first=4)]
    for f, (cs, got) in enumerate(zip(sets, _frames_call(torch_cuda, scene, sets, W, H))):
        single = render_shutter(torch_cuda, scene, cs, W, H)
        assert np.array_equal(got[0], single[0]) and np.array_equal(got[1], single[1]), f"frame {f}"
        assert_both(got, reference(cs, W, H), F32, f"frame {f}")


def test_multi_frame_through_the_device_table(torch_cuda, scene):
    """5 frames x n = 8 (40 cameras: more than travel in the kernel argument) gives the same bytes."""
    W, H, n = 40, 24, 8
    sets = [mixed(n, W, H, first=f) for f in range(4)] + [sweep(n, W, H)]
    for f, (cs, got) in enumerate(zip(sets, _frames_call(torch_cuda, scene, sets, W, H))):
        single = render_shutter(torch_cuda, scene, cs, W, H)
        assert np.array_equal(got[0], single[0]) and np.array_equal(got[1], single[1]), f"frame {f}"
        assert_both(got, reference(cs, W, H), F32, f"frame {f}")


def test_graph(torch_cuda):
    """After a warm call, an n = 4 call captured on a stream replays into sentinel-filled targets to the same
    bytes; in the same capture a call of more than 32 cameras is refused with BH_ERR_UNSUPPORTED and launches
    nothing."""
    torch = torch_cuda
    W, H, n = 40, 24, 4
    cs = mixed(n, W, H)
    many = [mixed(8, W, H, first=f) for f in range(5)]
    sc = new_scene()
    try:
        s = torch.cuda.Stream()
        col, bo = Target(torch, W, H, F32), Target(torch, W, H, F32)
        mcol = [Target(torch, W, H, F32) for _ in many]

        def call():
            sc.render_shutter(col.ptr, bo.ptr, cameras=list(cs), width=W, height=H, stream=s)

        call()  # allocates this (geometry, stream)'s order state
        torch.cuda.synchronize()
        warm = (col.bytes(), bo.bytes())
        assert_both(warm, reference(cs, W, H), F32, "warm call")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            with pytest.raises(bh.BhError) as e:
                sc.render_frames_shutter([t.ptr for t in mcol], None, cameras=[list(m) for m in many], width=W,
                                         height=H, stream=s)
            assert e.value.status == _abi.BH_ERR_UNSUPPORTED
            call()
        for _ in range(2):
            col.reset()
            bo.reset()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(col.bytes(), warm[0]) and np.array_equal(bo.bytes(), warm[1])
            assert col.guards_intact() and bo.guards_intact() and all(t.untouched() for t in mcol)
        del g
        sc.graph_release()
    finally:
        sc.close()


@functools.lru_cache(maxsize=None)
def _fast_frames(torch, W, H):
    """The plain fast-math render's RGBA32F frames (col, blackout_col) of the 8 mixed cameras, fp32 (8, H, W, 4)"""
    sc = new_scene(math=bh.BH_MATH_FAST)
    try:
        out = []
        for cu in mixed(8, W, H):
            sc.camera_uniform = cu
            c, b = Target(torch, W, H, F32), Target(torch, W, H, F32)
            sc.render(c.ptr, b.ptr, width=W, height=H)
            torch.cuda.synchronize()
            out.append((c.bytes().view(np.float32).reshape(H, W, 4), b.bytes().view(np.float32).reshape(H, W, 4)))
        col, bo = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
        assert not np.isnan(col).any() and not np.isnan(bo).any()
        return col, bo
    finally:
        sc.close()


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("n", [2, 8])
def test_fast_math_by_composition(torch_cuda, n, W, H):
    """BH_MATH_FAST has no bit-exact oracle, so it is checked by composition: the shutter render in fast math must
    be bit-equal to the numpy time tree over the GPU's OWN fast-math plain RGBA32F frames of the same cameras.
    This checks the new resolve (and that it takes each sample exactly as the plain kernel stores it) against the
    existing fast march, which the parity tests hold to its tolerance."""
    col, bo = _fast_frames(torch_cuda, W, H)
    sc = new_scene(math=bh.BH_MATH_FAST)
    try:
        got = render_shutter(torch_cuda, sc, mixed(n, W, H), W, H)
    finally:
        sc.close()
    assert_both(got, (time_tree_np(col[:n]), time_tree_np(bo[:n])), F32, "fast math")


REFUSALS = ["layout", "shard_count", "partition", "pair", "persistent", "dbg_n_rk", "dbg_fate", "dbg_steps"]


@pytest.mark.parametrize("what", REFUSALS)
def test_refuses_what_bh_render_ss_refuses(torch_cuda, scene, what):
    """BH_ERR_UNSUPPORTED with a sentence that starts with bh_render_shutter; nothing is launched."""
    torch = torch_cuda
    W, H, n = 40, 24, 2
    col = Target(torch, W, H, F32)
    dbg = torch.zeros((H, W), dtype=torch.int16, device="cuda")
    d = scene._desc(col.ptr, None, F32, None, None, None, bh.BH_LAYOUT_ROWMAJOR, 0, 1, W, H, 0, None)
    part = None
    if what == "layout":
        d.layout = bh.BH_LAYOUT_TILES
    elif what == "shard_count":
        d.shard_count, d.shard_index = 2, 1
    elif what == "partition":
        part = bh.Partition(W, H, [1])
        d.partition = part.handle
    elif what == "pair":
        d.schedule = bh.BH_SCHED_PAIR
    elif what == "persistent":
        d.schedule = bh.BH_SCHED_PERSISTENT
    else:
        setattr(d, what, dbg.data_ptr())
    try:
        cams = (_abi.bh_camera_uniform * n)(*[c.c for c in mixed(n, W, H)])
        st = scene.lib.bh_render_shutter(scene._ctx, n, cams, C.byref(scene.uniforms.to_c()), C.byref(d), 1,
                                         torch.cuda.current_stream().cuda_stream)
        assert st == _abi.BH_ERR_UNSUPPORTED
        text = scene.lib.bh_last_error().decode()
        assert text.startswith("bh_render_shutter") and text.endswith(".") and " " in text
        torch.cuda.synchronize()
        assert col.untouched() and not dbg.cpu().numpy().any()
    finally:
        if part is not None:
            part.close()


@pytest.mark.parametrize("n_frames,n_sub,ss,W,H", [(1, 3, 1, 40, 24), (1, 32, 1, 40, 24), (1, 0, 1, 40, 24),
                                                  (17, 16, 1, 40, 24), (1, 2, 3, 40, 24), (1, 2, 16, 40, 24),
                                                  (1, 2, 2, 32769, 1), (1, 2, 2, 1, 32769)])
def test_refuses_bad_arguments(torch_cuda, scene, n_frames, n_sub, ss, W, H):
    """BH_ERR_INVALID_ARG for n_sub outside {1, 2, 4, 8, 16}, n_frames * n_sub above BH_MAX_FRAMES, and the ss
    and size limits of bh_render_ss; nothing is launched."""
    torch = torch_cuda
    col = Target(torch, 40, 24, F32)
    d = scene._desc(col.ptr, None, F32, None, None, None, bh.BH_LAYOUT_ROWMAJOR, 0, 1, W, H, 0, None)
    descs = (_abi.bh_render_desc * n_frames)(*[d] * n_frames)
    cu = camera_uniform("E", 40, 24)
    cams = (_abi.bh_camera_uniform * max(1, n_frames * n_sub))(*[cu.c] * max(1, n_frames * n_sub))
    st = scene.lib.bh_render_frames_shutter(scene._ctx, n_frames, n_sub, cams, C.byref(scene.uniforms.to_c()), descs, ss,
                                            torch.cuda.current_stream().cuda_stream)
    assert st == _abi.BH_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert col.untouched()


def test_flags_are_allowed(torch_cuda, scene):
    W, H, n = 13, 7, 4
    cs = sweep(n, W, H)
    got = render_shutter(torch_cuda, scene, cs, W, H, ss=2, schedule=bh.BH_SCHED_TILE | bh.BH_SCHED_FLAG_STATIC_ORDER |
                         bh.BH_SCHED_FLAG_LATENCY)
    assert_both(got, reference(cs, W, H, 2), F32, "static order, latency build, ss=2")


def test_render_path_tool(torch_cuda, tmp_path):
    """tools/render_path.py --shutter runs end to end in a child process."""
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "render_path.py"), "--shutter", "4", "--frames", "2",
                        "--width", "40", "--height", "24", "--no-png", "--out", str(tmp_path / "path")],
                       capture_output=True, text=True, timeout=300, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout + r.stderr
    assert '"shutter": 4' in r.stdout
