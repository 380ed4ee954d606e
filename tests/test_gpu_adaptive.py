"""Adaptive supersampled render on the GPU (bh_render_adaptive / Scene.render(ss=k, adaptive=T)): the plain
frame, with every 8x8 tile that shows an edge marched again with k x k rays.  The reference is the composition
where(mask, S_ref, P_ref) of tests/_adaptive_ref.py -- the CPU oracle's plain frame, tests/_ss_ref.py's
supersampled reference and the numpy rule -- bit for bit; never the GPU's own output, except in the fast-math
test, which says why."""
import ctypes as C

import numpy as np
import pytest

import black_hole_ray_marching_amd as bh
from black_hole_ray_marching_amd import _abi
from tests._adaptive_ref import CAMS, KS, SIZES, T, composed, pixel_mask, plain, tile_mask
from tests._cases import camera_uniform, uniforms
from tests._gpu_common import FAST_TOL
from tests._ss_ref import CAP, FLAGS, expected_bytes, reference, sky_ss

pytestmark = pytest.mark.gpu

DT = {bh.BH_OUT_RGBA32F: "float32", bh.BH_OUT_RGBA16F: "float16", bh.BH_OUT_BGRA8_SRGB: "uint8"}
SENTINEL = 0xA5  # every byte of a buffer before a render
F32 = bh.BH_OUT_RGBA32F
# refined tiles of the reference masks at T = 0.1, cameras D / E / H (checked on the CPU oracle)
REFINED = {(40, 24, bh.BH_OUT_RGBA32F): (7, 8, 4), (40, 24, bh.BH_OUT_BGRA8_SRGB): (10, 13, 5),
           (44, 27, bh.BH_OUT_RGBA32F): (11, 16, 8), (44, 27, bh.BH_OUT_BGRA8_SRGB): (12, 17, 8)}


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


def tiles(W, H):
    return (H + 7) // 8, (W + 7) // 8


def render_adaptive(torch, scene, cam, W, H, k, t=T, fmt=F32, blackout=True, math=None, **kw):
    """(col bytes, blackout bytes or None, tile mask, refined count) of Scene.render(ss=k, adaptive=t) into
    sentinel-filled buffers"""
    scene.camera_uniform, scene.uniforms = camera_uniform(cam, W, H), uniforms()
    col = target(torch, W, H, fmt)
    bo = target(torch, W, H, fmt) if blackout else None
    mask = torch.full(tiles(W, H), SENTINEL, dtype=torch.uint8, device="cuda")
    count = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    scene.render(col, bo, fmt=fmt, width=W, height=H, ss=k, adaptive=t, tile_mask=mask, refined_tiles=count, math=math, **kw)
    torch.cuda.synchronize()
    return as_bytes(col), None if bo is None else as_bytes(bo), mask.cpu().numpy(), int(count.item())


def assert_frame(got, want, what):
    want = np.ascontiguousarray(want).view(np.uint8).reshape(got.shape)
    bad = (got != want).any(-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ, first at {np.argwhere(bad)[:4].tolist()}"


def assert_composed(got, cam, W, H, k, fmt=F32, t=T, blackout=True, what=""):
    gc, gb, gm, gn = got
    wc, wb, wm = composed(cam, W, H, k, fmt, t, blackout)
    assert np.array_equal(gm, wm), f"{what} tile_mask: got\n{gm}\nwant\n{wm}"
    assert gn == int(wm.sum()), f"{what} refined_tiles"
    assert_frame(gc, wc, f"{what} col")
    if blackout:
        assert_frame(gb, wb, f"{what} blackout_col")


def check_input_conditions(cam, W, H, fmt=F32):
    """What the issue states about the reference masks, asserted so that a degenerate mask cannot hide a failure."""
    m = tile_mask(fmt, *plain(cam, W, H, fmt), T)
    n = int(m.sum())
    if (W, H) == (13, 7):
        assert m.shape == (1, 2) and n == 2, "13x7: both tiles are refined"
        return
    assert 0 < n < m.size, f"{W}x{H}: the reference mask is mixed"
    assert n == REFINED[(W, H, fmt)][CAMS.index(cam)]
    if (W, H) == (44, 27) and cam in ("E", "H") and fmt == F32:
        assert set(m[:, -1].tolist()) == {0, 1} and set(m[-1, :].tolist()) == {0, 1}, \
            "44x27: the partial last tile column and row hold refined and unrefined tiles"


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("cam", CAMS)
def test_oracle_parity(torch_cuda, cam, W, H, k):
    """Both targets, the mask and the count equal the composed reference; a fresh scene, so the first call's
    pass 1 runs in the centre-out order and the second's in the order learned from the first's tile costs."""
    check_input_conditions(cam, W, H)
    sc = new_scene()
    try:
        for order in ("centre-out", "learned"):
            got = render_adaptive(torch_cuda, sc, cam, W, H, k)
            assert_composed(got, cam, W, H, k, what=f"{order} order:")
            if (W, H) == (13, 7):  # everything refined: bh_render_ss outright
                rc, rb = reference(cam, W, H, k)
                assert_frame(got[0], expected_bytes(F32, rc), "col against the supersampled reference")
                assert_frame(got[1], expected_bytes(F32, rb), "blackout_col against the supersampled reference")
    finally:
        sc.close()


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("fmt", [bh.BH_OUT_RGBA16F, bh.BH_OUT_BGRA8_SRGB])
def test_formats_take_the_mask_from_the_encoded_bytes(torch_cuda, scene, fmt, k):
    W, H = 44, 27
    if fmt == bh.BH_OUT_BGRA8_SRGB:
        check_input_conditions("E", W, H, fmt)
        assert not np.array_equal(composed("E", W, H, k, fmt)[2], composed("E", W, H, k, F32)[2]), \
            "the BGRA8 mask differs from the fp32 one: a mask taken before the encode would show"
    assert_composed(render_adaptive(torch_cuda, scene, "E", W, H, k, fmt=fmt), "E", W, H, k, fmt=fmt)


@pytest.mark.parametrize("k", KS)
def test_one_target(torch_cuda, scene, k):
    """out_blackout NULL: col is the composition under the col-only mask; a separately allocated buffer keeps
    its sentinel."""
    W, H = 44, 27
    other = target(torch_cuda, W, H, F32)
    got = render_adaptive(torch_cuda, scene, "E", W, H, k, blackout=False)
    assert got[1] is None
    assert_composed(got, "E", W, H, k, blackout=False)
    assert (as_bytes(other) == SENTINEL).all()


@pytest.mark.parametrize("W,H", [(40, 24), (44, 27)])
def test_nothing_refined(torch_cuda, scene, W, H):
    """T = 3e38: the plain frame, an all-zero mask, a count of 0 -- and pass 2 over an empty list ends."""
    gc, gb, gm, gn = render_adaptive(torch_cuda, scene, "E", W, H, 4, t=3e38)
    pc, pb = plain("E", W, H)
    assert not gm.any() and gn == 0
    assert_frame(gc, pc, "col")
    assert_frame(gb, pb, "blackout_col")


def test_multi_frame(torch_cuda, scene):
    """Three cameras in one render_frames call: each frame against its own reference, masks frame-major."""
    torch = torch_cuda
    W, H, k = 44, 27, 2
    scene.uniforms = uniforms()
    cols = [target(torch, W, H, F32) for _ in CAMS]
    bos = [target(torch, W, H, F32) for _ in CAMS]
    mask = torch.full((len(CAMS),) + tiles(W, H), SENTINEL, dtype=torch.uint8, device="cuda")
    count = torch.full((len(CAMS),), -1, dtype=torch.int32, device="cuda")
    scene.render_frames(cols, bos, cameras=[camera_uniform(c, W, H) for c in CAMS], width=W, height=H, ss=k,
                        adaptive=T, tile_mask=mask, refined_tiles=count)
    torch.cuda.synchronize()
    for i, cam in enumerate(CAMS):
        got = as_bytes(cols[i]), as_bytes(bos[i]), mask[i].cpu().numpy(), int(count[i].item())
        assert_composed(got, cam, W, H, k, what=f"frame {cam}:")


@pytest.mark.parametrize("k", [2, 8])
def test_no_side_effects(torch_cuda, k):
    """After an adaptive call a plain Scene.render(ss=k) and a plain Scene.render of the same size still equal
    their references (no order state of either geometry was disturbed), and so does a second adaptive call."""
    torch = torch_cuda
    W, H = 44, 27
    sc = new_scene()
    try:
        assert_composed(render_adaptive(torch, sc, "E", W, H, k), "E", W, H, k)
        rc, rb = reference("E", W, H, k)
        pc, pb = plain("E", W, H)
        for _ in range(2):  # centre-out, then learned
            c, b = target(torch, W, H, F32), target(torch, W, H, F32)
            sc.render(c, b, width=W, height=H, ss=k)
            torch.cuda.synchronize()
            assert_frame(as_bytes(c), expected_bytes(F32, rc), "ss col")
            assert_frame(as_bytes(b), expected_bytes(F32, rb), "ss blackout_col")
            c, b = target(torch, W, H, F32), target(torch, W, H, F32)
            sc.render(c, b, width=W, height=H)
            torch.cuda.synchronize()
            assert_frame(as_bytes(c), pc, "plain col")
            assert_frame(as_bytes(b), pb, "plain blackout_col")
            assert_composed(render_adaptive(torch, sc, "E", W, H, k), "E", W, H, k)
    finally:
        sc.close()


def test_graph(torch_cuda):
    """After one warm call, an adaptive render captured on a single stream replays into sentinel-filled
    outputs and equals the reference.  In the same capture, the first call of a new size -- and of a size that
    only a plain render has warmed -- is refused with BH_ERR_UNSUPPORTED and leaves its sentinels in place."""
    torch = torch_cuda
    W, H, k = 44, 27, 4
    sc = new_scene()
    try:
        sc.uniforms = uniforms()
        s = torch.cuda.Stream()

        def buffers(w, h):
            return (target(torch, w, h, F32), target(torch, w, h, F32),
                    torch.full(tiles(w, h), SENTINEL, dtype=torch.uint8, device="cuda"),
                    torch.full((1,), -1, dtype=torch.int32, device="cuda"))

        def call(buf, w, h, **kw):
            sc.camera_uniform = camera_uniform("E", w, h)
            sc.render(buf[0], buf[1], width=w, height=h, stream=s, **kw)

        def adaptive(buf, w, h):
            call(buf, w, h, ss=k, adaptive=T, tile_mask=buf[2], refined_tiles=buf[3])

        def untouched(buf):
            return ((as_bytes(buf[0]) == SENTINEL).all() and (as_bytes(buf[1]) == SENTINEL).all() and
                    (buf[2].cpu().numpy() == SENTINEL).all() and int(buf[3].item()) == -1)

        main, new, plain_only = buffers(W, H), buffers(40, 24), buffers(13, 7)
        adaptive(main, W, H)            # the warm call: allocates this (geometry, stream)'s state and work list
        call(plain_only, 13, 7)         # a plain render: the order state alone
        torch.cuda.synchronize()
        for t in plain_only[:2]:
            t.view(torch.uint8).fill_(SENTINEL)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for buf, w, h in ((new, 40, 24), (plain_only, 13, 7)):
                with pytest.raises(bh.BhError) as e:
                    adaptive(buf, w, h)
                assert e.value.status == _abi.BH_ERR_UNSUPPORTED
                assert sc.lib.bh_last_error().decode().startswith("bh_render_adaptive")
            adaptive(main, W, H)
        for _ in range(2):
            for t in main[:2]:
                t.view(torch.uint8).fill_(SENTINEL)
            main[2].fill_(SENTINEL)
            main[3].fill_(-1)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert_composed((as_bytes(main[0]), as_bytes(main[1]), main[2].cpu().numpy(), int(main[3].item())),
                            "E", W, H, k, what="replay:")
            assert untouched(new) and untouched(plain_only)
        del g
        sc.lib.bh_graph_release(sc._ctx)
    finally:
        sc.close()




@pytest.mark.parametrize("k", [2, 4])
def test_fast_math_by_composition(torch_cuda, k):
    """BH_MATH_FAST has no bit-exact oracle, so it is checked by composition on the GPU's own fast frames: the
    mask is the numpy rule over the GPU's fast plain frame, unrefined pixels are that frame's bytes, refined
    pixels are within FAST_TOL of the GPU's fast bh_render_ss (bit equality is expected, printed, and not
    required: the fast build's contraction depends on the surrounding code)."""
    torch = torch_cuda
    W, H = 44, 27
    sc = new_scene(math=bh.BH_MATH_FAST)
    try:
        sc.camera_uniform, sc.uniforms = camera_uniform("E", W, H), uniforms()
        pc, pb, sc_, sb = (target(torch, W, H, F32) for _ in range(4))
        sc.render(pc, pb, width=W, height=H)
        sc.render(sc_, sb, width=W, height=H, ss=k)
        torch.cuda.synchronize()
        pc, pb, sc_, sb = (x.cpu().numpy() for x in (pc, pb, sc_, sb))
        gc, gb, gm, gn = render_adaptive(torch, sc, "E", W, H, k)
        wm = tile_mask(F32, pc, pb, T)
        assert 0 < int(wm.sum()) < wm.size
        assert np.array_equal(gm, wm) and gn == int(wm.sum())
        pm = pixel_mask(wm, W, H)
        for name, g, p, s in (("col", gc, pc, sc_), ("blackout_col", gb, pb, sb)):
            g = g.view(np.float32).reshape(H, W, 4)
            assert np.array_equal(g[~pm].view(np.uint32), p[~pm].view(np.uint32)), f"{name}: unrefined pixels"
            diff = (g[pm].view(np.uint32) != s[pm].view(np.uint32)).any(-1)
            print(f"fast adaptive ss={k} {name}: {int(diff.sum())} of {int(pm.sum())} refined pixels differ in bits "
                  f"from bh_render_ss, max |delta| {float(np.abs(g[pm] - s[pm]).max()):.3e}")
            assert float(np.abs(g[pm] - s[pm]).max()) < FAST_TOL, f"{name}: refined pixels"
    finally:
        sc.close()


def _refused(torch, scene, status, W=40, H=24, ss=2, t=T, sentence=False, **kw):
    """The render raises `status` and launches nothing: outputs, mask and count keep their sentinels."""
    scene.camera_uniform, scene.uniforms = camera_uniform("E", 40, 24), uniforms()
    col, bo = target(torch, W, H, F32), target(torch, W, H, F32)
    mask = torch.full(tiles(W, H), SENTINEL, dtype=torch.uint8, device="cuda")
    count = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    with pytest.raises(bh.BhError) as e:
        scene.render(col, bo, width=W, height=H, ss=ss, adaptive=t, tile_mask=mask, refined_tiles=count, **kw)
    assert e.value.status == status
    if sentence:
        text = scene.lib.bh_last_error().decode()
        assert text.startswith("bh_render_adaptive") and text.endswith(".") and " " in text
    torch.cuda.synchronize()
    assert (as_bytes(col) == SENTINEL).all() and (as_bytes(bo) == SENTINEL).all()
    assert (mask.cpu().numpy() == SENTINEL).all() and int(count.item()) == -1


@pytest.mark.parametrize("ss", [0, 1, 3, 16])
def test_refuses_bad_ss(torch_cuda, scene, ss):
    _refused(torch_cuda, scene, _abi.BH_ERR_INVALID_ARG, ss=ss)


@pytest.mark.parametrize("t", [float("nan"), -1.0, float("inf")])
def test_refuses_bad_thresholds(torch_cuda, scene, t):
    _refused(torch_cuda, scene, _abi.BH_ERR_INVALID_ARG, t=t)


@pytest.mark.parametrize("W,H", [(32769, 1), (1, 32769)])
def test_refuses_a_virtual_frame_above_65536(torch_cuda, scene, W, H):
    _refused(torch_cuda, scene, _abi.BH_ERR_INVALID_ARG, W=W, H=H, ss=2)


@pytest.mark.parametrize("what", ["layout", "shard_count", "pair", "persistent", "dbg_n_rk", "dbg_fate", "dbg_steps"])
def test_refuses_what_bh_render_ss_refuses(torch_cuda, scene, what):
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


def test_refuses_a_partition_and_a_null_desc(torch_cuda, scene):
    torch = torch_cuda
    W, H = 40, 24
    part = bh.Partition(W, H, [1])
    try:
        scene.camera_uniform, scene.uniforms = camera_uniform("E", W, H), uniforms()
        col = target(torch, W, H, F32)
        d = scene._desc(col, None, F32, None, None, None, bh.BH_LAYOUT_ROWMAJOR, 0, 1, W, H, 0, None)
        a = _abi.bh_adaptive_desc()
        a.ss, a.threshold = 2, T
        args = (scene._ctx, C.byref(scene.camera_uniform.c), C.byref(scene.uniforms.to_c()), C.byref(d))
        stream = torch.cuda.current_stream().cuda_stream
        assert scene.lib.bh_render_adaptive(*args, None, stream) == _abi.BH_ERR_INVALID_ARG
        d.partition = part.handle
        assert scene.lib.bh_render_adaptive(*args, C.byref(a), stream) == _abi.BH_ERR_UNSUPPORTED
        assert scene.lib.bh_last_error().decode().startswith("bh_render_adaptive")
        torch.cuda.synchronize()
        assert (as_bytes(col) == SENTINEL).all()
    finally:
        part.close()


def test_schedule_flags_are_allowed(torch_cuda, scene):
    """The BH_SCHED_FLAG_* flags pass through: a static order (no order state in pass 1), and each build of
    the exact kernels in pass 2."""
    W, H, k = 44, 27, 4
    for flag in (bh.BH_SCHED_FLAG_STATIC_ORDER, bh.BH_SCHED_FLAG_ISSUE_ORDER, bh.BH_SCHED_FLAG_LATENCY):
        got = render_adaptive(torch_cuda, scene, "E", W, H, k, schedule=bh.BH_SCHED_TILE | flag)
        assert_composed(got, "E", W, H, k, what=f"schedule flag {flag:#x}:")
