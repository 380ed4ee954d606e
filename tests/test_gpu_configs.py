"""Full-size GPU parity of every BASELINE.json configuration, and the multi-GPU transport's two targets.

Each BASELINE config is rendered whole, through the C ABI, and compared with the CPU oracle
(oracle/bh_oracle.c, every host thread) on EVERY pixel: fp32 col and blackout_col bit for bit, n_rk and
fate equal; the timed format of the headline (RGBA16F: the `march_tile_kernel<1u, 3u>` instantiation
the bench times) equals the round-to-nearest-even of the oracle's fp32 words, and BGRA8 its normative
sRGB encode.  BASELINE configs:
  1  256x256,   cap 64,   no surfaces, camera A
  2  1920x1080, cap 256,  disc+markers+sky, camera B
  3  4096x2048, cap 512,  disc+markers+sky, camera A (headline) and B
  4  8192x4096, cap 512,  camera A (the frame the 8-GPU config splits; here on one GPU and as 8 shards)
  5  4096x2048, cap 1000, camera C
"""
import numpy as np
import pytest

import black_hole_ray_marching_amd as bh
import oracle
from tests._cases import camera_uniform, uniforms

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module")
def sky_full():
    return bh.synthetic_sky()  # the bench's 4096x2048 sky


DT = {bh.BH_OUT_RGBA32F: "float32", bh.BH_OUT_RGBA16F: "float16", bh.BH_OUT_BGRA8_SRGB: "uint8"}


def expected_bytes(fmt, x):
    """The bytes `fmt` stores for the oracle's fp32 RGBA image x."""
    if fmt == bh.BH_OUT_RGBA32F:
        return x.view(np.uint8)
    if fmt == bh.BH_OUT_RGBA16F:
        return x.astype(np.float16).view(np.uint8)
    e = oracle.srgb_encode(x[..., :3])
    return np.stack([e[..., 2], e[..., 1], e[..., 0], np.full(e.shape[:2], 255, np.uint8)], -1)


def render_full(torch, scene, W, H, fmt, dbg=False, schedule=0):
    dt = getattr(torch, DT[fmt])
    col = torch.zeros((H, W, 4), dtype=dt, device="cuda")
    bo = torch.zeros((H, W, 4), dtype=dt, device="cuda")
    kw = {}
    if dbg:
        kw = dict(dbg_n_rk=torch.zeros((H, W), dtype=torch.int16, device="cuda"),
                  dbg_fate=torch.full((H, W), 0xFF, dtype=torch.uint8, device="cuda"))
    scene.render(col, bo, fmt=fmt, schedule=schedule, **kw)
    torch.cuda.synchronize()
    out = [col.cpu().numpy(), bo.cpu().numpy()]
    if dbg:
        out += [kw["dbg_n_rk"].cpu().numpy().view(np.uint16), kw["dbg_fate"].cpu().numpy()]
    return out


CONFIGS = [
    # id, W, H, cap, camera, scene flags, formats checked besides RGBA32F
    ("c1_256x256_cap64_nosurf_A", 256, 256, 64, "A", 0, [bh.BH_OUT_RGBA16F]),
    ("c2_1920x1080_cap256_B", 1920, 1080, 256, "B", 3, [bh.BH_OUT_RGBA16F, bh.BH_OUT_BGRA8_SRGB]),
    ("c3_4096x2048_cap512_A_headline", 4096, 2048, 512, "A", 3, [bh.BH_OUT_RGBA16F, bh.BH_OUT_BGRA8_SRGB]),
    ("c3_4096x2048_cap512_B", 4096, 2048, 512, "B", 3, [bh.BH_OUT_RGBA16F]),
    ("c5_4096x2048_cap1000_C", 4096, 2048, 1000, "C", 3, [bh.BH_OUT_RGBA16F]),
    ("c4_8192x4096_cap512_A_one_gpu", 8192, 4096, 512, "A", 3, [bh.BH_OUT_RGBA16F]),
]


@pytest.mark.parametrize("cid,W,H,cap,cam,flags,fmts", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_full_frame_bitexact(torch_cuda, sky_full, cid, W, H, cap, cam, flags, fmts):
    torch = torch_cuda
    cu, U = camera_uniform(cam, W, H), uniforms()
    scene = bh.Scene(W, H, sky=sky_full, max_iters=cap, scene_flags=flags, math=bh.BH_MATH_EXACT)
    scene.camera_uniform = cu
    oc, ob, on, of = oracle.render_rows(cu.to_bytes(), bytes(U.to_c()), sky_full, W, H, cap, flags)
    # first frame (centre-out order) and second (learned cost order); then both exact builds forced (camera B:
    # photon-sphere rays whose tail steps take the tiny-dt form, bh_march_step.hpp step_bf TINY / step_tail)
    scheds = [0, 0] + ([bh.BH_SCHED_FLAG_ISSUE_ORDER, bh.BH_SCHED_FLAG_LATENCY] if cam == "B" else [])
    for frame, sched in enumerate(scheds):
        gc, gb, gn, gf = render_full(torch, scene, W, H, bh.BH_OUT_RGBA32F, dbg=True, schedule=sched)
        assert np.array_equal(gf, of), f"{cid} frame {frame}: fate mismatch at {np.argwhere(gf != of)[:5]}"
        assert np.array_equal(gn, on), f"{cid} frame {frame}: n_rk mismatch at {np.argwhere(gn != on)[:5]}"
        bad = gc.view(np.uint32) != oc.view(np.uint32)
        assert not bad.any(), f"{cid} frame {frame}: col mismatch at {np.argwhere(bad)[:5]}"
        assert np.array_equal(gb.view(np.uint32), ob.view(np.uint32)), f"{cid}: blackout_col"
    for fmt in fmts:
        gc, gb = render_full(torch, scene, W, H, fmt)
        assert np.array_equal(gc.view(np.uint8), expected_bytes(fmt, oc)), f"{cid} fmt {fmt}: col"
        assert np.array_equal(gb.view(np.uint8), expected_bytes(fmt, ob)), f"{cid} fmt {fmt}: blackout_col"
    # size-independent properties: alpha 1, n_rk within the cap, fates valid
    assert int(on.max()) <= cap and of.max() <= 3
    scene.close()


def _shards_rgbm(torch, scene, W, H, S, fmt, schedule):
    """Every shard rendered in BH_LAYOUT_TILES_RGBM (col only, blackout None: what a rank ships),
    concatenated as the gather produces them."""
    tb = bh.tile_bytes(bh.BH_LAYOUT_TILES_RGBM, fmt)
    stride = max(bh.shard_tile_count(W, H, k, S) for k in range(S))
    packed = torch.zeros((S * stride, tb), dtype=torch.uint8, device="cuda")
    for k in range(S):
        n = bh.shard_tile_count(W, H, k, S)
        scene.render(packed[k * stride:k * stride + n], None, fmt=fmt, layout=bh.BH_LAYOUT_TILES_RGBM,
                     shard_index=k, shard_count=S, width=W, height=H, schedule=schedule)
    return packed, stride


@pytest.mark.parametrize("schedule", [bh.BH_SCHED_TILE, bh.BH_SCHED_PAIR])
@pytest.mark.parametrize("fmt", [bh.BH_OUT_RGBA32F, bh.BH_OUT_RGBA16F, bh.BH_OUT_BGRA8_SRGB])
@pytest.mark.parametrize("S", [2, 3, 8])
def test_rgbm_shards_unpack_both_targets(torch_cuda, sky_full, S, fmt, schedule):
    """VERDICT r01 "Next round" 4: the multi-GPU frame carries both Scene::render targets.  Ranks ship
    col only (RGBM: RGB planes + the per-tile blackout mask); rank 0's bh_tiles_unpack_rgbm restores
    col AND blackout_col, equal bit for bit to a single-GPU two-target render, throttled or not."""
    torch = torch_cuda
    W, H = 200, 104  # 25 x 13 tiles (test_rgbm_partial_tiles_and_mask_word covers partial ones)
    dt = getattr(torch, DT[fmt])
    scene = bh.Scene(W, H, sky=sky_full, max_iters=512, math=bh.BH_MATH_EXACT)
    scene.camera_uniform = camera_uniform("D", W, H)
    ref_c = torch.zeros((H, W, 4), dtype=dt, device="cuda")
    ref_b = torch.zeros_like(ref_c)
    scene.render(ref_c, ref_b, fmt=fmt)
    packed, stride = _shards_rgbm(torch, scene, W, H, S, fmt, schedule)
    for rows in (0, 3):
        out_c = torch.full((H, W, 4), 7, dtype=dt, device="cuda")
        out_b = torch.full((H, W, 4), 7, dtype=dt, device="cuda")
        bh.tiles_unpack_rgbm(packed, out_c, out_b, W, H, S, stride, fmt, rows_in_flight=rows)
        torch.cuda.synchronize()
        assert torch.equal(out_c.view(torch.uint8), ref_c.view(torch.uint8)), f"col, rows={rows}"
        assert torch.equal(out_b.view(torch.uint8), ref_b.view(torch.uint8)), f"blackout, rows={rows}"
    # Option::None for the blackout target: col alone
    out_c = torch.zeros((H, W, 4), dtype=dt, device="cuda")
    bh.tiles_unpack_rgbm(packed, out_c, None, W, H, S, stride, fmt)
    torch.cuda.synchronize()
    assert torch.equal(out_c.view(torch.uint8), ref_c.view(torch.uint8))
    scene.close()


def _shards_rgbm14(torch, scene, W, H, S, schedule, partition=None):
    """Every shard rendered in BH_LAYOUT_TILES_RGBM14 (RGBA16F col only), concatenated as the gather
    produces them."""
    tb = bh.tile_bytes(bh.BH_LAYOUT_TILES_RGBM14, bh.BH_OUT_RGBA16F)
    counts = partition.counts if partition else [bh.shard_tile_count(W, H, k, S) for k in range(S)]
    stride = max(counts)
    packed = torch.zeros((S * stride, tb), dtype=torch.uint8, device="cuda")
    for k in range(S):
        if counts[k] == 0:  # a weight-0 rank renders nothing
            continue
        kw = dict(partition=partition) if partition else {}
        scene.render(packed[k * stride:k * stride + counts[k]], None, fmt=bh.BH_OUT_RGBA16F,
                     layout=bh.BH_LAYOUT_TILES_RGBM14, shard_index=k, shard_count=S, width=W, height=H,
                     schedule=schedule, **kw)
    return packed, stride


@pytest.mark.parametrize("schedule", [bh.BH_SCHED_TILE, bh.BH_SCHED_PAIR])
@pytest.mark.parametrize("S", [1, 2, 3, 8])
@pytest.mark.parametrize("cam", ["A", "D"])
def test_rgbm14_shards_unpack_both_targets(torch_cuda, sky_full, S, schedule, cam):
    """The 14-bit transport (BH_LAYOUT_TILES_RGBM14, 5.375 B/pixel): every RGBA16F channel of the march is
    an fp16 in [0, 1], so rank 0's unpack with BH_UNPACK_RGBM14 restores col and blackout_col equal bit
    for bit to a single-GPU two-target render (frames with sky, disc, markers, shadow and partial
    tiles)."""
    torch = torch_cuda
    W, H = 204, 100  # partial edge tiles
    scene = bh.Scene(W, H, sky=sky_full, max_iters=512, math=bh.BH_MATH_EXACT)
    scene.camera_uniform = camera_uniform(cam, W, H)
    ref_c = torch.zeros((H, W, 4), dtype=torch.float16, device="cuda")
    ref_b = torch.zeros_like(ref_c)
    scene.render(ref_c, ref_b, fmt=bh.BH_OUT_RGBA16F)
    packed, stride = _shards_rgbm14(torch, scene, W, H, S, schedule)
    for rows in (0, 3):
        out_c = torch.full((H, W, 4), 7, dtype=torch.float16, device="cuda")
        out_b = torch.full_like(out_c, 7)
        bh.tiles_unpack_rgbm(packed, out_c, out_b, W, H, S, stride, bh.BH_OUT_RGBA16F | bh.BH_UNPACK_RGBM14,
                             rows_in_flight=rows)
        torch.cuda.synchronize()
        assert torch.equal(out_c.view(torch.uint8), ref_c.view(torch.uint8)), f"col, rows={rows}"
        assert torch.equal(out_b.view(torch.uint8), ref_b.view(torch.uint8)), f"blackout, rows={rows}"
    # the host mirror of the unpack reads the same bytes
    from black_hole_ray_marching_amd import multigpu
    c, b = multigpu.unpack_rgbm14_numpy(packed.cpu().numpy(), W, H, S, stride)
    assert np.array_equal(c.view(np.uint16), ref_c.cpu().numpy().view(np.uint16))
    assert np.array_equal(b.view(np.uint16), ref_b.cpu().numpy().view(np.uint16))
    scene.close()


@pytest.mark.parametrize("weights", [[3, 4], [16, 20, 20, 20, 20, 20, 20, 20], [0, 5, 7]])
def test_rgbm14_partition_shards_unpack_both_targets(torch_cuda, sky_full, weights):
    """RGBM14 shards of weighted partitions (rank 0 lighter, a rank with weight 0) unpack with
    bh_tiles_unpack_rgbm_partition to both targets of a single-GPU render, bit for bit."""
    torch = torch_cuda
    W, H = 256, 128
    scene = bh.Scene(W, H, sky=sky_full, max_iters=512, math=bh.BH_MATH_EXACT)
    ref_c = torch.zeros((H, W, 4), dtype=torch.float16, device="cuda")
    ref_b = torch.zeros_like(ref_c)
    scene.render(ref_c, ref_b, fmt=bh.BH_OUT_RGBA16F)
    part = bh.Partition(W, H, weights)
    packed, stride = _shards_rgbm14(torch, scene, W, H, len(weights), bh.BH_SCHED_TILE, part)
    out_c = torch.zeros_like(ref_c)
    out_b = torch.zeros_like(ref_c)
    bh.tiles_unpack_rgbm_partition(packed, out_c, out_b, part, stride, bh.BH_OUT_RGBA16F | bh.BH_UNPACK_RGBM14)
    torch.cuda.synchronize()
    assert torch.equal(out_c.view(torch.uint8), ref_c.view(torch.uint8))
    assert torch.equal(out_b.view(torch.uint8), ref_b.view(torch.uint8))
    part.close()
    scene.close()


def test_rgbm14_needs_rgba16f(torch_cuda, sky_small):
    torch = torch_cuda
    scene = bh.Scene(16, 16, sky=sky_small)
    buf = torch.zeros((64, 392), dtype=torch.uint8, device="cuda")
    for fmt in (bh.BH_OUT_RGBA32F, bh.BH_OUT_BGRA8_SRGB):
        with pytest.raises(bh.BhError):
            scene.render(buf, None, fmt=fmt, layout=bh.BH_LAYOUT_TILES_RGBM14, shard_index=0, shard_count=2)
    scene.close()


def test_rgbm_partial_tiles_and_mask_word(torch_cuda, sky_small):
    """Partial edge tiles (100 x 52): the mask bits of pixels outside the frame are clear, and each
    tile's mask word equals the blackout decision of the fp32 render (dot(col, col) < 1)."""
    torch = torch_cuda
    W, H, S = 100, 52, 3
    scene = bh.Scene(W, H, sky=sky_small, max_iters=512, math=bh.BH_MATH_EXACT)
    scene.camera_uniform = camera_uniform("D", W, H)
    c32 = torch.zeros((H, W, 4), device="cuda")
    scene.render(c32, None)
    packed, stride = _shards_rgbm(torch, scene, W, H, S, bh.BH_OUT_RGBA16F, bh.BH_SCHED_TILE)
    torch.cuda.synchronize()
    c = c32.cpu().numpy()
    zero = ((c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1]) + c[..., 2] * c[..., 2]) < 1.0
    from black_hole_ray_marching_amd import multigpu
    p = packed.cpu().numpy()
    lane = np.arange(64)
    for k in range(S):
        for t, (tx, ty) in enumerate(multigpu.shard_tiles(W, H, k, S)):
            m = int(p[k * stride + t, 384:392].view(np.uint64)[0])
            px, py = tx * 8 + (lane & 7), ty * 8 + (lane >> 3)
            ok = (px < W) & (py < H)
            want = sum(1 << int(i) for i in lane[ok] if zero[py[i], px[i]])
            assert m == want, (k, t, hex(m), hex(want))
    scene.close()


def test_rgbm_rejects_the_persistent_schedule(torch_cuda, sky_small):
    torch = torch_cuda
    scene = bh.Scene(16, 16, sky=sky_small)
    buf = torch.zeros((64, 392), dtype=torch.uint8, device="cuda")
    with pytest.raises(bh.BhError, match="unsupported"):
        scene.render(buf, None, fmt=bh.BH_OUT_RGBA16F, layout=bh.BH_LAYOUT_TILES_RGBM, shard_index=0, shard_count=2,
                     schedule=bh.BH_SCHED_PERSISTENT)
    scene.close()


def test_config4_frame_as_eight_shards(torch_cuda, sky_full):
    """BASELINE config 4's frame (8192 x 4096, cap 512, camera A) as the 8-GPU bench splits it, the
    shards rendered one after another on this GPU: rank 0's unpack of the RGBM shards equals the
    single-GPU two-target render bit for bit (RGBA16F, the timed format)."""
    torch = torch_cuda
    W, H, S, fmt = 8192, 4096, 8, bh.BH_OUT_RGBA16F
    scene = bh.Scene(W, H, sky=sky_full, max_iters=512, math=bh.BH_MATH_EXACT)
    ref_c, ref_b = (torch.from_numpy(x).cuda() for x in render_full(torch, scene, W, H, fmt))
    packed, stride = _shards_rgbm(torch, scene, W, H, S, fmt, bh.BH_SCHED_TILE)
    out_c = torch.zeros((H, W, 4), dtype=torch.float16, device="cuda")
    out_b = torch.zeros_like(out_c)
    bh.tiles_unpack_rgbm(packed, out_c, out_b, W, H, S, stride, fmt, rows_in_flight=16)
    torch.cuda.synchronize()
    assert torch.equal(out_c.view(torch.uint8), ref_c.view(torch.uint8))
    assert torch.equal(out_b.view(torch.uint8), ref_b.view(torch.uint8))
    scene.close()


def test_renders_on_two_streams_keep_separate_order_state(torch_cuda, sky_small):
    """include/bh_render.h: the temporal dispatch order is kept per (geometry, shard, stream), so frames
    in flight on two streams of one ctx never share cost buffers or counters; results are unchanged."""
    torch = torch_cuda
    W, H = 256, 128
    scene = bh.Scene(W, H, sky=sky_small, max_iters=512, math=bh.BH_MATH_EXACT)
    ref = torch.zeros((H, W, 4), device="cuda")
    scene.render(ref, None, schedule=bh.BH_SCHED_TILE | bh.BH_SCHED_FLAG_STATIC_ORDER)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [torch.zeros((H, W, 4), device="cuda") for _ in range(8)]
    for i, o in enumerate(outs):
        scene.render(o, None, stream=streams[i % 2])
    torch.cuda.synchronize()
    for o in outs:
        assert torch.equal(o.view(torch.int32), ref.view(torch.int32))
    scene.close()


@pytest.mark.parametrize("layout,S", [(bh.BH_LAYOUT_ROWMAJOR, 1), (bh.BH_LAYOUT_TILES_RGBM, 3)])
@pytest.mark.parametrize("n", [1, 2, 5, 8, 32, 33, 100, bh.BH_MAX_FRAMES])
def test_render_frames_equals_single_renders(torch_cuda, sky_small, n, layout, S):
    """bh_render_frames: n frames with DIFFERENT cameras in one launch (tiles interleaved across frames),
    each frame's targets and debug counters identical to its own bh_render, and to the oracle.  Up to
    32 frames travel in the kernel argument, more through the stream's device frame table."""
    torch = torch_cuda
    W, H, cap = 96, 64, 512
    names = [["A", "B", "C", "D", "E"][i % 5] for i in range(n)]
    scene = bh.Scene(W, H, sky=sky_small, max_iters=cap, math=bh.BH_MATH_EXACT)
    cams = [camera_uniform(c, W, H) for c in names]
    if layout == bh.BH_LAYOUT_ROWMAJOR:
        shape, nt = (H, W, 4), None
        mk = lambda: torch.full(shape, float("nan"), device="cuda")  # noqa: E731
        dshape = (H, W)
        kw = {}
    else:
        nt = bh.shard_tile_count(W, H, 1, S)
        mk = lambda: torch.zeros((nt, bh.tile_bytes(layout, bh.BH_OUT_RGBA32F)), dtype=torch.uint8, device="cuda")  # noqa: E731
        dshape = (nt * 64,)
        kw = dict(layout=layout, shard_index=1, shard_count=S)
    outs, bos = [mk() for _ in cams], [mk() for _ in cams]
    nrk = [torch.zeros(dshape, dtype=torch.int16, device="cuda") for _ in cams]
    for rep in range(2):  # second launch: learned order from frame 0
        scene.render_frames(outs, bos, cameras=cams, dbg_n_rk=nrk, **kw)
        torch.cuda.synchronize()
        for i, cu in enumerate(cams):
            scene.camera_uniform = cu
            o1, b1, n1 = mk(), mk(), torch.zeros(dshape, dtype=torch.int16, device="cuda")
            scene.render(o1, b1, dbg_n_rk=n1, schedule=bh.BH_SCHED_TILE | bh.BH_SCHED_FLAG_STATIC_ORDER, **kw)
            torch.cuda.synchronize()
            assert torch.equal(outs[i].view(torch.uint8), o1.view(torch.uint8)), (rep, i, names[i])
            assert torch.equal(bos[i].view(torch.uint8), b1.view(torch.uint8)), (rep, i, names[i])
            assert torch.equal(nrk[i], n1), (rep, i)
            if layout == bh.BH_LAYOUT_ROWMAJOR and (i < 5 or i == n - 1):
                o = oracle.render_rows(cu.to_bytes(), bytes(uniforms().to_c()), sky_small, W, H, cap, 3)
                assert np.array_equal(o1.cpu().numpy().view(np.uint32), o[0].view(np.uint32))
    scene.close()


def test_render_frames_rejects_mixed_descs(torch_cuda, sky_small):
    torch = torch_cuda
    scene = bh.Scene(32, 16, sky=sky_small)
    a = [torch.zeros((16, 32, 4), device="cuda") for _ in range(bh.BH_MAX_FRAMES + 1)]
    with pytest.raises(bh.BhError):
        scene.render_frames(a)                       # > BH_MAX_FRAMES
    d = (bh._abi.bh_render_desc * 2)()
    for i in range(2):
        d[i] = scene._desc(a[i], None, bh.BH_OUT_RGBA32F, None, None, None, bh.BH_LAYOUT_ROWMAJOR, 0, 1,
                           None, None, 0, None)
    d[1].max_iters = 7                               # descs must agree but for their pointers
    cu = (bh._abi.bh_camera_uniform * 2)(scene.camera_uniform.c, scene.camera_uniform.c)
    assert scene.lib.bh_render_frames(scene._ctx, 2, cu, __import__("ctypes").byref(scene.uniforms.to_c()), d,
                                      None) == bh._abi.BH_ERR_INVALID_ARG
    scene.close()


# ---- weighted partitions (bh_partition: rank 0 lighter, it also unpacks) ---------------------------

@pytest.mark.parametrize("fmt", [bh.BH_OUT_RGBA32F, bh.BH_OUT_RGBA16F, bh.BH_OUT_BGRA8_SRGB])
@pytest.mark.parametrize("weights", [[1, 2], [18, 20, 20], [16] + [20] * 7, [0, 3, 3, 3], [5, 1, 7]])
def test_partition_shards_unpack_both_targets(torch_cuda, sky_full, weights, fmt):
    """Shards of a weighted partition, rendered in BH_LAYOUT_TILES_RGBM (col only) several frames per
    launch, unpack with bh_tiles_unpack_rgbm_partition to both targets of a single-GPU render, bit for
    bit; each shard's tiles are exactly its share of the host map (bh_partition_map)."""
    torch = torch_cuda
    from black_hole_ray_marching_amd import multigpu
    W, H = 200, 100  # 25 x 13 tiles, a partial bottom tile row
    S = len(weights)
    dt = getattr(torch, DT[fmt])
    scene = bh.Scene(W, H, sky=sky_full, max_iters=512, math=bh.BH_MATH_EXACT)
    cams = [camera_uniform(c, W, H) for c in ("D", "A")]
    part = bh.Partition(W, H, weights)
    owner, _ = bh.partition_map(W, H, weights)
    assert part.counts == [int((owner == k).sum()) for k in range(S)]
    assert part.counts == [len(multigpu.shard_tiles(W, H, k, S, weights)) for k in range(S)]
    tb = bh.tile_bytes(bh.BH_LAYOUT_TILES_RGBM, fmt)
    stride = max(part.counts)
    D = len(cams)
    packed = torch.zeros((S * D * stride, tb), dtype=torch.uint8, device="cuda")
    for rep in range(2):  # the second launch runs the learned order of the partition's shards
        for k in range(S):
            if part.counts[k] == 0:
                continue
            blk = packed[k * D * stride:(k + 1) * D * stride]
            frames = [blk[f * stride:f * stride + part.counts[k]] for f in range(D)]
            kw = dict(fmt=fmt, layout=bh.BH_LAYOUT_TILES_RGBM, shard_index=k, shard_count=S, partition=part)
            if rep == 0:
                scene.render_frames(frames, None, cameras=cams, **kw)
            else:  # the bench's N > 1 launches: a prepared call (Scene.prepare_frames)
                scene.prepare_frames(frames, None, **kw).render(cameras=cams)
    for f, cu in enumerate(cams):
        scene.camera_uniform = cu
        ref_c = torch.zeros((H, W, 4), dtype=dt, device="cuda")
        ref_b = torch.zeros_like(ref_c)
        scene.render(ref_c, ref_b, fmt=fmt)
        out_c = torch.full((H, W, 4), 7, dtype=dt, device="cuda")
        out_b = torch.full((H, W, 4), 7, dtype=dt, device="cuda")
        bh.tiles_unpack_rgbm_partition(packed[f * stride:], out_c, out_b, part, D * stride, fmt, rows_in_flight=3)
        torch.cuda.synchronize()
        assert torch.equal(out_c.view(torch.uint8), ref_c.view(torch.uint8)), (weights, f)
        assert torch.equal(out_b.view(torch.uint8), ref_b.view(torch.uint8)), (weights, f)
    part.close()
    scene.close()


def test_partition_replaced_keeps_its_own_order_state(torch_cuda, sky_small):
    """A partition destroyed and another created in its place (the allocator may hand out the same
    address) never inherits the first one's temporal-order state: the state is keyed by the
    partition's serial and the shard's tile count, so a larger shard gets buffers of its own size."""
    torch = torch_cuda
    W, H = 96, 64
    scene = bh.Scene(W, H, sky=sky_small, max_iters=512, math=bh.BH_MATH_EXACT)
    fmt = bh.BH_OUT_RGBA16F
    tb = bh.tile_bytes(bh.BH_LAYOUT_TILES_RGBM, fmt)
    ref_c = torch.zeros((H, W, 4), dtype=torch.float16, device="cuda")
    ref_b = torch.zeros_like(ref_c)
    scene.render(ref_c, ref_b, fmt=fmt)
    for weights in ([5, 1], [1, 5], [1, 1], [1, 7]):  # shard 1 grows from the first partition to the next
        part = bh.Partition(W, H, weights)
        stride = max(part.counts)
        packed = torch.zeros((2 * stride, tb), dtype=torch.uint8, device="cuda")
        for rep in range(2):  # the second render runs the learned order
            for k in range(2):
                scene.render(packed[k * stride:k * stride + part.counts[k]], None, fmt=fmt,
                             layout=bh.BH_LAYOUT_TILES_RGBM, shard_index=k, shard_count=2, partition=part)
        out_c = torch.full_like(ref_c, 7)
        out_b = torch.full_like(ref_c, 7)
        bh.tiles_unpack_rgbm_partition(packed, out_c, out_b, part, stride, fmt)
        torch.cuda.synchronize()
        assert torch.equal(out_c.view(torch.uint8), ref_c.view(torch.uint8)), weights
        assert torch.equal(out_b.view(torch.uint8), ref_b.view(torch.uint8)), weights
        part.close()
    scene.close()


def test_partition_rejects_mismatches(torch_cuda, sky_small):
    """A partition is bound to its frame size, shard count and the tile schedule; other schedules and
    row-major layouts are refused with a status, never rendered with the wrong map."""
    torch = torch_cuda
    W, H = 96, 64
    scene = bh.Scene(W, H, sky=sky_small, max_iters=64, math=bh.BH_MATH_EXACT)
    part = bh.Partition(W, H, [1, 2])
    buf = torch.zeros((part.counts[1], bh.tile_bytes(bh.BH_LAYOUT_TILES_RGBM, bh.BH_OUT_RGBA16F)), dtype=torch.uint8,
                      device="cuda")
    with pytest.raises(bh.BhError):
        scene.render(buf, None, fmt=bh.BH_OUT_RGBA16F, layout=bh.BH_LAYOUT_TILES_RGBM, shard_index=1, shard_count=2,
                     partition=part, schedule=bh.BH_SCHED_PAIR)
    with pytest.raises(bh.BhError):
        scene.render(buf, None, fmt=bh.BH_OUT_RGBA16F, layout=bh.BH_LAYOUT_TILES_RGBM, shard_index=1, shard_count=3,
                     partition=part)
    other = bh.Partition(W, 56, [1, 2])
    with pytest.raises(bh.BhError):
        scene.render(buf, None, fmt=bh.BH_OUT_RGBA16F, layout=bh.BH_LAYOUT_TILES_RGBM, shard_index=1, shard_count=2,
                     partition=other)
    other.close()
    part.close()
    scene.close()


def test_prepared_frames_equal_render_frames(torch_cuda, sky_small):
    """Scene.prepare_frames + FrameBatch.render (the bench's launches): the first n of the prepared
    frames, each camera its own, equal render_frames' bytes; a batch rejects n outside 1..len."""
    torch = torch_cuda
    W, H = 96, 64
    scene = bh.Scene(W, H, sky=sky_small, max_iters=512, math=bh.BH_MATH_EXACT)
    cams = [camera_uniform(c, W, H) for c in ["A", "B", "C", "D", "E"]]
    mk = lambda: torch.full((H, W, 4), float("nan"), device="cuda")  # noqa: E731
    outs, bos = [mk() for _ in cams], [mk() for _ in cams]
    batch = scene.prepare_frames(outs, bos, fmt=bh.BH_OUT_RGBA32F)
    for n in (5, 3, 1):
        for o in outs + bos:
            o.fill_(float("nan"))
        batch.render(n=n, cameras=cams[:n])
        ro, rb = [mk() for _ in range(n)], [mk() for _ in range(n)]
        scene.render_frames(ro, rb, cameras=cams[:n], fmt=bh.BH_OUT_RGBA32F)
        torch.cuda.synchronize()
        for i in range(n):
            assert torch.equal(outs[i].view(torch.int32), ro[i].view(torch.int32)), (n, i)
            assert torch.equal(bos[i].view(torch.int32), rb[i].view(torch.int32)), (n, i)
        for i in range(n, len(cams)):
            assert torch.isnan(outs[i]).all()  # frames past n are not rendered
    for bad in (0, 6):
        with pytest.raises(bh.BhError):
            batch.render(n=bad)
    with pytest.raises(bh.BhError):
        batch.render(n=2, cameras=cams[:3])
    scene.close()


def test_graph_capture_of_render_frames(torch_cuda, sky_small):
    """bh_render_frames inside a HIP graph: after a first call of the (geometry, stream) key, a launch of
    up to 32 frames (kernel-argument frames) captures and replays to the same bytes; a launch of more
    (the device frame table, staged from a host ring) is refused on a capturing stream with a status
    and launches nothing, so the capture stays valid."""
    torch = torch_cuda
    W, H = 64, 32
    scene = bh.Scene(W, H, sky=sky_small, max_iters=512, math=bh.BH_MATH_EXACT)
    cams = [camera_uniform(c, W, H) for c in ("A", "B")]
    mk = lambda: torch.full((H, W, 4), float("nan"), device="cuda")  # noqa: E731
    outs = [mk() for _ in cams]
    many = [mk() for _ in range(33)]
    s = torch.cuda.Stream()
    scene.render_frames(outs, None, cameras=cams, stream=s)  # allocates this stream's order state
    torch.cuda.synchronize()
    for o in outs:
        o.fill_(float("nan"))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        with pytest.raises(bh.BhError):
            scene.render_frames(many, None, stream=s)
        scene.render_frames(outs, None, cameras=cams, stream=s)
    g.replay()
    torch.cuda.synchronize()
    for o, cu in zip(outs, cams):
        scene.camera_uniform = cu
        ref = mk()
        scene.render(ref, None)
        torch.cuda.synchronize()
        assert torch.equal(o.view(torch.int32), ref.view(torch.int32))
    scene.close()


def test_graph_keeps_its_order_state_past_eviction(torch_cuda, sky_small):
    """Graph contract (include/bh_render.h): a (geometry, shard, stream) key rendered
    under stream capture is never evicted, however many other keys are rendered after it (beyond
    BH_ORDER_STATES), so a replay never touches a freed buffer and renders the same bytes; a key seen for
    the first time on a capturing stream is refused with a status (it would allocate)."""
    torch = torch_cuda
    W, H = 64, 32
    scene = bh.Scene(W, H, sky=sky_small, max_iters=512, math=bh.BH_MATH_EXACT)
    out = torch.full((H, W, 4), float("nan"), device="cuda")
    s = torch.cuda.Stream()
    scene.render(out, None, stream=s)  # allocates this key's order state
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    other = torch.empty((2 * H, 2 * W, 4), device="cuda")
    with torch.cuda.graph(g, stream=s):
        with pytest.raises(bh.BhError):  # a new key under capture: refused, nothing launched
            scene.render(other, None, stream=s, width=2 * W, height=2 * H)
        scene.render(out, None, stream=s)
    # 33 other keys (frame widths) on the same stream: more than BH_ORDER_STATES
    big = torch.empty((H, W + 8 * (bh.BH_ORDER_STATES + 2), 4), device="cuda")
    for k in range(bh.BH_ORDER_STATES + 1):
        w = W + 8 * (k + 1)
        scene.render(big, None, stream=s, width=w, height=H)
    torch.cuda.synchronize()
    out.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    ref = torch.empty_like(out)
    scene.render(ref, None)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))
    scene.close()


def test_clock_probe_samples_the_march_without_changing_it(torch_cuda, sky_small):
    """bh_set_clock_probe: the sampled waves report a plausible shader clock (MHz from s_memtime /
    s_memrealtime), on at least one XCD, and the frame's bytes are those of an unprobed render."""
    torch = torch_cuda
    W, H = 512, 256
    scene = bh.Scene(W, H, sky=sky_small, max_iters=512, math=bh.BH_MATH_EXACT)
    a = torch.empty((H, W, 4), device="cuda")
    b = torch.empty((H, W, 4), device="cuda")
    scene.render(a, a.clone())
    acc = torch.zeros(128, dtype=torch.int64, device="cuda")
    scene.set_clock_probe(acc, 16)
    scene.render(b, b.clone())
    scene.set_clock_probe(None)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    c = bh.clock_mhz(acc.cpu().numpy())
    # clock_end drops a sample whose tick ratio is implausible (a wave preempted and restored on another
    # XCD): most sampled waves count, none beyond the sampled slots
    expected = (W // 8) * (H // 8) // 16
    assert 0.9 * expected <= c["waves"] <= expected, c
    assert 300.0 < c["mhz"] < 3500.0, c
    with pytest.raises(bh.BhError):
        scene.set_clock_probe(acc, 3)  # stride must be a power of two
    scene.close()
