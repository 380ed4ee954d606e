"""Ray-map renders on the GPU (bh_render_rays / bh_render_lens_rays; Scene.render_rays, Scene.render_lens(dirs=...)):
every pixel equals the reference of tests/_rays_ref.py -- the CPU oracle's trace_ray of the map's direction,
normalised in numpy -- bit for bit in RGBA32F and as that reference's encode in the other formats; over the
pinhole map the result is the CPU oracle's frame.  The reference is never the GPU's own output; where a test also
compares two GPU results, both have been compared with the reference first."""
import ctypes as C

import numpy as np
import pytest

import black_hole_ray_marching_amd as bh
from black_hole_ray_marching_amd import _abi
from tests import _rays_ref as ref
from tests._cases import camera_uniform, uniforms
from tests._lens_ref import frame, sky
from tests._ss_ref import CAP, FLAGS, expected_bytes, reference as ss_reference, sky_ss

pytestmark = pytest.mark.gpu

DT = {bh.BH_OUT_RGBA32F: "float32", bh.BH_OUT_RGBA16F: "float16", bh.BH_OUT_BGRA8_SRGB: "uint8"}
FMTS = [bh.BH_OUT_RGBA32F, bh.BH_OUT_RGBA16F, bh.BH_OUT_BGRA8_SRGB]
F32 = bh.BH_OUT_RGBA32F
SENTINEL = 0xA5  # every byte of a buffer before a call
GUARD = 64       # pixels (records) after the last one that must keep their sentinels


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def new_scene():
    return bh.Scene(16, 16, sky=sky_ss(), max_iters=CAP, scene_flags=FLAGS, math=bh.BH_MATH_EXACT)


@pytest.fixture(scope="module")
def scene(torch_cuda):
    s = new_scene()
    s.uniforms = uniforms()
    yield s
    s.close()


def guarded(torch, n, bytes_per):
    """n elements of bytes_per bytes and GUARD more, every byte the sentinel -> (the n elements, the guard)"""
    buf = torch.full(((n + GUARD) * bytes_per,), SENTINEL, dtype=torch.uint8, device="cuda")
    return buf[:n * bytes_per], buf[n * bytes_per:]


def target(torch, W, H, fmt):
    body, guard = guarded(torch, W * H, _abi.BYTES_PER_PIXEL[fmt])
    t = body.view(getattr(torch, DT[fmt])).view(H, W, 4)
    t.guard = guard
    return t


def as_bytes(t):
    return t.cpu().numpy().view(np.uint8)


def untouched(*ts):
    return all((as_bytes(t) == SENTINEL).all() for t in ts if t is not None)


def guards_ok(*ts):
    return all((as_bytes(t.guard) == SENTINEL).all() for t in ts if t is not None)


def upload(torch, m):
    return torch.from_numpy(np.array(m, dtype=np.float32, order="C")).cuda()  # a copy: the reference maps are read-only


def render(torch, sc, dirs, pos, W, H, fmt=F32, blackout=True, **kw):
    """(col bytes, blackout bytes or None) of Scene.render_rays into sentinel-filled, guarded targets"""
    col = target(torch, W, H, fmt)
    bo = target(torch, W, H, fmt) if blackout else None
    sc.render_rays(dirs, col, bo, pos=pos, fmt=fmt, width=W, height=H, **kw)
    torch.cuda.synchronize()
    assert guards_ok(col, bo), "the guard region after a target was written"
    return as_bytes(col), None if bo is None else as_bytes(bo)


def assert_frame(got, want, what):
    want = np.ascontiguousarray(want).view(np.uint8).reshape(got.shape)
    bad = (got != want).any(-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ, first at {np.argwhere(bad)[:4].tolist()}"


def assert_formats(torch, sc, dirs, pos, W, H, wc, wb, what, **kw):
    for fmt in FMTS:
        col, bo = render(torch, sc, dirs, pos, W, H, fmt, **kw)
        assert_frame(col, expected_bytes(fmt, wc), f"{what} fmt {fmt} col")
        assert_frame(bo, expected_bytes(fmt, wb), f"{what} fmt {fmt} blackout_col")
        col, bo = render(torch, sc, dirs, pos, W, H, fmt, blackout=False, **kw)
        assert bo is None
        assert_frame(col, expected_bytes(fmt, wc), f"{what} fmt {fmt} col alone")


# ---- identity: the pinhole map is bh_render ------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(13, 7), (40, 24)])
@pytest.mark.parametrize("cam", ["D", "E", "F2", "H"])
def test_pinhole_map_is_the_oracle_frame(torch_cuda, scene, cam, W, H):
    torch = torch_cuda
    cu = camera_uniform(cam, W, H)
    dirs = upload(torch, ref.pinhole_map(cam, W, H))
    wc, wb = frame(cam, W, H, "ctx")
    assert_formats(torch, scene, dirs, cu.pos, W, H, wc, wb, "pinhole")
    # pos defaults to the scene camera's; the dbg outputs are bh_render's
    scene.camera_uniform = cu
    col, bo = target(torch, W, H, F32), target(torch, W, H, F32)
    nrk = torch.zeros((H, W), dtype=torch.int16, device="cuda")
    fate = torch.full((H, W), 0xFF, dtype=torch.uint8, device="cuda")
    scene.render_rays(dirs, col, bo, width=W, height=H, dbg_n_rk=nrk, dbg_fate=fate)
    torch.cuda.synchronize()
    assert_frame(as_bytes(col), wc, "default pos col")
    assert_frame(as_bytes(bo), wb, "default pos blackout_col")
    want_nrk, want_fate = ref.oracle_dbg(cam, W, H)
    assert np.array_equal(fate.cpu().numpy(), want_fate)
    assert np.array_equal(nrk.cpu().numpy().view(np.uint16), want_nrk)


# ---- general maps: the full sphere and the rays no pinhole makes -----------------------------------------------
@pytest.mark.parametrize("W,H", ref.SIZES)
@pytest.mark.parametrize("name", ref.POSITIONS)
def test_general_map(torch_cuda, scene, name, W, H):
    torch = torch_cuda
    wc, wb, _, want_fate, want_nrk = ref.general(name, W, H)
    assert not np.isnan(wc).any()
    dirs = upload(torch, ref.general_map(name, W, H))
    assert_formats(torch, scene, dirs, ref.position(name), W, H, wc, wb, f"general {name}")
    col = target(torch, W, H, F32)
    nrk = torch.zeros((H, W), dtype=torch.int16, device="cuda")
    fate = torch.full((H, W), 0xFF, dtype=torch.uint8, device="cuda")
    scene.render_rays(dirs, col, pos=ref.position(name), width=W, height=H, dbg_n_rk=nrk, dbg_fate=fate)
    torch.cuda.synchronize()
    assert np.array_equal(fate.cpu().numpy(), want_fate)
    assert np.array_equal(nrk.cpu().numpy().view(np.uint16), want_nrk)


# ---- non-finite directions ----------------------------------------------------------------------------------------
def assert_equal_up_to_nan_payload(got_bytes, want, what):
    got = np.ascontiguousarray(got_bytes).view(np.float32).reshape(want.shape)
    g, w = got.view(np.uint32).copy(), np.ascontiguousarray(want).view(np.uint32).copy()
    both = np.isnan(got) & np.isnan(want)
    g[both] = w[both] = 0x7FC00000
    bad = (g != w).any(-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ, first at {np.argwhere(bad)[:4].tolist()}"


@pytest.mark.parametrize("name", ref.POSITIONS)
def test_non_finite_directions(torch_cuda, scene, name):
    """Four rays of an 8 x 8 map are the zero vector, (inf, 0, 0), (nan, 1, 0) and (0, -inf, inf): every pixel is
    trace_ray of the numpy-normalised direction, NaN payloads aside, and nothing outside the targets is written."""
    torch = torch_cuda
    wc, wb, wrec, _, _ = ref.nonfinite(name)
    body, guard = guarded(torch, 8 * 8 * 3, 4)
    dirs = body.view(torch.float32).view(8, 8, 3)
    dirs.copy_(upload(torch, ref.nonfinite_map()))
    col, bo = render(torch, scene, dirs, ref.position(name), 8, 8)
    assert_equal_up_to_nan_payload(col, wc, "col")
    assert_equal_up_to_nan_payload(bo, wb, "blackout_col")
    lens_body, lens_guard = guarded(torch, 8 * 8, 8)
    lens = lens_body.view(torch.float32).view(8, 8, 2)
    scene.render_lens(lens, width=8, height=8, dirs=dirs, pos=ref.position(name))
    torch.cuda.synchronize()
    assert_equal_up_to_nan_payload(as_bytes(lens), wrec, "lens")
    assert (as_bytes(guard) == SENTINEL).all() and (as_bytes(lens_guard) == SENTINEL).all()
    assert np.array_equal(dirs.cpu().numpy().view(np.uint32), ref.nonfinite_map().view(np.uint32)), "the map is an input"


# ---- lens ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", ref.SIZES)
@pytest.mark.parametrize("name", ref.POSITIONS)
def test_lens_of_a_map(torch_cuda, scene, name, W, H):
    torch = torch_cuda
    _, _, wrec, _, _ = ref.general(name, W, H)
    dirs = upload(torch, ref.general_map(name, W, H))
    pos = ref.position(name)
    body, guard = guarded(torch, W * H, 8)
    lens = body.view(torch.float32).view(H, W, 2)
    for order in ("first", "repeated"):
        body.fill_(SENTINEL)
        scene.render_lens(lens, width=W, height=H, dirs=dirs, pos=pos)
        torch.cuda.synchronize()
        got = lens.cpu().numpy().view(np.uint32)
        bad = (got != wrec.view(np.uint32)).any(-1)
        assert not bad.any(), f"{order}: {int(bad.sum())} records differ, first at {np.argwhere(bad)[:4].tolist()}"
        assert (as_bytes(guard) == SENTINEL).all()
    for fmt in FMTS:  # shade of that lens is render_rays of the same map (itself compared with the reference above)
        sc, sb = target(torch, W, H, fmt), target(torch, W, H, fmt)
        scene.shade(lens, sc, sb, fmt=fmt, width=W, height=H)
        torch.cuda.synchronize()
        rc, rb = render(torch, scene, dirs, pos, W, H, fmt)
        assert np.array_equal(as_bytes(sc), rc) and np.array_equal(as_bytes(sb), rb), fmt
    mips = bh.Sky(scene, sky("96x40"), mips=True)
    try:
        sc, sb = target(torch, W, H, F32), target(torch, W, H, F32)
        scene.shade(lens, sc, sb, sky=mips, width=W, height=H, mip=True)
        torch.cuda.synchronize()
        hc, hb = bh.lens_shade_host(wrec, sky("96x40"), mip=True)
        assert_frame(as_bytes(sc), hc, "filtered shade col")
        assert_frame(as_bytes(sb), hb, "filtered shade blackout_col")
    finally:
        mips.close()


# ---- supersampling -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,k", [(13, 7, 2), (13, 7, 4), (5, 3, 8)])
def test_supersampled_equirect(torch_cuda, scene, W, H, k):
    torch = torch_cuda
    for name in ("D", "H"):
        wc, wb = ref.equirect_ss(name, W, H, k)
        dirs = upload(torch, ref.equirect_map(k * W, k * H))
        assert_formats(torch, scene, dirs, ref.position(name), W, H, wc, wb, f"ss {k} {name}", ss=k)


@pytest.mark.parametrize("W,H,k", [(13, 7, 2), (13, 7, 4), (5, 3, 8)])
def test_supersampled_pinhole_is_render_ss(torch_cuda, scene, W, H, k):
    torch = torch_cuda
    cam = "E"
    dirs = upload(torch, ref.pinhole_map(cam, W, H, k))
    wc, wb = ss_reference(cam, W, H, k)
    assert_formats(torch, scene, dirs, camera_uniform(cam, W, H).pos, W, H, wc, wb, f"pinhole ss {k}", ss=k)


# ---- order and state -----------------------------------------------------------------------------------------------
def test_order_and_state(torch_cuda):
    """The bytes do not depend on the dispatch order, the build or what else the stream rendered at this size; a
    plain render keeps its own state; a map rewritten in place gives the new map's frame."""
    torch = torch_cuda
    W, H, name, cam = 40, 24, "D", "D"
    sc = new_scene()
    try:
        sc.uniforms = uniforms()
        sc.camera_uniform = camera_uniform(cam, W, H)
        pos = ref.position(name)
        wc, wb, _, _, _ = ref.general(name, W, H)
        pc, pb = frame(cam, W, H, "ctx")
        dirs = upload(torch, ref.general_map(name, W, H))

        def rays(what, **kw):
            col, bo = render(torch, sc, dirs, pos, W, H, **kw)
            assert_frame(col, wc, f"{what} col")
            assert_frame(bo, wb, f"{what} blackout_col")

        def plain(what):
            col, bo = target(torch, W, H, F32), target(torch, W, H, F32)
            sc.render(col, bo, width=W, height=H)
            torch.cuda.synchronize()
            assert_frame(as_bytes(col), pc, f"{what} col")
            assert_frame(as_bytes(bo), pb, f"{what} blackout_col")

        rays("static order", schedule=bh.BH_SCHED_TILE | bh.BH_SCHED_FLAG_STATIC_ORDER)
        rays("first call (centre-out)")
        rays("second call (learned order)")
        rays("third call (repeated frame)")
        rays("latency build", schedule=bh.BH_SCHED_TILE | bh.BH_SCHED_FLAG_LATENCY)
        rays("issue-order build", schedule=bh.BH_SCHED_TILE | bh.BH_SCHED_FLAG_ISSUE_ORDER)
        plain("a plain render after render_rays")
        plain("its repeat")
        rays("after a plain render of the same size")
        plain("a plain render after that")
        # the same pointer, another map: the repeated-frame key cannot see it, the bytes must
        dirs.copy_(upload(torch, ref.general_map(name, W, H)[::-1].copy()))
        col, bo = render(torch, sc, dirs, pos, W, H)
        assert_frame(col, wc[::-1], "map rewritten in place col")
        assert_frame(bo, wb[::-1], "map rewritten in place blackout_col")
    finally:
        sc.close()


# ---- graph -----------------------------------------------------------------------------------------------------------
def test_graph(torch_cuda):
    """The first call of a key under capture is refused (BH_ERR_UNSUPPORTED) and writes nothing; after one eager call
    a capture of the same call on one stream, replayed twice, gives the eager bytes (the reference's)."""
    torch = torch_cuda
    W, H, name = 40, 24, "D"
    sc = new_scene()
    try:
        sc.uniforms = uniforms()
        pos = ref.position(name)
        wc, wb, _, _, _ = ref.general(name, W, H)
        dirs = upload(torch, ref.general_map(name, W, H))
        small = upload(torch, ref.general_map(name, 13, 7))
        col, bo = target(torch, W, H, F32), target(torch, W, H, F32)
        other = target(torch, 13, 7, F32)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        sc.render_rays(dirs, col, bo, pos=pos, width=W, height=H, stream=s)  # eager, on the stream of the capture
        s.synchronize()
        assert_frame(as_bytes(col), wc, "eager col")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            with pytest.raises(bh.BhError) as e:
                sc.render_rays(small, other, pos=pos, width=13, height=7, stream=s)
            assert e.value.status == _abi.BH_ERR_UNSUPPORTED
            sc.render_rays(dirs, col, bo, pos=pos, width=W, height=H, stream=s)
        for _ in range(2):
            for t in (col, bo):
                t.view(torch.uint8).fill_(SENTINEL)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert_frame(as_bytes(col), wc, "replay col")
            assert_frame(as_bytes(bo), wb, "replay blackout_col")
            assert untouched(other) and guards_ok(col, bo)
        del g
        sc.graph_release()
    finally:
        sc.close()


# ---- refusals --------------------------------------------------------------------------------------------------------
def _desc(W, H, **kw):
    d = _abi.bh_render_desc()
    d.width, d.height, d.max_iters, d.scene_flags = W, H, CAP, FLAGS
    d.format, d.math, d.layout, d.shard_count, d.schedule = F32, bh.BH_MATH_EXACT, bh.BH_LAYOUT_ROWMAJOR, 1, bh.BH_SCHED_TILE
    for k, v in kw.items():
        setattr(d, k, v)
    return d


UNSUPPORTED = ["math", "layout", "shard_count", "partition", "pair", "persistent"]
DBG = ["dbg_n_rk", "dbg_fate", "dbg_steps"]
# what each entry refuses: with ss == 1 the dbg_* outputs are bh_render's (test_general_map); a lens render has no targets
REFUSALS = ([("bh_render_rays", w) for w in UNSUPPORTED] + [("bh_render_rays ss", w) for w in UNSUPPORTED + DBG] +
            [("bh_render_lens_rays", w) for w in UNSUPPORTED + DBG + ["out_col", "out_blackout"]])


@pytest.mark.parametrize("entry,what", REFUSALS)
def test_refuses_unsupported(torch_cuda, scene, what, entry):
    torch = torch_cuda
    W, H = 40, 24
    lens_entry, ss = entry == "bh_render_lens_rays", 2 if entry.endswith("ss") else 1
    dirs = upload(torch, ref.equirect_map(ss * W, ss * H))
    before = dirs.clone()
    col, bo = target(torch, W, H, F32), target(torch, W, H, F32)
    side = torch.full((H, W, 16), SENTINEL, dtype=torch.uint8, device="cuda")
    lens, _ = guarded(torch, W * H, 8)
    part = bh.Partition(W, H, [1]) if what == "partition" else None
    try:
        kw = {"math": dict(math=bh.BH_MATH_FAST), "layout": dict(layout=bh.BH_LAYOUT_TILES),
              "shard_count": dict(shard_count=2, shard_index=1), "partition": dict(partition=part and part.handle),
              "pair": dict(schedule=bh.BH_SCHED_PAIR), "persistent": dict(schedule=bh.BH_SCHED_PERSISTENT),
              "dbg_n_rk": dict(dbg_n_rk=side.data_ptr()), "dbg_fate": dict(dbg_fate=side.data_ptr()),
              "dbg_steps": dict(dbg_steps=side.data_ptr()), "out_col": dict(out_col=side.data_ptr()),
              "out_blackout": dict(out_blackout=side.data_ptr())}[what]
        if not lens_entry:
            kw = dict(out_col=col.data_ptr(), out_blackout=bo.data_ptr(), **kw)
        d = _desc(W, H, **kw)
        pos = (C.c_float * 3)(*ref.position("D"))
        U, stream = C.byref(scene.uniforms.to_c()), torch.cuda.current_stream().cuda_stream
        if lens_entry:
            st = scene.lib.bh_render_lens_rays(scene._ctx, pos, U, C.byref(d), dirs.data_ptr(), lens.data_ptr(), stream)
        else:
            st = scene.lib.bh_render_rays(scene._ctx, pos, U, C.byref(d), dirs.data_ptr(), ss, stream)
        assert st == _abi.BH_ERR_UNSUPPORTED
        text = scene.lib.bh_last_error().decode()
        assert text.startswith(entry.split()[0] + ":") and text.endswith(".") and " " in text
        torch.cuda.synchronize()
        assert untouched(col, bo, side, lens) and torch.equal(dirs, before)
    finally:
        if part is not None:
            part.close()


def test_refuses_invalid_arguments(torch_cuda, scene):
    torch = torch_cuda
    W, H = 40, 24
    dirs = upload(torch, ref.equirect_map(W, H))
    col, bo = target(torch, W, H, F32), target(torch, W, H, F32)
    lens, _ = guarded(torch, W * H, 8)
    pos = (C.c_float * 3)(*ref.position("D"))
    U, stream = C.byref(scene.uniforms.to_c()), torch.cuda.current_stream().cuda_stream
    bad, ctx = _abi.BH_ERR_INVALID_ARG, scene._ctx
    rays, lens_rays = scene.lib.bh_render_rays, scene.lib.bh_render_lens_rays
    d = _desc(W, H, out_col=col.data_ptr(), out_blackout=bo.data_ptr())
    ld = _desc(W, H)
    p, lp = dirs.data_ptr(), lens.data_ptr()
    assert rays(ctx, pos, U, C.byref(d), None, 1, stream) == bad
    assert scene.lib.bh_last_error().decode().startswith("bh_render_rays")
    for off in (1, 2, 3):
        assert rays(ctx, pos, U, C.byref(d), p + off, 1, stream) == bad, off
        assert lens_rays(ctx, pos, U, C.byref(ld), p + off, lp, stream) == bad, off
    assert rays(ctx, None, U, C.byref(d), p, 1, stream) == bad
    assert rays(ctx, pos, None, C.byref(d), p, 1, stream) == bad
    assert rays(ctx, pos, U, None, p, 1, stream) == bad
    assert rays(None, pos, U, C.byref(d), p, 1, stream) == bad
    for ss in (0, 3, 5, 16, 0xFFFFFFFF):
        assert rays(ctx, pos, U, C.byref(d), p, ss, stream) == bad, ss
    for kw in (dict(width=0), dict(height=0), dict(width=65537), dict(max_iters=0), dict(max_iters=65536),
               dict(scene_flags=4), dict(format=3), dict(out_col=None), dict(math=2), dict(schedule=0x800)):
        assert rays(ctx, pos, U, C.byref(_desc(W, H, **{**dict(out_col=col.data_ptr()), **kw})), p, 1, stream) == bad, kw
    for ss, (w, h) in ((2, (32769, 1)), (4, (1, 16385)), (8, (8193, 1))):
        assert rays(ctx, pos, U, C.byref(_desc(w, h, out_col=col.data_ptr())), p, ss, stream) == bad, (ss, w, h)
    assert lens_rays(ctx, pos, U, C.byref(ld), None, lp, stream) == bad
    assert scene.lib.bh_last_error().decode().startswith("bh_render_lens_rays")
    assert lens_rays(ctx, pos, U, C.byref(ld), p, None, stream) == bad
    assert lens_rays(ctx, pos, U, C.byref(ld), p, lp + 4, stream) == bad
    assert lens_rays(ctx, None, U, C.byref(ld), p, lp, stream) == bad
    for kw in (dict(width=0), dict(height=65537), dict(max_iters=0), dict(scene_flags=4)):
        assert lens_rays(ctx, pos, U, C.byref(_desc(W, H, **kw)), p, lp, stream) == bad, kw
    # the Python layer: ss, the map's shape against ss, pos
    for kw in (dict(ss=3), dict(ss=0), dict(ss=2), dict(pos=(1.0, 2.0))):
        with pytest.raises(bh.BhError) as e:
            scene.render_rays(dirs, col, bo, width=W, height=H, **kw)
        assert e.value.status == bad, kw
    with pytest.raises(bh.BhError) as e:
        scene.render_lens(lens.view(torch.float32), width=W, height=H, pos=(0.0, 0.0, -20.0))
    assert e.value.status == bad
    torch.cuda.synchronize()
    assert untouched(col, bo, lens) and guards_ok(col, bo)
    assert rays(ctx, pos, U, C.byref(d), p, 1, stream) == _abi.BH_OK  # the arguments themselves are good
    torch.cuda.synchronize()
    assert not untouched(col) and guards_ok(col, bo)
