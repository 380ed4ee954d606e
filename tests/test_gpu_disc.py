"""Hit maps and disc shades on the GPU (bh_render_lens_hits, bh_render_lens_rays_posed_hits, bh_shade_lens_disc;
Scene.render_lens(hits=), Scene.shade(hits=, disc=), bh.Disc), bit for bit against tests/_disc_ref.py: the lens
records and the hits of the CPU oracle's rays, and the numpy restatement of include/bh_render.h's rule over them.  The
reference is never the GPU's own output; where two GPU results are compared (the lens of bh_render_lens, the bytes of
bh_shade_lens) each side is also compared with the reference."""
import ctypes as C

import numpy as np
import pytest

import black_hole_ray_marching_amd as bh
from black_hole_ray_marching_amd import _abi, raymap
from tests import _disc_ref as ref
from tests._cases import uniforms
from tests._ss_ref import expected_bytes, sky_ss

pytestmark = pytest.mark.gpu

DT = {bh.BH_OUT_RGBA32F: "float32", bh.BH_OUT_RGBA16F: "float16", bh.BH_OUT_BGRA8_SRGB: "uint8"}
FMTS = [bh.BH_OUT_RGBA32F, bh.BH_OUT_RGBA16F, bh.BH_OUT_BGRA8_SRGB]
F32 = bh.BH_OUT_RGBA32F
SENTINEL = 0xA5  # every byte of a buffer before a call
GUARD = 64       # records after the last one that must keep their sentinels
BUILDS = [bh.BH_SCHED_FLAG_ISSUE_ORDER, bh.BH_SCHED_FLAG_LATENCY]


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def new_scene():
    return bh.Scene(16, 16, sky=sky_ss(), max_iters=64, scene_flags=3, math=bh.BH_MATH_EXACT)


@pytest.fixture(scope="module")
def scene(torch_cuda):
    s = new_scene()
    s.test_disc = bh.Disc(s, ref.disc_texture(37, 5))
    s.white_disc = bh.Disc(s, ref.white_disc())
    yield s
    s.close()


def buffer(torch, n, words):
    """n elements of `words` floats and GUARD more, every byte the sentinel"""
    return torch.full((n + GUARD, words * 4), SENTINEL, dtype=torch.uint8, device="cuda").view(torch.float32)


def target(torch, W, H, fmt):
    t = torch.full((H, W, _abi.BYTES_PER_PIXEL[fmt]), SENTINEL, dtype=torch.uint8, device="cuda")
    return t.view(getattr(torch, DT[fmt]))


def as_bytes(t):
    return t.cpu().numpy().view(np.uint8)


def untouched(*ts):
    return all((as_bytes(t) == SENTINEL).all() for t in ts if t is not None)


def march(torch, sc, cam, W, H, cap, flags=3, k=1, kind=None, hits=True, **kw):
    """(lens, hits) device tensors (kH, kW, 2 / 3) of one march with the camera uniform of W x H, guards checked.
    kind: None for the pinhole form, "pinhole" / "equirect" for the posed form over that map; hits=False: the call the
    form extends (bh_render_lens, bh_render_lens_rays_posed)."""
    sc.camera_uniform, sc.uniforms = ref.view_uniform(cam, W, H), uniforms()
    sc.max_iters, sc.scene_flags = cap, flags
    n = k * W * k * H
    lens, hit = buffer(torch, n, 2), buffer(torch, n, 3) if hits else None
    if kind is not None:
        assert k == 1
        p = ref.pose_rows(cam, kind)
        pose = raymap.pose(p[0])
        pose.r, pose.u, pose.f = ((C.c_float * 3)(*row.tolist()) for row in p[1:])
        assert np.array_equal(raymap.pose_rows(pose), p)
        kw.update(dirs=torch.from_numpy(ref.ray_map(cam, kind, W, H).copy()).cuda(), pose=pose)
    if hits:
        kw.update(hits=hit[:n].view(k * H, k * W, 3))
    sc.render_lens(lens, width=k * W, height=k * H, **kw)
    torch.cuda.synchronize()
    assert untouched(lens[n:]) and (hit is None or untouched(hit[n:])), "a guard region was written"
    return lens[:n].view(k * H, k * W, 2), None if hit is None else hit[:n].view(k * H, k * W, 3)


def assert_same(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    got, want = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    bad = (got != want).any(-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[:4].tolist()}"


def assert_view(lens, hits, view, what):
    """the lens records and the hit map of a march against the oracle's: final ro where its fate is SURFACE, +0
    (all-zero bits) elsewhere"""
    rec, fate, ro = view
    assert_same(lens, rec, f"{what}: lens")
    assert not ro[fate != bh.BH_FATE_SURFACE].view(np.uint32).any()
    assert_same(hits, ro, f"{what}: hits")


@pytest.mark.parametrize("cam,W,H,cap", ref.FRAMES)
def test_pinhole_hit_map(torch_cuda, cam, W, H, cap):
    """A fresh scene: centre-out order, then the learned order (a repeated frame), then after bh_render_lens of the
    same geometry, whose lens bytes bh_render_lens_hits writes."""
    view = ref.pinhole_view(cam, W, H, cap)
    ref.assert_all_kinds(view, f"{cam} {W}x{H} cap {cap}")
    sc = new_scene()
    try:
        for order in ("centre-out", "learned"):
            assert_view(*march(torch_cuda, sc, cam, W, H, cap), view, order)
        plain, _ = march(torch_cuda, sc, cam, W, H, cap, hits=False)
        assert_same(plain, view[0], "bh_render_lens")
        lens, hits = march(torch_cuda, sc, cam, W, H, cap)
        assert_view(lens, hits, view, "after bh_render_lens")
        assert np.array_equal(as_bytes(lens), as_bytes(plain))
    finally:
        sc.close()


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("flags", ref.FLAG_SETS)
@pytest.mark.parametrize("kind", [None, "pinhole", "equirect"])
def test_hit_map_of_every_form_fold_and_build(torch_cuda, scene, kind, flags, build):
    """The pinhole form and the posed form over raymap.pinhole (unit axes) and raymap.equirect (a turned basis), each
    scene-flag fold, both builds of the kernels; 67x41: partial tiles on both axes."""
    cam, W, H, cap = "DISC_IN", 67, 41, 64
    get = ref.pinhole_view if kind is None else lambda *a: ref.posed_view(a[0], kind, *a[1:])
    ref.assert_all_kinds(get(cam, W, H, cap, 3), f"{kind}: the frame in the reference's scene")
    view = get(cam, W, H, cap, flags)
    lens, hits = march(torch_cuda, scene, cam, W, H, cap, flags, kind=kind, schedule=bh.BH_SCHED_TILE | build)
    assert_view(lens, hits, view, f"{kind} flags {flags} build {build:#x}")


@pytest.mark.parametrize("kind", ["pinhole", "equirect"])
def test_posed_hit_map_long_cap(torch_cuda, scene, kind):
    """cap 256: surface rays that end in the tail's loop (after iteration 48), and bh_render_lens_rays_posed's lens."""
    cam, W, H, cap = "DISC_IN", 64, 40, 256
    view = ref.posed_view(cam, kind, W, H, cap)
    ref.assert_all_kinds(view, kind)
    lens, hits = march(torch_cuda, scene, cam, W, H, cap, kind=kind)
    assert_view(lens, hits, view, kind)
    plain, _ = march(torch_cuda, scene, cam, W, H, cap, kind=kind, hits=False)
    assert np.array_equal(as_bytes(lens), as_bytes(plain))


def shade(torch, sc, lens, hits, W, H, fmt=F32, blackout=True, ss=1, disc=None, **kw):
    col = target(torch, W, H, fmt)
    bo = target(torch, W, H, fmt) if blackout else None
    sc.shade(lens, col, bo, fmt=fmt, ss=ss, width=W, height=H, hits=hits, disc=disc or sc.test_disc, **kw)
    torch.cuda.synchronize()
    return as_bytes(col), None if bo is None else as_bytes(bo)


def assert_frame(got, want, what):
    want = np.ascontiguousarray(want).view(np.uint8).reshape(got.shape)
    bad = (got != want).any(-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ, first at {np.argwhere(bad)[:4].tolist()}"


@pytest.mark.parametrize("cam,W,H,cap,k", [("DISC_IN", 67, 41, 64, 1), ("B", 64, 40, 256, 1), ("DISC_IN", 16, 8, 256, 2),
                                           ("DISC_IN", 16, 8, 64, 4), ("A", 67, 41, 64, 1)])
def test_shade_equals_the_restatement(torch_cuda, scene, cam, W, H, cap, k):
    """Three formats, one and two targets, a turned and brightened disc; the inputs are the reference's records and
    hits, which the march of this view reproduces (asserted first)."""
    torch = torch_cuda
    ref.assert_all_kinds(ref.pinhole_view(cam, W, H, cap), "the output frame")
    view = ref.pinhole_view(cam, W, H, cap, 3, k)
    lens, hits = march(torch, scene, cam, W, H, cap, k=k)
    assert_view(lens, hits, view, "march")
    for spin, gain in ((0.37, 1.0), (-2.5, 4.0)):
        wc, wb = ref.shade_ss(view[0], view[2], sky_ss(), ref.disc_texture(37, 5), k, spin=spin, gain=gain)
        for fmt in FMTS:
            col, bo = shade(torch, scene, lens, hits, W, H, fmt, ss=k, spin=spin, gain=gain)
            assert_frame(col, expected_bytes(fmt, wc), f"spin {spin} fmt {fmt} col")
            assert_frame(bo, expected_bytes(fmt, wb), f"spin {spin} fmt {fmt} blackout_col")
            col, bo = shade(torch, scene, lens, hits, W, H, fmt, blackout=False, ss=k, spin=spin, gain=gain)
            assert bo is None
            assert_frame(col, expected_bytes(fmt, wc), f"spin {spin} fmt {fmt} col alone")


def test_shade_ss8_and_scene_without_disc(torch_cuda, scene):
    torch = torch_cuda
    cam, W, H, cap = "DISC_IN", 16, 8, 64
    view = ref.pinhole_view(cam, W, H, cap, 3, 8)
    lens, hits = march(torch, scene, cam, W, H, cap, k=8)
    assert_view(lens, hits, view, "march")
    wc, wb = ref.shade_ss(view[0], view[2], sky_ss(), ref.disc_texture(37, 5), 8, spin=0.37, gain=1.0)
    col, bo = shade(torch, scene, lens, hits, W, H, ss=8, spin=0.37)
    assert_frame(col, wc, "ss 8 col")
    assert_frame(bo, wb, "ss 8 blackout_col")
    wc, wb = ref.shade_ss(view[0], view[2], sky_ss(), ref.disc_texture(37, 5), 8, spin=0.37, flags=2)
    col, bo = shade(torch, scene, lens, hits, W, H, ss=8, spin=0.37, scene_flags=2)
    assert_frame(col, wc, "markers only: col")
    assert_frame(bo, wb, "markers only: blackout_col")


@pytest.mark.parametrize("k", [1, 2])
def test_identity_white_disc_is_bh_shade_lens(torch_cuda, scene, k):
    """A 1x1 disc of (255, 255, 255) with gain 1 and any spin: bh_shade_lens's bytes for the same lens, which are
    the restatement's."""
    torch = torch_cuda
    cam, W, H, cap = "DISC_IN", 67, 41, 64
    view = ref.pinhole_view(cam, W, H, cap, 3, k)
    ref.assert_all_kinds(view, "the frame")
    lens, hits = march(torch, scene, cam, W, H, cap, k=k)
    for fmt in FMTS:
        pc, pb = target(torch, W, H, fmt), target(torch, W, H, fmt)
        scene.shade(lens, pc, pb, fmt=fmt, ss=k, width=W, height=H)
        torch.cuda.synchronize()
        for spin in (0.0, 0.37, -1000.0):
            col, bo = shade(torch, scene, lens, hits, W, H, fmt, ss=k, disc=scene.white_disc, spin=spin)
            assert np.array_equal(col, as_bytes(pc)) and np.array_equal(bo, as_bytes(pb)), (fmt, spin)
    wc, wb = ref.shade_ss(view[0], view[2], sky_ss(), ref.white_disc(), k, spin=0.37)
    col, bo = shade(torch, scene, lens, hits, W, H, ss=k, disc=scene.white_disc, spin=0.37)
    assert_frame(col, wc, "col")
    assert_frame(bo, wb, "blackout_col")


def test_graph(torch_cuda):
    """bh_shade_lens_disc is capturable from its first call and replays to the same bytes; in the same capture
    bh_render_lens_hits of a geometry never rendered is refused, as bh_render_lens's would be, and writes nothing."""
    torch = torch_cuda
    cam, W, H, cap = "DISC_IN", 67, 41, 64
    sc = new_scene()
    try:
        disc = bh.Disc(sc, ref.disc_texture(37, 5))
        lens, hits = march(torch, sc, cam, W, H, cap)
        new_lens, new_hits = buffer(torch, 16 * 8, 2), buffer(torch, 16 * 8, 3)
        col, bo = target(torch, W, H, F32), target(torch, W, H, F32)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            with pytest.raises(bh.BhError) as e:
                sc.render_lens(new_lens, width=16, height=8, hits=new_hits[:128].view(8, 16, 3), stream=s)
            assert e.value.status == _abi.BH_ERR_UNSUPPORTED
            sc.shade(lens, col, bo, width=W, height=H, hits=hits, disc=disc, spin=0.37, stream=s)
        view = ref.pinhole_view(cam, W, H, cap)
        wc, wb = ref.shade_ss(view[0], view[2], sky_ss(), ref.disc_texture(37, 5), 1, spin=0.37)
        for _ in range(2):
            for t in (col, bo):
                t.view(torch.uint8).fill_(SENTINEL)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert_frame(as_bytes(col), wc, "replay: col")
            assert_frame(as_bytes(bo), wb, "replay: blackout_col")
            assert untouched(new_lens, new_hits)
        del g
        sc.graph_release()
    finally:
        sc.close()


def test_refusals(torch_cuda, scene):
    """The march forms refuse what the calls they extend refuse, by their own name; the shade refuses bh_shade_lens's
    list and its own.  Nothing is written."""
    torch = torch_cuda
    W, H = 16, 8
    scene.camera_uniform, scene.uniforms = ref.view_uniform("DISC_IN", W, H), uniforms()
    lens, hits, side = buffer(torch, W * H, 2), buffer(torch, W * H, 3), buffer(torch, W * H, 4)
    dirs = torch.from_numpy(ref.ray_map("DISC_IN", "equirect", W, H).copy()).cuda()
    lib, ctx, stream = scene.lib, scene._ctx, torch.cuda.current_stream().cuda_stream
    cam, U = C.byref(scene.camera_uniform.c), C.byref(scene.uniforms.to_c())
    pose = C.byref(raymap.pose((2.66, 0.089, 2.72)))

    def desc(**kw):
        d = _abi.bh_render_desc()
        d.width, d.height, d.max_iters, d.scene_flags = W, H, 64, 3
        d.math, d.layout, d.shard_count, d.schedule = bh.BH_MATH_EXACT, bh.BH_LAYOUT_ROWMAJOR, 1, bh.BH_SCHED_TILE
        for k, v in kw.items():
            setattr(d, k, v)
        return C.byref(d)

    def pin(d, l=lens.data_ptr(), h=hits.data_ptr()):
        return lib.bh_render_lens_hits(ctx, cam, U, d, l, h, stream)

    def posed(d, l=lens.data_ptr(), h=hits.data_ptr(), m=dirs.data_ptr()):
        return lib.bh_render_lens_rays_posed_hits(ctx, pose, U, d, m, l, h, stream)

    for name, call in (("bh_render_lens_hits", pin), ("bh_render_lens_rays_posed_hits", posed)):
        for kw in (dict(math=bh.BH_MATH_FAST), dict(layout=bh.BH_LAYOUT_TILES), dict(shard_count=2, shard_index=1),
                   dict(schedule=bh.BH_SCHED_PAIR), dict(dbg_fate=side.data_ptr()), dict(out_col=side.data_ptr())):
            assert call(desc(**kw)) == _abi.BH_ERR_UNSUPPORTED, (name, kw)
            text = lib.bh_last_error().decode()
            assert text.startswith(name + ":") and text.endswith("."), (name, kw, text)
        for bad in (dict(h=None), dict(h=hits.data_ptr() + 2), dict(l=None), dict(l=lens.data_ptr() + 4)):
            assert call(desc(), **bad) == _abi.BH_ERR_INVALID_ARG, (name, bad)
            assert lib.bh_last_error().decode().startswith(name + ":"), (name, bad)
        for kw in (dict(width=0), dict(height=65537), dict(max_iters=0), dict(scene_flags=4)):
            assert call(desc(**kw)) == _abi.BH_ERR_INVALID_ARG, (name, kw)
    assert posed(desc(), m=None) == _abi.BH_ERR_INVALID_ARG

    col, bo = target(torch, W, H, F32), target(torch, W, H, F32)
    other = new_scene()
    try:
        foreign = bh.Disc(other, ref.white_disc())

        def sdesc(**kw):
            d = _abi.bh_shade_desc()
            d.width, d.height, d.ss, d.format = W, H, 1, F32
            d.lens, d.out_col, d.out_blackout = lens.data_ptr(), col.data_ptr(), bo.data_ptr()
            for k, v in kw.items():
                setattr(d, k, v)
            return C.byref(d)

        def ddesc(**kw):
            d = _abi.bh_disc_desc()
            d.hits, d.disc, d.rs, d.scene_flags, d.spin, d.gain = hits.data_ptr(), scene.test_disc.handle, 1.0, 3, 0.37, 1.0
            for k, v in kw.items():
                setattr(d, k, v)
            return C.byref(d)

        nan, inf = float("nan"), float("inf")
        for kw in (dict(ss=0), dict(ss=3), dict(lens=None), dict(lens=lens.data_ptr() + 4), dict(out_col=None), dict(width=0),
                   dict(width=65537), dict(format=3)):
            assert lib.bh_shade_lens_disc(ctx, sdesc(**kw), ddesc(), stream) == _abi.BH_ERR_INVALID_ARG, kw
        for kw in (dict(hits=None), dict(hits=hits.data_ptr() + 2), dict(disc=None), dict(disc=foreign.handle),
                   dict(scene_flags=4), dict(spin=nan), dict(spin=inf), dict(spin=-inf), dict(gain=-1.0), dict(gain=nan),
                   dict(gain=inf)):
            assert lib.bh_shade_lens_disc(ctx, sdesc(), ddesc(**kw), stream) == _abi.BH_ERR_INVALID_ARG, kw
            assert lib.bh_last_error().decode().startswith("bh_shade_lens_disc:"), kw
        assert lib.bh_shade_lens_disc(ctx, sdesc(), None, stream) == _abi.BH_ERR_INVALID_ARG
        with pytest.raises(bh.BhError):
            scene.shade(lens[:W * H], col, bo, width=W, height=H, hits=hits[:W * H].view(H, W, 3), disc=foreign)
        with pytest.raises(bh.BhError):
            scene.shade(lens[:W * H], col, bo, width=W, height=H, hits=hits[:W * H].view(H, W, 3))
        for a in ((None, 1, 1), (ref.white_disc().ctypes.data, 0, 1), (ref.white_disc().ctypes.data, 1, 32769)):
            assert lib.bh_disc_create(ctx, *a, C.byref(C.c_void_p())) == _abi.BH_ERR_INVALID_ARG
            assert lib.bh_last_error().decode().startswith("bh_disc_create:")
        torch.cuda.synchronize()
        assert untouched(lens, hits, side, col, bo)
    finally:
        other.close()


def test_disc_close_after_scene_close(torch_cuda):
    sc = new_scene()
    a, b = bh.Disc(sc, ref.disc_texture(37, 5)), bh.Disc(sc, ref.white_disc())
    assert (a.n_phi, a.n_r) == (37, 5)
    b.close()
    assert b.handle is None
    b.close()
    sc.close()
    assert a.handle is None
    a.close()
