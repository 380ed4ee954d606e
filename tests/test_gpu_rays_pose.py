"""Posed ray-map renders on the GPU (bh_render_frames_rays, bh_render_frames_shutter_rays, bh_render_lens_rays_posed;
Scene.render_frames_rays, render_(frames_)shutter_rays, render_lens(pose=...)): every pixel of every frame equals the
reference of tests/_rays_pose_ref.py -- the pose formula restated in numpy fp32, then the CPU oracle's trace_ray of
the normalised vector, the numpy resolve trees -- bit for bit in RGBA32F and as that reference's encode in the other
formats.  The reference is never the GPU's own output; where a test also compares two GPU results, both have been
compared with the reference first.  No pixel is left out of a comparison."""
import ctypes as C

import numpy as np
import pytest

import black_hole_ray_marching_amd as bh
from black_hole_ray_marching_amd import _abi, raymap
from tests import _rays_pose_ref as pref
from tests import _rays_ref as ref
from tests._cases import camera_uniform, uniforms
from tests._lens_ref import frame
from tests._ss_ref import CAP, FLAGS, expected_bytes, sky_ss

pytestmark = pytest.mark.gpu

DT = {bh.BH_OUT_RGBA32F: "float32", bh.BH_OUT_RGBA16F: "float16", bh.BH_OUT_BGRA8_SRGB: "uint8"}
FMTS = [bh.BH_OUT_RGBA32F, bh.BH_OUT_RGBA16F, bh.BH_OUT_BGRA8_SRGB]
F32 = bh.BH_OUT_RGBA32F
SENTINEL = 0xA5  # every byte of a buffer before a call
GUARD = 64       # pixels (records, map vectors) after the last one that must keep their sentinels


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
    """The map in a guarded device buffer (a copy: the reference maps are read-only)."""
    m = np.array(m, dtype=np.float32, order="C")
    H, W = m.shape[:2]
    body, guard = guarded(torch, W * H * 3, 4)
    t = body.view(torch.float32).view(H, W, 3)
    t.copy_(torch.from_numpy(m))
    t.guard, t.host = guard, m
    return t


def map_ok(dirs):
    return guards_ok(dirs) and np.array_equal(dirs.cpu().numpy().view(np.uint32), dirs.host.view(np.uint32))


def rows(names):
    return [pref.rows(n) for n in names]


def render_frames(torch, sc, dirs, names, W, H, fmt=F32, blackout=True, **kw):
    """[(col bytes, blackout bytes or None)] per pose of Scene.render_frames_rays into sentinel-filled, guarded targets"""
    cols = [target(torch, W, H, fmt) for _ in names]
    bos = [target(torch, W, H, fmt) for _ in names] if blackout else None
    sc.render_frames_rays(dirs, cols, bos, poses=rows(names), fmt=fmt, width=W, height=H, **kw)
    torch.cuda.synchronize()
    assert guards_ok(*cols) and (bos is None or guards_ok(*bos)), "the guard region after a target was written"
    assert map_ok(dirs), "the map is an input"
    return [(as_bytes(c), None if bos is None else as_bytes(bos[i])) for i, c in enumerate(cols)]


def render_shutter(torch, sc, dirs, groups, W, H, fmt=F32, blackout=True, **kw):
    cols = [target(torch, W, H, fmt) for _ in groups]
    bos = [target(torch, W, H, fmt) for _ in groups] if blackout else None
    sc.render_frames_shutter_rays(dirs, cols, bos, poses=[rows(g) for g in groups], fmt=fmt, width=W, height=H, **kw)
    torch.cuda.synchronize()
    assert guards_ok(*cols) and (bos is None or guards_ok(*bos)), "the guard region after a target was written"
    assert map_ok(dirs), "the map is an input"
    return [(as_bytes(c), None if bos is None else as_bytes(bos[i])) for i, c in enumerate(cols)]


def assert_frame(got, want, what):
    want = np.ascontiguousarray(want).view(np.uint8).reshape(got.shape)
    bad = (got != want).any(-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ, first at {np.argwhere(bad)[:4].tolist()}"


def assert_frames(got, want, fmt, what):
    assert len(got) == len(want)
    for i, ((gc, gb), (wc, wb)) in enumerate(zip(got, want)):
        assert not np.isnan(wc).any() and not np.isnan(wb).any()
        assert_frame(gc, expected_bytes(fmt, wc), f"{what} frame {i} fmt {fmt} col")
        if gb is not None:
            assert_frame(gb, expected_bytes(fmt, wb), f"{what} frame {i} fmt {fmt} blackout_col")


def assert_equal_up_to_nan_payload(got_bytes, want, what):
    got = np.ascontiguousarray(got_bytes).view(np.float32).reshape(want.shape)
    bad = (ref.canonical_nan(got) != ref.canonical_nan(want)).any(-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} pixels differ, first at {np.argwhere(bad)[:4].tolist()}"


# ---- frames ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 33])
def test_frames_of_distinct_poses(torch_cuda, scene, n):
    """n frames of one launch over one map, every pose different: 3 is no power of two, 33 reads the device table."""
    torch = torch_cuda
    W, H = 13, 7
    names = pref.sequence(n)
    pref.assert_all_fates(names, "general", W, H, f"n = {n}")
    dirs = upload(torch, pref.camera_map("general", W, H))
    assert_frames(render_frames(torch, scene, dirs, names, W, H), pref.frames(names, "general", W, H), F32, f"n {n}")
    if n == 1:
        col = target(torch, W, H, F32)
        nrk = torch.zeros((H, W), dtype=torch.int16, device="cuda")
        fate = torch.full((H, W), 0xFF, dtype=torch.uint8, device="cuda")
        scene.render_frames_rays(dirs, [col], poses=rows(names), width=W, height=H, dbg_n_rk=[nrk], dbg_fate=[fate])
        torch.cuda.synchronize()
        want = pref.posed(names[0], "general", W, H)
        assert_frame(as_bytes(col), want[0], "col with dbg outputs")
        assert np.array_equal(fate.cpu().numpy(), want[3])
        assert np.array_equal(nrk.cpu().numpy().view(np.uint16), want[4])


@pytest.mark.parametrize("blackout", [True, False])
@pytest.mark.parametrize("fmt", FMTS)
def test_three_frames_formats_and_targets(torch_cuda, scene, fmt, blackout):
    torch = torch_cuda
    W, H = 40, 24
    names = pref.sequence(3)
    pref.assert_all_fates(names, "general", W, H, "n = 3 40x24")
    dirs = upload(torch, pref.camera_map("general", W, H))
    got = render_frames(torch, scene, dirs, names, W, H, fmt, blackout)
    assert_frames(got, pref.frames(names, "general", W, H), fmt, "n 3 40x24")


@pytest.mark.parametrize("name", pref.POSES)
def test_each_named_pose(torch_cuda, scene, name):
    """The rotated, unit, sheared and mirrored bases alone, at both sizes, against the reference; and the same bytes
    from render_rays over the map turned on the host (raymap.apply_pose): exact by definition."""
    torch = torch_cuda
    for W, H in ref.SIZES:
        m = pref.camera_map("general", W, H)
        dirs = upload(torch, m)
        (col, bo), = render_frames(torch, scene, dirs, [name], W, H)
        assert_frames([(col, bo)], pref.frames([name], "general", W, H), F32, f"{name} {W}x{H}")
        p = pref.rows(name)
        world = upload(torch, raymap.apply_pose(p, m))
        wc, wb = target(torch, W, H, F32), target(torch, W, H, F32)
        scene.render_rays(world, wc, wb, pos=p[0], width=W, height=H)
        torch.cuda.synchronize()
        assert np.array_equal(as_bytes(wc), col) and np.array_equal(as_bytes(wb), bo), f"{name} {W}x{H}: render_rays differs"


@pytest.mark.parametrize("name", pref.POSES)
def test_non_finite_directions(torch_cuda, scene, name):
    """Four rays of the 8 x 8 map are the zero vector, (inf, 0, 0), (nan, 1, 0) and (0, -inf, inf): every pixel is
    trace_ray of the numpy formula's normalised result, and render_rays over the host-turned map gives the same,
    NaN payloads aside (the host's and the device's NaNs differ in nothing else)."""
    torch = torch_cuda
    m = pref.camera_map("nonfinite", 8, 8)
    want = pref.posed(name, "nonfinite", 8, 8)
    dirs = upload(torch, m)
    (col, bo), = render_frames(torch, scene, dirs, [name], 8, 8)
    assert_equal_up_to_nan_payload(col, want[0], "col")
    assert_equal_up_to_nan_payload(bo, want[1], "blackout_col")
    p = pref.rows(name)
    world = upload(torch, raymap.apply_pose(p, m))
    wc, wb = target(torch, 8, 8, F32), target(torch, 8, 8, F32)
    scene.render_rays(world, wc, wb, pos=p[0], width=8, height=8)
    torch.cuda.synchronize()
    assert_equal_up_to_nan_payload(as_bytes(wc), want[0], "render_rays col")
    assert_equal_up_to_nan_payload(col, as_bytes(wc).view(np.float32).reshape(8, 8, 4), "posed against render_rays col")
    assert_equal_up_to_nan_payload(bo, as_bytes(wb).view(np.float32).reshape(8, 8, 4), "posed against render_rays blackout_col")
    lens_body, lens_guard = guarded(torch, 8 * 8, 8)
    lens = lens_body.view(torch.float32).view(8, 8, 2)
    scene.render_lens(lens, width=8, height=8, dirs=dirs, pose=p)
    torch.cuda.synchronize()
    assert_equal_up_to_nan_payload(as_bytes(lens), want[2], "lens")
    assert (as_bytes(lens_guard) == SENTINEL).all() and map_ok(dirs)


# ---- supersampling -------------------------------------------------------------------------------------------------
SS_POSES = ("rotD", "rotH")


@pytest.mark.parametrize("W,H,k", [(13, 7, 2), (13, 7, 4), (5, 3, 8)])
def test_supersampled_frames(torch_cuda, scene, W, H, k):
    torch = torch_cuda
    pref.assert_all_fates(SS_POSES, "equirect", k * W, k * H, f"ss {k}")
    dirs = upload(torch, pref.camera_map("equirect", k * W, k * H))
    want = pref.frames(SS_POSES, "equirect", W, H, k)
    for fmt in FMTS:
        assert_frames(render_frames(torch, scene, dirs, SS_POSES, W, H, fmt, ss=k), want, fmt, f"ss {k}")
    assert_frames(render_frames(torch, scene, dirs, SS_POSES, W, H, F32, False, ss=k), want, F32, f"ss {k} col alone")


# ---- shutter -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_sub", [2, 4, 8, 16])
def test_shutter_over_a_map(torch_cuda, scene, n_sub):
    torch = torch_cuda
    W, H = 13, 7
    names = pref.sequence(n_sub)
    pref.assert_all_fates(names, "general", W, H, f"n_sub {n_sub}")
    dirs = upload(torch, pref.camera_map("general", W, H))
    got = render_shutter(torch, scene, dirs, [names], W, H)
    assert_frames(got, [pref.shutter(names, "general", W, H)], F32, f"n_sub {n_sub}")


@pytest.mark.parametrize("blackout", [True, False])
@pytest.mark.parametrize("fmt", FMTS)
def test_shutter_formats_and_targets(torch_cuda, scene, fmt, blackout):
    torch = torch_cuda
    W, H = 13, 7
    names = pref.sequence(4, 1)
    dirs = upload(torch, pref.camera_map("general", W, H))
    got = render_shutter(torch, scene, dirs, [names], W, H, fmt, blackout)
    assert_frames(got, [pref.shutter(names, "general", W, H)], fmt, "n_sub 4")
    # n_sub = 1 is bh_render_frames_rays
    got = render_shutter(torch, scene, dirs, [names[:1], names[1:2]], W, H, fmt, blackout)
    assert_frames(got, pref.frames(names[:2], "general", W, H), fmt, "n_sub 1")


def test_shutter_two_output_frames(torch_cuda, scene):
    torch = torch_cuda
    W, H = 40, 24
    names = pref.sequence(8)
    groups = [names[:4], names[4:]]
    pref.assert_all_fates(names, "general", W, H, "shutter 2 x 4 40x24")
    dirs = upload(torch, pref.camera_map("general", W, H))
    got = render_shutter(torch, scene, dirs, groups, W, H)
    assert_frames(got, [pref.shutter(g, "general", W, H) for g in groups], F32, "2 frames of n_sub 4")


def test_shutter_supersampled(torch_cuda, scene):
    torch = torch_cuda
    W, H, k = 13, 7, 2
    names = ("rotD", "rotH", "mirrorD", "turn1")
    pref.assert_all_fates(names, "equirect", k * W, k * H, "shutter ss 2")
    dirs = upload(torch, pref.camera_map("equirect", k * W, k * H))
    for fmt in (F32, bh.BH_OUT_BGRA8_SRGB):
        got = render_shutter(torch, scene, dirs, [names], W, H, fmt, ss=k)
        assert_frames(got, [pref.shutter(names, "equirect", W, H, k)], fmt, "n_sub 4 ss 2")


# ---- lens ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,W,H", [(n, 13, 7) for n in pref.POSES] + [("rotH", 40, 24), ("shearF2", 40, 24)])
def test_posed_lens(torch_cuda, scene, name, W, H):
    torch = torch_cuda
    wrec = pref.posed(name, "general", W, H)[2]
    dirs = upload(torch, pref.camera_map("general", W, H))
    body, guard = guarded(torch, W * H, 8)
    lens = body.view(torch.float32).view(H, W, 2)
    for order in ("first", "repeated"):
        body.fill_(SENTINEL)
        scene.render_lens(lens, width=W, height=H, dirs=dirs, pose=pref.rows(name))
        torch.cuda.synchronize()
        got = lens.cpu().numpy().view(np.uint32)
        bad = (got != wrec.view(np.uint32)).any(-1)
        assert not bad.any(), f"{order}: {int(bad.sum())} records differ, first at {np.argwhere(bad)[:4].tolist()}"
        assert (as_bytes(guard) == SENTINEL).all() and map_ok(dirs)
    for fmt in FMTS:  # shade of that lens is render_frames_rays of the pose (itself compared with the reference)
        sc, sb = target(torch, W, H, fmt), target(torch, W, H, fmt)
        scene.shade(lens, sc, sb, fmt=fmt, width=W, height=H)
        torch.cuda.synchronize()
        (rc, rb), = render_frames(torch, scene, dirs, [name], W, H, fmt)
        assert_frames([(rc, rb)], pref.frames([name], "general", W, H), fmt, "render_frames_rays")
        assert np.array_equal(as_bytes(sc), rc) and np.array_equal(as_bytes(sb), rb), fmt


# ---- order and state -----------------------------------------------------------------------------------------------
def test_order_and_state(torch_cuda):
    """The bytes do not depend on the dispatch order, the build or what else the stream rendered at this size:
    posed launches interleaved with render, render_rays and render_frames of the same geometry, the same every time."""
    torch = torch_cuda
    W, H, cam = 40, 24, "D"
    names = pref.sequence(3)
    groups = [pref.sequence(4), pref.sequence(4, 4)]
    sc = new_scene()
    try:
        sc.uniforms = uniforms()
        sc.camera_uniform = camera_uniform(cam, W, H)
        want = pref.frames(names, "general", W, H)
        want_sh = [pref.shutter(g, "general", W, H) for g in groups]
        pc, pb = frame(cam, W, H, "ctx")
        wc, wb = ref.general("D", W, H)[:2]
        dirs = upload(torch, pref.camera_map("general", W, H))
        world = upload(torch, ref.general_map("D", W, H))

        def posed(what, **kw):
            assert_frames(render_frames(torch, sc, dirs, names, W, H, **kw), want, F32, what)

        def shutter(what, **kw):
            assert_frames(render_shutter(torch, sc, dirs, groups, W, H, **kw), want_sh, F32, what)

        def plain(what, n=1):
            cols, bos = [target(torch, W, H, F32) for _ in range(n)], [target(torch, W, H, F32) for _ in range(n)]
            if n == 1:
                sc.render(cols[0], bos[0], width=W, height=H)
            else:
                sc.render_frames(cols, bos, width=W, height=H)
            torch.cuda.synchronize()
            for c, b in zip(cols, bos):
                assert_frame(as_bytes(c), pc, f"{what} col")
                assert_frame(as_bytes(b), pb, f"{what} blackout_col")

        def rays(what):
            c, b = target(torch, W, H, F32), target(torch, W, H, F32)
            sc.render_rays(world, c, b, pos=ref.position("D"), width=W, height=H)
            torch.cuda.synchronize()
            assert_frame(as_bytes(c), wc, f"{what} col")
            assert_frame(as_bytes(b), wb, f"{what} blackout_col")

        static, lat, issue = (bh.BH_SCHED_TILE | f for f in (bh.BH_SCHED_FLAG_STATIC_ORDER, bh.BH_SCHED_FLAG_LATENCY,
                                                            bh.BH_SCHED_FLAG_ISSUE_ORDER))
        posed("static order", schedule=static)
        posed("first call (centre-out)")
        posed("second call (learned order)")
        posed("third call (repeated frame)")
        posed("latency build", schedule=lat)
        posed("issue-order build", schedule=issue)
        shutter("shutter static order", schedule=static)
        shutter("shutter")
        shutter("shutter repeated")
        shutter("shutter latency build", schedule=lat)
        shutter("shutter issue-order build", schedule=issue)
        plain("a plain render after posed launches")
        posed("after a plain render")
        rays("render_rays of the same geometry")
        posed("after render_rays")
        plain("render_frames", n=3)
        posed("after render_frames")
        rays("render_rays again")
        shutter("shutter at the end")
        plain("a plain render at the end")
    finally:
        sc.close()


# ---- graph -----------------------------------------------------------------------------------------------------------
def test_graph(torch_cuda):
    """The first call of a key under capture is refused (BH_ERR_UNSUPPORTED) and writes nothing; after one eager call
    a linear capture of a second call on one stream, replayed twice, gives the eager bytes (the reference's)."""
    torch = torch_cuda
    W, H = 40, 24
    names = pref.sequence(2)
    sc = new_scene()
    try:
        sc.uniforms = uniforms()
        want = pref.frames(names, "general", W, H)
        dirs = upload(torch, pref.camera_map("general", W, H))
        small = upload(torch, pref.camera_map("general", 13, 7))
        cols, bos = [target(torch, W, H, F32) for _ in names], [target(torch, W, H, F32) for _ in names]
        other = target(torch, 13, 7, F32)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        sc.render_frames_rays(dirs, cols, bos, poses=rows(names), width=W, height=H, stream=s)  # eager, on the capture's stream
        s.synchronize()
        assert_frames([(as_bytes(c), as_bytes(b)) for c, b in zip(cols, bos)], want, F32, "eager")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            with pytest.raises(bh.BhError) as e:
                sc.render_frames_rays(small, [other], poses=rows(names[:1]), width=13, height=7, stream=s)
            assert e.value.status == _abi.BH_ERR_UNSUPPORTED
            sc.render_frames_rays(dirs, cols, bos, poses=rows(names), width=W, height=H, stream=s)
        for _ in range(2):
            for t in cols + bos:
                t.view(torch.uint8).fill_(SENTINEL)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert_frames([(as_bytes(c), as_bytes(b)) for c, b in zip(cols, bos)], want, F32, "replay")
            assert untouched(other) and guards_ok(*cols, *bos) and map_ok(dirs)
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


def _poses(names):
    ps = (_abi.bh_ray_pose * len(names))()
    for i, n in enumerate(names):
        ps[i] = _abi.bh_ray_pose.from_buffer_copy(pref.rows(n).tobytes())
    return ps


UNSUPPORTED = ["math", "layout", "shard_count", "partition", "pair", "persistent"]
DBG = ["dbg_n_rk", "dbg_fate", "dbg_steps"]
# what each entry refuses: with ss == 1 the dbg_* outputs are bh_render_frames' (test_frames_of_distinct_poses); a
# shutter resolves rays away as ss does; a lens render has no targets
REFUSALS = ([("bh_render_frames_rays", w) for w in UNSUPPORTED] + [("bh_render_frames_rays ss", w) for w in UNSUPPORTED + DBG] +
            [("bh_render_frames_shutter_rays", w) for w in UNSUPPORTED + DBG] +
            [("bh_render_lens_rays_posed", w) for w in UNSUPPORTED + DBG + ["out_col", "out_blackout"]])


@pytest.mark.parametrize("entry,what", REFUSALS)
def test_refuses_unsupported(torch_cuda, scene, what, entry):
    """The offending field sits in the LAST desc of the call: every desc is checked."""
    torch = torch_cuda
    W, H = 40, 24
    fn = entry.split()[0]
    lens_entry, ss = fn == "bh_render_lens_rays_posed", 2 if entry.endswith("ss") else 1
    n_sub = 2 if fn == "bh_render_frames_shutter_rays" else 1
    n = 1 if lens_entry else 2
    dirs = upload(torch, pref.camera_map("equirect", ss * W, ss * H))
    cols, bos = [target(torch, W, H, F32) for _ in range(n)], [target(torch, W, H, F32) for _ in range(n)]
    side = torch.full((H, W, 16), SENTINEL, dtype=torch.uint8, device="cuda")
    lens, lens_guard = guarded(torch, W * H, 8)
    part = bh.Partition(W, H, [1]) if what == "partition" else None
    try:
        kw = {"math": dict(math=bh.BH_MATH_FAST), "layout": dict(layout=bh.BH_LAYOUT_TILES),
              "shard_count": dict(shard_count=2, shard_index=1), "partition": dict(partition=part and part.handle),
              "pair": dict(schedule=bh.BH_SCHED_PAIR), "persistent": dict(schedule=bh.BH_SCHED_PERSISTENT),
              "dbg_n_rk": dict(dbg_n_rk=side.data_ptr()), "dbg_fate": dict(dbg_fate=side.data_ptr()),
              "dbg_steps": dict(dbg_steps=side.data_ptr()), "out_col": dict(out_col=side.data_ptr()),
              "out_blackout": dict(out_blackout=side.data_ptr())}[what]
        descs = (_abi.bh_render_desc * n)()
        for i in range(n):
            base = {} if lens_entry else dict(out_col=cols[i].data_ptr(), out_blackout=bos[i].data_ptr())
            descs[i] = _desc(W, H, **{**base, **(kw if i == n - 1 else {})})
        if what in UNSUPPORTED and n > 1:  # what makes a launch is the same in every desc (else: invalid argument)
            descs[0] = _desc(W, H, **{**dict(out_col=cols[0].data_ptr(), out_blackout=bos[0].data_ptr()), **kw})
        ps = _poses(pref.sequence(n * n_sub))
        U, stream = C.byref(scene.uniforms.to_c()), torch.cuda.current_stream().cuda_stream
        lib, p = scene.lib, dirs.data_ptr()
        if lens_entry:
            st = lib.bh_render_lens_rays_posed(scene._ctx, ps, U, descs, p, lens.data_ptr(), stream)
        elif n_sub > 1:
            st = lib.bh_render_frames_shutter_rays(scene._ctx, n, n_sub, ps, U, descs, p, ss, stream)
        else:
            st = lib.bh_render_frames_rays(scene._ctx, n, ps, U, descs, p, ss, stream)
        assert st == _abi.BH_ERR_UNSUPPORTED
        text = lib.bh_last_error().decode()
        assert text.startswith(fn + ":") and text.endswith(".") and " " in text
        torch.cuda.synchronize()
        assert untouched(*cols, *bos, side, lens) and guards_ok(*cols, *bos) and (as_bytes(lens_guard) == SENTINEL).all()
        assert map_ok(dirs)
    finally:
        if part is not None:
            part.close()


def test_refuses_invalid_arguments(torch_cuda, scene):
    torch = torch_cuda
    W, H = 40, 24
    dirs = upload(torch, pref.camera_map("equirect", W, H))
    cols, bos = [target(torch, W, H, F32) for _ in range(2)], [target(torch, W, H, F32) for _ in range(2)]
    lens, lens_guard = guarded(torch, W * H, 8)
    U, stream = C.byref(scene.uniforms.to_c()), torch.cuda.current_stream().cuda_stream
    bad, ctx, lib = _abi.BH_ERR_INVALID_ARG, scene._ctx, scene.lib
    frames, shut, lensp = lib.bh_render_frames_rays, lib.bh_render_frames_shutter_rays, lib.bh_render_lens_rays_posed

    def descs(n=2, **kw):
        d = (_abi.bh_render_desc * n)()
        for i in range(n):
            d[i] = _desc(W, H, **{**dict(out_col=cols[i % 2].data_ptr(), out_blackout=bos[i % 2].data_ptr()), **kw})
        return d

    d, ld = descs(), _desc(W, H)
    ps = _poses(pref.sequence(4))
    many = _poses(pref.sequence(256) + pref.sequence(1))
    p, lp = dirs.data_ptr(), lens.data_ptr()
    assert frames(ctx, 2, ps, U, d, None, 1, stream) == bad
    assert lib.bh_last_error().decode().startswith("bh_render_frames_rays")
    assert shut(ctx, 2, 2, ps, U, d, None, 1, stream) == bad
    assert lib.bh_last_error().decode().startswith("bh_render_frames_shutter_rays")
    assert lensp(ctx, ps, U, C.byref(ld), None, lp, stream) == bad
    assert lib.bh_last_error().decode().startswith("bh_render_lens_rays_posed")
    for off in (1, 2, 3):
        assert frames(ctx, 2, ps, U, d, p + off, 1, stream) == bad, off
        assert shut(ctx, 2, 2, ps, U, d, p + off, 1, stream) == bad, off
        assert lensp(ctx, ps, U, C.byref(ld), p + off, lp, stream) == bad, off
    assert frames(ctx, 2, None, U, d, p, 1, stream) == bad
    assert frames(ctx, 2, ps, None, d, p, 1, stream) == bad
    assert frames(ctx, 2, ps, U, None, p, 1, stream) == bad
    assert frames(None, 2, ps, U, d, p, 1, stream) == bad
    assert shut(ctx, 2, 2, None, U, d, p, 1, stream) == bad
    assert lensp(ctx, None, U, C.byref(ld), p, lp, stream) == bad
    assert lensp(ctx, ps, U, C.byref(ld), p, None, stream) == bad
    assert lensp(ctx, ps, U, C.byref(ld), p, lp + 4, stream) == bad
    for n in (0, 257, 0xFFFFFFFF):
        assert frames(ctx, n, many, U, descs(1), p, 1, stream) == bad, n
    for n_sub in (0, 3, 5, 32, 0xFFFFFFFF):
        assert shut(ctx, 1, n_sub, many, U, d, p, 1, stream) == bad, n_sub
    for n, n_sub in ((129, 2), (65, 4), (17, 16), (0, 2), (0x10000000, 16)):  # more than BH_MAX_FRAMES cameras
        assert shut(ctx, n, n_sub, many, U, descs(1), p, 1, stream) == bad, (n, n_sub)
    for ss in (0, 3, 5, 16, 0xFFFFFFFF):
        assert frames(ctx, 2, ps, U, d, p, ss, stream) == bad, ss
        assert shut(ctx, 2, 2, ps, U, d, p, ss, stream) == bad, ss
    for kw in (dict(width=0), dict(height=0), dict(width=65537), dict(max_iters=0), dict(max_iters=65536),
               dict(scene_flags=4), dict(format=3), dict(out_col=None), dict(math=2), dict(schedule=0x800)):
        assert frames(ctx, 2, ps, U, descs(**kw), p, 1, stream) == bad, kw
        assert shut(ctx, 2, 2, ps, U, descs(**kw), p, 1, stream) == bad, kw
    for kw in (dict(width=W - 8), dict(max_iters=CAP - 1), dict(format=bh.BH_OUT_RGBA16F), dict(out_col=None)):
        two = descs()  # frames of one launch differ in their outputs alone
        two[1] = _desc(W, H, **{**dict(out_col=cols[1].data_ptr(), out_blackout=bos[1].data_ptr()), **kw})
        assert frames(ctx, 2, ps, U, two, p, 1, stream) == bad, kw
        assert shut(ctx, 2, 2, ps, U, two, p, 1, stream) == bad, kw
    for ss, (w, h) in ((2, (32769, 1)), (4, (1, 16385)), (8, (8193, 1))):
        one = (_abi.bh_render_desc * 1)(_desc(w, h, out_col=cols[0].data_ptr()))
        assert frames(ctx, 1, ps, U, one, p, ss, stream) == bad, (ss, w, h)
    for kw in (dict(width=0), dict(height=65537), dict(max_iters=0), dict(scene_flags=4)):
        assert lensp(ctx, ps, U, C.byref(_desc(W, H, **kw)), p, lp, stream) == bad, kw
    # the Python layer: ss, the map's shape against ss, the poses' count and form, pos with pose
    good = rows(pref.sequence(2))
    for kw in (dict(ss=3), dict(ss=0), dict(ss=2), dict(poses=good[:1]), dict(poses=None), dict(poses=[good[0], good[1][:3]])):
        with pytest.raises(bh.BhError) as e:
            scene.render_frames_rays(dirs, cols, bos, **{**dict(poses=good, width=W, height=H), **kw})
        assert e.value.status == bad, kw
    for poses in ([good], [good[:1]], [good, good[:1]], good):
        with pytest.raises(bh.BhError) as e:
            scene.render_frames_shutter_rays(dirs, cols, bos, poses=poses, width=W, height=H)
        assert e.value.status == bad
    with pytest.raises(bh.BhError) as e:
        scene.render_shutter_rays(dirs, cols[0], bos[0], poses=good + good[:1], width=W, height=H)  # n_sub = 3
    assert e.value.status == bad
    with pytest.raises(bh.BhError) as e:
        scene.render_lens(lens.view(torch.float32), width=W, height=H, dirs=dirs, pose=good[0], pos=(0.0, 0.0, -20.0))
    assert e.value.status == bad
    with pytest.raises(bh.BhError) as e:
        scene.render_lens(lens.view(torch.float32), width=W, height=H, pose=good[0])  # a pose needs a map
    assert e.value.status == bad
    torch.cuda.synchronize()
    assert untouched(*cols, *bos, lens) and guards_ok(*cols, *bos) and (as_bytes(lens_guard) == SENTINEL).all() and map_ok(dirs)
    assert frames(ctx, 2, ps, U, d, p, 1, stream) == _abi.BH_OK  # the arguments themselves are good
    assert shut(ctx, 1, 2, ps, U, d, p, 1, stream) == _abi.BH_OK
    assert lensp(ctx, ps, U, C.byref(ld), p, lp, stream) == _abi.BH_OK
    torch.cuda.synchronize()
    assert not untouched(cols[0]) and not untouched(lens) and guards_ok(*cols, *bos) and map_ok(dirs)
