"""Origin-map renders on the GPU (bh_render_frames_rays_origins, bh_render_lens_rays_origins;
Scene.render_frames_rays(origins=...), Scene.render_lens(origins=...)): every pixel of every frame equals the reference
of tests/_rays_origins_ref.py -- the origin and pose formulas restated in numpy fp32, then the CPU oracle's
trace_ray(ro0, rd0) ray by ray, the numpy resolve tree -- bit for bit in RGBA32F and as that reference's encode in the
other formats.  The reference is never the GPU's own output; where a test also compares two GPU results, one of them
has been compared with the reference first.  No pixel is left out of a comparison."""
import ctypes as C

import numpy as np
import pytest

import black_hole_ray_marching_amd as bh
from black_hole_ray_marching_amd import _abi, raymap
from tests import _rays_origins_ref as oref
from tests import _rays_pose_ref as pref
from tests import _rays_ref as ref
from tests._cases import camera_uniform, uniforms
from tests._lens_mip_ref import sky
from tests._lens_ref import frame
from tests._ss_ref import CAP, FLAGS, expected_bytes, sky_ss

pytestmark = pytest.mark.gpu

DT = {bh.BH_OUT_RGBA32F: "float32", bh.BH_OUT_RGBA16F: "float16", bh.BH_OUT_BGRA8_SRGB: "uint8"}
FMTS = [bh.BH_OUT_RGBA32F, bh.BH_OUT_RGBA16F, bh.BH_OUT_BGRA8_SRGB]
F32 = bh.BH_OUT_RGBA32F
SENTINEL = 0xA5  # every byte of a buffer before a call
GUARD = 64       # pixels (records, map vectors) after the last one that must keep their sentinels
STATIC, LAT, ISSUE = (bh.BH_SCHED_TILE | f for f in (bh.BH_SCHED_FLAG_STATIC_ORDER, bh.BH_SCHED_FLAG_LATENCY,
                                                     bh.BH_SCHED_FLAG_ISSUE_ORDER))


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
    """n elements of bytes_per bytes between two guards of GUARD elements, every byte the sentinel ->
    (the n elements, the guards)"""
    g = GUARD * bytes_per
    buf = torch.full((g + n * bytes_per + g,), SENTINEL, dtype=torch.uint8, device="cuda")
    return buf[g:g + n * bytes_per], (buf[:g], buf[g + n * bytes_per:])


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
    return all((as_bytes(g) == SENTINEL).all() for t in ts if t is not None for g in t.guard)


def upload(torch, m):
    """The map in a guarded device buffer (a copy: the reference maps are read-only)."""
    m = np.array(m, dtype=np.float32, order="C")
    H, W = m.shape[:2]
    body, guard = guarded(torch, W * H * 3, 4)
    t = body.view(torch.float32).view(H, W, 3)
    t.copy_(torch.from_numpy(m))
    t.guard, t.host = guard, m
    return t


def map_ok(*ms):
    return all(guards_ok(m) and np.array_equal(m.cpu().numpy().view(np.uint32), m.host.view(np.uint32)) for m in ms)


def rows(names):
    return [oref.rows(n) for n in names]


def render_frames(torch, sc, dirs, orgs, names, W, H, fmt=F32, blackout=True, **kw):
    """[(col bytes, blackout bytes or None)] per pose of Scene.render_frames_rays(origins=orgs) into sentinel-filled,
    guarded targets (orgs None: the call without origins)"""
    cols = [target(torch, W, H, fmt) for _ in names]
    bos = [target(torch, W, H, fmt) for _ in names] if blackout else None
    sc.render_frames_rays(dirs, cols, bos, poses=rows(names), origins=orgs, fmt=fmt, width=W, height=H, **kw)
    torch.cuda.synchronize()
    assert guards_ok(*cols) and (bos is None or guards_ok(*bos)), "a guard region beside a target was written"
    assert map_ok(dirs) and (orgs is None or map_ok(orgs)), "the maps are inputs"
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


def maps(torch, mkind, okind, W, H):
    return upload(torch, pref.camera_map(mkind, W, H)), upload(torch, oref.origins(okind, W, H))


# ---- parity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 33])
def test_frames_of_distinct_poses(torch_cuda, scene, n):
    """n frames of one launch over one pair of maps -- the general map, the scatter with the hand row -- every pose
    different, from positions D, H and F2: 3 is no power of two, 33 reads the device table."""
    torch = torch_cuda
    W, H = 13, 7
    names = oref.sequence(n)
    assert n < 3 or oref.fates(names, "general", "hand", W, H) == oref.ALL_FATES
    dirs, orgs = maps(torch, "general", "hand", W, H)
    got = render_frames(torch, scene, dirs, orgs, names, W, H)
    assert_frames(got, oref.frames(names, "general", "hand", W, H), F32, f"n {n}")
    if n == 1:
        for name in ("axesD", "axesH"):  # ro0 = 0 under the first, the exact radii around the threshold under the second
            col = target(torch, W, H, F32)
            nrk = torch.zeros((H, W), dtype=torch.int16, device="cuda")
            fate = torch.full((H, W), 0xFF, dtype=torch.uint8, device="cuda")
            scene.render_frames_rays(dirs, [col], poses=rows([name]), origins=orgs, width=W, height=H, dbg_n_rk=[nrk],
                                     dbg_fate=[fate])
            torch.cuda.synchronize()
            want = oref.traced(name, "general", "hand", W, H)
            assert_frame(as_bytes(col), want[0], f"{name} col with dbg outputs")
            assert np.array_equal(fate.cpu().numpy(), want[3]), name
            assert np.array_equal(nrk.cpu().numpy().view(np.uint16), want[4]), name


@pytest.mark.parametrize("blackout", [True, False])
@pytest.mark.parametrize("fmt", FMTS)
def test_three_frames_formats_and_targets(torch_cuda, scene, fmt, blackout):
    torch = torch_cuda
    W, H = 40, 24
    names = oref.sequence(3)
    dirs, orgs = maps(torch, "general", "hand", W, H)
    got = render_frames(torch, scene, dirs, orgs, names, W, H, fmt, blackout)
    assert_frames(got, oref.frames(names, "general", "hand", W, H), fmt, "n 3 40x24")


@pytest.mark.parametrize("name", ["rotD", "rotF2", "turn4"])
def test_scatter_at_40x24(torch_cuda, scene, name):
    """The scatter alone from each position: D (every origin outside: the camera-outside step), F2 (every origin inside
    the unit sphere), and a turned H (tiles on both sides of the threshold)."""
    torch = torch_cuda
    W, H = 40, 24
    assert name != "turn4" or oref.straddling_tiles(name, "scatter", W, H) >= 1
    dirs, orgs = maps(torch, "general", "scatter", W, H)
    got = render_frames(torch, scene, dirs, orgs, [name], W, H)
    assert_frames(got, oref.frames([name], "general", "scatter", W, H), F32, name)


# ---- identity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", [LAT, ISSUE], ids=["latency", "issue-order"])
@pytest.mark.parametrize("name", oref.NAMED_POSES)
def test_zero_origins_are_render_frames_rays(torch_cuda, scene, name, schedule):
    """An all +0 origin map renders bh_render_frames_rays' bytes (themselves the reference's), in both exact builds."""
    torch = torch_cuda
    for W, H in ref.SIZES:
        dirs, orgs = maps(torch, "general", "zero", W, H)
        (pc, pb), = render_frames(torch, scene, dirs, None, [name], W, H, schedule=schedule)
        want = ref.trace(pref.apply_np(oref.rows(name), pref.camera_map("general", W, H)), oref.rows(name)[0])[:2]
        assert_frames([(pc, pb)], [want], F32, f"{name} {W}x{H} render_frames_rays")
        (oc, ob), = render_frames(torch, scene, dirs, orgs, [name], W, H, schedule=schedule)
        assert np.array_equal(oc, pc) and np.array_equal(ob, pb), f"{name} {W}x{H}: zero origins differ"


# ---- against the host helper -------------------------------------------------------------------------------------------
def test_against_the_host_helpers(torch_cuda, scene):
    """Per-ray origins have no single-position GPU counterpart, so the comparison is the reference: trace_ray of every
    ray of raymap.apply_pose's map from raymap.apply_origins' origin -- the library's own host formulas, not numpy's."""
    torch = torch_cuda
    name = "rotH"
    for W, H in ref.SIZES:
        m, o, p = pref.camera_map("general", W, H), oref.origins("hand", W, H), oref.rows(name)
        want = oref.trace(raymap.apply_pose(p, m), raymap.apply_origins(p, o))
        dirs, orgs = upload(torch, m), upload(torch, o)
        (col, bo), = render_frames(torch, scene, dirs, orgs, [name], W, H)
        assert_frames([(col, bo)], [want[:2]], F32, f"{name} {W}x{H}")


# ---- non-finite origins ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", oref.NAMED_POSES)
def test_non_finite_origins(torch_cuda, scene, name):
    """Four origins of the 8 x 8 set are (nan, 0, 0), (inf, 0, 0), (0, -inf, inf) and (1e30, 0, 0): every pixel and
    every lens record is trace_ray's of the numpy formulas' origin, NaN payloads aside; guards around both maps, the
    targets and the lens keep their bytes."""
    torch = torch_cuda
    want = oref.traced(name, "general", "nonfinite", 8, 8)
    dirs, orgs = maps(torch, "general", "nonfinite", 8, 8)
    for schedule in (LAT, ISSUE):
        (col, bo), = render_frames(torch, scene, dirs, orgs, [name], 8, 8, schedule=schedule)
        assert_equal_up_to_nan_payload(col, want[0], "col")
        assert_equal_up_to_nan_payload(bo, want[1], "blackout_col")
    lens_body, lens_guard = guarded(torch, 8 * 8, 8)
    lens = lens_body.view(torch.float32).view(8, 8, 2)
    scene.render_lens(lens, width=8, height=8, dirs=dirs, pose=oref.rows(name), origins=orgs)
    torch.cuda.synchronize()
    assert_equal_up_to_nan_payload(as_bytes(lens), want[2], "lens")
    assert all((as_bytes(g) == SENTINEL).all() for g in lens_guard) and map_ok(dirs, orgs)
    col = target(torch, 8, 8, F32)
    nrk = torch.zeros((8, 8), dtype=torch.int16, device="cuda")
    fate = torch.full((8, 8), 0xFF, dtype=torch.uint8, device="cuda")
    scene.render_frames_rays(dirs, [col], poses=rows([name]), origins=orgs, width=8, height=8, dbg_n_rk=[nrk], dbg_fate=[fate])
    torch.cuda.synchronize()
    assert np.array_equal(fate.cpu().numpy(), want[3]) and np.array_equal(nrk.cpu().numpy().view(np.uint16), want[4])


# ---- supersampling -------------------------------------------------------------------------------------------------
SS_POSES = ("rotD", "rotH")


@pytest.mark.parametrize("W,H,k", [(13, 7, 2), (13, 7, 4), (5, 3, 8)])
def test_supersampled_frames(torch_cuda, scene, W, H, k):
    """Maps and origins are the virtual frame's; rotH's origins straddle the threshold in several tiles."""
    torch = torch_cuda
    assert oref.fates(SS_POSES, "equirect", "scatter", k * W, k * H) == oref.ALL_FATES
    assert oref.straddling_tiles("rotH", "scatter", k * W, k * H) >= 1
    dirs, orgs = maps(torch, "equirect", "scatter", k * W, k * H)
    want = oref.frames(SS_POSES, "equirect", "scatter", W, H, k)
    for fmt in FMTS:
        assert_frames(render_frames(torch, scene, dirs, orgs, SS_POSES, W, H, fmt, ss=k), want, fmt, f"ss {k}")
    assert_frames(render_frames(torch, scene, dirs, orgs, SS_POSES, W, H, F32, False, ss=k), want, F32, f"ss {k} col alone")


# ---- lens ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,W,H", [(n, 13, 7) for n in oref.NAMED_POSES] + [("rotH", 40, 24), ("shearF2", 40, 24)])
def test_lens_with_origins(torch_cuda, scene, name, W, H):
    """The records over both origin sets, equal as uint32 up to a NaN's payload (the general map's 1e30 direction and
    the hand row's far origins end in NaN directions); the shades of the scatter's records are the render's."""
    torch = torch_cuda
    body, guard = guarded(torch, W * H, 8)
    lens = body.view(torch.float32).view(H, W, 2)
    for okind in ("hand", "scatter"):
        wrec = oref.traced(name, "general", okind, W, H)[2]
        dirs, orgs = maps(torch, "general", okind, W, H)
        for order in ("first", "repeated"):
            body.fill_(SENTINEL)
            scene.render_lens(lens, width=W, height=H, dirs=dirs, pose=oref.rows(name), origins=orgs)
            torch.cuda.synchronize()
            got = lens.cpu().numpy()
            bad = (ref.canonical_nan(got) != ref.canonical_nan(wrec)).any(-1)
            assert not bad.any(), f"{okind} {order}: {int(bad.sum())} records differ, first at {np.argwhere(bad)[:4].tolist()}"
            assert all((as_bytes(g) == SENTINEL).all() for g in guard) and map_ok(dirs, orgs)
    for fmt in FMTS:  # shade of that lens is render_frames_rays(origins=...) (itself compared with the reference)
        sc, sb = target(torch, W, H, fmt), target(torch, W, H, fmt)
        scene.shade(lens, sc, sb, fmt=fmt, width=W, height=H)
        torch.cuda.synchronize()
        (rc, rb), = render_frames(torch, scene, dirs, orgs, [name], W, H, fmt)
        assert_frames([(rc, rb)], oref.frames([name], "general", "scatter", W, H), fmt, "render_frames_rays(origins)")
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


# ---- order and state -----------------------------------------------------------------------------------------------
def test_order_and_state(torch_cuda):
    """The bytes do not depend on the dispatch order, the build or what else the stream rendered at this size: launches
    with origins interleaved with render, render_rays and render_frames_rays of the same geometry, neither side's bytes
    changing; and an origin map rewritten in place under one address renders its new contents."""
    torch = torch_cuda
    W, H, cam = 40, 24, "D"
    names = oref.sequence(3)
    sc = new_scene()
    try:
        sc.uniforms = uniforms()
        sc.camera_uniform = camera_uniform(cam, W, H)
        want = oref.frames(names, "general", "hand", W, H)
        want_posed = [ref.trace(pref.apply_np(oref.rows(n), pref.camera_map("general", W, H)), oref.rows(n)[0])[:2] for n in names]
        want_scatter = oref.frames(names, "general", "scatter", W, H)
        pc, pb = frame(cam, W, H, "ctx")
        wc, wb = ref.general("D", W, H)[:2]
        dirs, orgs = maps(torch, "general", "hand", W, H)
        world = upload(torch, ref.general_map("D", W, H))

        def origins(what, **kw):
            assert_frames(render_frames(torch, sc, dirs, orgs, names, W, H, **kw), want, F32, what)

        def posed(what, **kw):
            assert_frames(render_frames(torch, sc, dirs, None, names, W, H, **kw), want_posed, F32, what)

        def plain(what):
            c, b = target(torch, W, H, F32), target(torch, W, H, F32)
            sc.render(c, b, width=W, height=H)
            torch.cuda.synchronize()
            assert_frame(as_bytes(c), pc, f"{what} col")
            assert_frame(as_bytes(b), pb, f"{what} blackout_col")

        def rays(what):
            c, b = target(torch, W, H, F32), target(torch, W, H, F32)
            sc.render_rays(world, c, b, pos=ref.position("D"), width=W, height=H)
            torch.cuda.synchronize()
            assert_frame(as_bytes(c), wc, f"{what} col")
            assert_frame(as_bytes(b), wb, f"{what} blackout_col")

        origins("static order", schedule=STATIC)
        origins("first call (centre-out)")
        origins("second call (learned order)")
        origins("third call (repeated frame)")
        origins("latency build", schedule=LAT)
        origins("issue-order build", schedule=ISSUE)
        plain("a plain render after launches with origins")
        origins("after a plain render")
        rays("render_rays of the same geometry")
        origins("after render_rays")
        posed("render_frames_rays of the same maps")
        origins("after render_frames_rays")
        posed("render_frames_rays again (repeated)")
        posed("render_frames_rays a third time")
        origins("repeated after it")
        # the origin map rewritten in place: the same address, a repeated-frame key that still matches, new bytes
        new = np.array(oref.origins("scatter", W, H))
        orgs.copy_(torch.from_numpy(new))
        orgs.host = new
        torch.cuda.synchronize()
        got = render_frames(torch, sc, dirs, orgs, names, W, H)
        assert_frames(got, want_scatter, F32, "an origin map rewritten in place")
        assert any(not np.array_equal(a[0], expected_bytes(F32, w[0]).view(np.uint8).reshape(a[0].shape))
                   for a, w in zip(got, want)), "the two origin sets render different frames"
        plain("a plain render at the end")
        rays("render_rays at the end")
    finally:
        sc.close()


# ---- graph -----------------------------------------------------------------------------------------------------------
def test_graph(torch_cuda):
    """The first call of a key under capture is refused (BH_ERR_UNSUPPORTED) and writes nothing; after one eager call a
    linear capture of a second call on one stream, replayed twice, gives the eager bytes (the reference's)."""
    torch = torch_cuda
    W, H = 40, 24
    names = oref.sequence(2)
    sc = new_scene()
    try:
        sc.uniforms = uniforms()
        want = oref.frames(names, "general", "hand", W, H)
        dirs, orgs = maps(torch, "general", "hand", W, H)
        small, small_o = maps(torch, "general", "hand", 13, 7)
        cols, bos = [target(torch, W, H, F32) for _ in names], [target(torch, W, H, F32) for _ in names]
        other = target(torch, 13, 7, F32)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        sc.render_frames_rays(dirs, cols, bos, poses=rows(names), origins=orgs, width=W, height=H, stream=s)  # eager
        s.synchronize()
        assert_frames([(as_bytes(c), as_bytes(b)) for c, b in zip(cols, bos)], want, F32, "eager")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            with pytest.raises(bh.BhError) as e:
                sc.render_frames_rays(small, [other], poses=rows(names[:1]), origins=small_o, width=13, height=7, stream=s)
            assert e.value.status == _abi.BH_ERR_UNSUPPORTED
            sc.render_frames_rays(dirs, cols, bos, poses=rows(names), origins=orgs, width=W, height=H, stream=s)
        for _ in range(2):
            for t in cols + bos:
                t.view(torch.uint8).fill_(SENTINEL)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert_frames([(as_bytes(c), as_bytes(b)) for c, b in zip(cols, bos)], want, F32, "replay")
            assert untouched(other) and guards_ok(*cols, *bos) and map_ok(dirs, orgs)
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
        ps[i] = _abi.bh_ray_pose.from_buffer_copy(oref.rows(n).tobytes())
    return ps


UNSUPPORTED = ["math", "layout", "shard_count", "partition", "pair", "persistent"]
DBG = ["dbg_n_rk", "dbg_fate", "dbg_steps"]
# with ss == 1 the dbg_* outputs are allowed (test_frames_of_distinct_poses); a lens render has no targets
REFUSALS = ([("bh_render_frames_rays_origins", w) for w in UNSUPPORTED] +
            [("bh_render_frames_rays_origins ss", w) for w in UNSUPPORTED + DBG] +
            [("bh_render_lens_rays_origins", w) for w in UNSUPPORTED + DBG + ["out_col", "out_blackout"]])


@pytest.mark.parametrize("entry,what", REFUSALS)
def test_refuses_unsupported(torch_cuda, scene, what, entry):
    """The offending field sits in the LAST desc of the call: every desc is checked."""
    torch = torch_cuda
    W, H = 40, 24
    fn = entry.split()[0]
    lens_entry, ss = fn == "bh_render_lens_rays_origins", 2 if entry.endswith("ss") else 1
    n = 1 if lens_entry else 2
    dirs, orgs = maps(torch, "equirect", "scatter", ss * W, ss * H)
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
        ps = _poses(oref.sequence(n))
        U, stream = C.byref(scene.uniforms.to_c()), torch.cuda.current_stream().cuda_stream
        lib, p, o = scene.lib, dirs.data_ptr(), orgs.data_ptr()
        if lens_entry:
            st = lib.bh_render_lens_rays_origins(scene._ctx, ps, U, descs, p, o, lens.data_ptr(), stream)
        else:
            st = lib.bh_render_frames_rays_origins(scene._ctx, n, ps, U, descs, p, o, ss, stream)
        assert st == _abi.BH_ERR_UNSUPPORTED
        text = lib.bh_last_error().decode()
        assert text.startswith(fn + ":") and text.endswith(".") and " " in text
        torch.cuda.synchronize()
        assert untouched(*cols, *bos, side, lens) and guards_ok(*cols, *bos)
        assert all((as_bytes(g) == SENTINEL).all() for g in lens_guard) and map_ok(dirs, orgs)
    finally:
        if part is not None:
            part.close()


def test_refuses_invalid_arguments(torch_cuda, scene):
    torch = torch_cuda
    W, H = 40, 24
    dirs, orgs = maps(torch, "equirect", "scatter", W, H)
    cols, bos = [target(torch, W, H, F32) for _ in range(2)], [target(torch, W, H, F32) for _ in range(2)]
    lens, lens_guard = guarded(torch, W * H, 8)
    U, stream = C.byref(scene.uniforms.to_c()), torch.cuda.current_stream().cuda_stream
    bad, ctx, lib = _abi.BH_ERR_INVALID_ARG, scene._ctx, scene.lib
    frames, lensp = lib.bh_render_frames_rays_origins, lib.bh_render_lens_rays_origins

    def descs(n=2, **kw):
        d = (_abi.bh_render_desc * n)()
        for i in range(n):
            d[i] = _desc(W, H, **{**dict(out_col=cols[i % 2].data_ptr(), out_blackout=bos[i % 2].data_ptr()), **kw})
        return d

    d, ld = descs(), _desc(W, H)
    ps = _poses(oref.sequence(4))
    many = _poses(oref.sequence(256) + oref.sequence(1))
    p, o, lp = dirs.data_ptr(), orgs.data_ptr(), lens.data_ptr()
    assert frames(ctx, 2, ps, U, d, p, None, 1, stream) == bad
    assert lib.bh_last_error().decode().startswith("bh_render_frames_rays_origins")
    assert lensp(ctx, ps, U, C.byref(ld), p, None, lp, stream) == bad
    assert lib.bh_last_error().decode().startswith("bh_render_lens_rays_origins")
    assert frames(ctx, 2, ps, U, d, None, o, 1, stream) == bad
    assert lensp(ctx, ps, U, C.byref(ld), None, o, lp, stream) == bad
    for off in (1, 2, 3):
        assert frames(ctx, 2, ps, U, d, p, o + off, 1, stream) == bad, off
        assert frames(ctx, 2, ps, U, d, p + off, o, 1, stream) == bad, off
        assert lensp(ctx, ps, U, C.byref(ld), p, o + off, lp, stream) == bad, off
        assert lensp(ctx, ps, U, C.byref(ld), p + off, o, lp, stream) == bad, off
    assert frames(ctx, 2, None, U, d, p, o, 1, stream) == bad
    assert frames(ctx, 2, ps, None, d, p, o, 1, stream) == bad
    assert frames(ctx, 2, ps, U, None, p, o, 1, stream) == bad
    assert frames(None, 2, ps, U, d, p, o, 1, stream) == bad
    assert lensp(ctx, None, U, C.byref(ld), p, o, lp, stream) == bad
    assert lensp(ctx, ps, U, C.byref(ld), p, o, None, stream) == bad
    assert lensp(ctx, ps, U, C.byref(ld), p, o, lp + 4, stream) == bad
    for n in (0, 257, 0xFFFFFFFF):
        assert frames(ctx, n, many, U, descs(1), p, o, 1, stream) == bad, n
    for ss in (0, 3, 5, 16, 0xFFFFFFFF):
        assert frames(ctx, 2, ps, U, d, p, o, ss, stream) == bad, ss
    for kw in (dict(width=0), dict(height=0), dict(width=65537), dict(max_iters=0), dict(max_iters=65536),
               dict(scene_flags=4), dict(format=3), dict(out_col=None), dict(math=2), dict(schedule=0x800)):
        assert frames(ctx, 2, ps, U, descs(**kw), p, o, 1, stream) == bad, kw
    for kw in (dict(width=W - 8), dict(max_iters=CAP - 1), dict(format=bh.BH_OUT_RGBA16F), dict(out_col=None)):
        two = descs()  # frames of one launch differ in their outputs alone
        two[1] = _desc(W, H, **{**dict(out_col=cols[1].data_ptr(), out_blackout=bos[1].data_ptr()), **kw})
        assert frames(ctx, 2, ps, U, two, p, o, 1, stream) == bad, kw
    for ss, (w, h) in ((2, (32769, 1)), (4, (1, 16385)), (8, (8193, 1))):
        one = (_abi.bh_render_desc * 1)(_desc(w, h, out_col=cols[0].data_ptr()))
        assert frames(ctx, 1, ps, U, one, p, o, ss, stream) == bad, (ss, w, h)
    for kw in (dict(width=0), dict(height=65537), dict(max_iters=0), dict(scene_flags=4)):
        assert lensp(ctx, ps, U, C.byref(_desc(W, H, **kw)), p, o, lp, stream) == bad, kw
    # the Python layer: the origin map's shape, dtype and place; origins without a pose
    good = rows(oref.sequence(2))
    half = torch.zeros((H, W, 3), dtype=torch.float16, device="cuda")
    for org in (orgs[:H - 1], orgs.cpu(), half, orgs.cpu().numpy(), orgs.transpose(0, 1)):
        with pytest.raises(bh.BhError) as e:
            scene.render_frames_rays(dirs, cols, bos, poses=good, origins=org, width=W, height=H)
        assert e.value.status == bad and "origins" in str(e.value)
    with pytest.raises(bh.BhError) as e:
        scene.render_frames_rays(dirs, cols, bos, poses=good, origins=orgs, ss=2, width=W, height=H)  # maps of ss 1
    assert e.value.status == bad
    with pytest.raises(bh.BhError) as e:
        scene.render_frames_rays(dirs, cols, bos, poses=None, origins=orgs, width=W, height=H)
    assert e.value.status == bad and "raymap.pose(pos)" in str(e.value)
    for kw in (dict(), dict(pos=(0.0, 0.0, -20.0))):
        with pytest.raises(bh.BhError) as e:
            scene.render_lens(lens.view(torch.float32), width=W, height=H, dirs=dirs, origins=orgs, **kw)
        assert e.value.status == bad and "raymap.pose(pos)" in str(e.value)
    with pytest.raises(bh.BhError) as e:
        scene.render_lens(lens.view(torch.float32), width=W, height=H, dirs=dirs, pose=good[0], origins=orgs[:H - 1])
    assert e.value.status == bad
    torch.cuda.synchronize()
    assert untouched(*cols, *bos, lens) and guards_ok(*cols, *bos) and map_ok(dirs, orgs)
    assert all((as_bytes(g) == SENTINEL).all() for g in lens_guard)
    assert frames(ctx, 2, ps, U, d, p, o, 1, stream) == _abi.BH_OK  # the arguments themselves are good
    assert lensp(ctx, ps, U, C.byref(ld), p, o, lp, stream) == _abi.BH_OK
    torch.cuda.synchronize()
    assert not untouched(cols[0]) and not untouched(lens) and guards_ok(*cols, *bos) and map_ok(dirs, orgs)
    assert all((as_bytes(g) == SENTINEL).all() for g in lens_guard)
